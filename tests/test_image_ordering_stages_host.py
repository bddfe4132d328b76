"""csrc/image_ordering.hpp - the stages of the image ordering (Cuthill-McKee, the band and graph dissectors with their memo tables, the co-visibility graph
from its three sources, the tile map of an order, the whole ChooseImageOrdering with the planner alone as its verifier) - without a device and without the
library: the header compiles with plain g++ under ASan/UBSan (tests/image_ordering_host_driver.cpp).  The driver checks what has a structural definition
(permutations, no edge across a cut, aligned parts, isolated vertices last, memoised objects) and exits on a violation; what it prints - tile maps,
adjacencies, an order - is compared here with brute-force numpy counterparts and with pp_ba_plan_ordering.  The graphs are the smallest a dissector still
cuts: Grain(6) looks at 69 images and more, Grain(8) at 53."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def graphs():
    """name -> (C, [(u, v)])"""
    path = [(i, i + 1) for i in range(69)]
    clique = lambda ids: [(a, b) for i, a in enumerate(ids) for b in ids[:i]]
    left, right, bridge = list(range(40)), list(range(40, 80)), [80, 81, 82]      # two cliques of 40 joined by 3 images that see both
    out = {"path70": (70, path), "ring70": (70, path + [(69, 0)])}
    out["bridged_cliques"] = (83, clique(left) + clique(right) + [(b, v) for b in bridge for v in left[:6] + right[:6]])
    out["joined_cliques"] = (80, clique(left) + clique(right) + [(a, b) for a in left[:3] for b in right[:3]])      # no image apart: three of either clique see the other's three
    spread = [i + i // 10 for i in range(70)]      # the path on 77 ids, every eleventh id (10, 21, ...) without a neighbour
    out["path70_isolated"] = (77, [(spread[a], spread[b]) for a, b in path])
    return out


def scenes():
    """name -> dict(C, obs_pose, obs_point, pose_const, point_const): a point per edge seen by its two images (three images for every fifth point)"""
    def of(C, edges, fixed=(), const_every=0):
        obs_pose, obs_point = [], []
        for p, (u, v) in enumerate(edges):
            seen = [u, v] + ([(u + 2) % C] if p % 5 == 0 else [])
            obs_pose += seen; obs_point += [p] * len(seen)
        pose_const = np.zeros(C, dtype=np.uint8); pose_const[list(fixed)] = 1
        point_const = np.zeros(len(edges), dtype=np.uint8)
        if const_every:
            point_const[::const_every] = 1
        return dict(C=C, P=len(edges), obs_pose=np.array(obs_pose, dtype=np.int32), obs_point=np.array(obs_point, dtype=np.int32), pose_const=pose_const, point_const=point_const)
    band = [(i, i + k) for i in range(150) for k in range(1, 6) if i + k < 150]
    out = {"band150": of(150, band, fixed=(0, 17, 18, 90), const_every=7)}
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(out["band150"]["obs_pose"]))      # observations not grouped by point
    out["band150_unsorted"] = dict(out["band150"], obs_pose=out["band150"]["obs_pose"][perm], obs_point=out["band150"]["obs_point"][perm])
    out["clique83"] = of(83, [(a, b) for a in range(83) for b in range(a)], fixed=(0,))
    return out


def covisible(sc):
    """C x C bool: two variable images share a variable point"""
    C = sc["C"]
    A = np.zeros((C, C), dtype=bool)
    for p in range(sc["P"]):
        if sc["point_const"][p]:
            continue
        seen = [c for c in sc["obs_pose"][sc["obs_point"] == p] if not sc["pose_const"][c]]
        A[np.ix_(seen, seen)] = True
    np.fill_diagonal(A, False)
    return A


def bits_of(A):
    C = A.shape[0]
    W = (C + 63) // 64
    bits = np.zeros((C, W), dtype=np.uint64)
    for i, j in zip(*np.nonzero(np.tril(A, -1))):
        bits[i, j >> 6] |= np.uint64(1) << np.uint64(j & 63)
    return bits


def driver_input():
    lines = []
    for name, (C, edges) in graphs().items():
        lines.append(" ".join(map(str, ["graph", name, C, len(edges)] + [x for e in edges for x in e])))
    for name, sc in scenes().items():
        A = covisible(sc)
        tok = ["scene", name, sc["C"], sc["P"], len(sc["obs_pose"])]
        for a in (sc["obs_pose"], sc["obs_point"], sc["pose_const"], sc["point_const"], A.astype(np.uint8).ravel(), bits_of(A).ravel()):
            tok += [int(x) for x in a]
        lines.append(" ".join(map(str, tok)))
    return "\n".join(lines) + "\n"


def parse(text):
    """{("graph" | "scene", name): {key: [token lists]}}"""
    out, cur = {}, None
    for line in text.splitlines():
        tok = line.split()
        if tok[0] in ("graph", "scene"):
            cur = out.setdefault((tok[0], tok[1]), {})
        elif tok[0] != "end":
            cur.setdefault(tok[0], []).append(tok[1:])
    return out


@pytest.fixture(scope="module")
def driven(tmp_path_factory):
    """the driver's output; built with every warning on (-O0: the run takes a tenth of a second, the optimiser would take ten), run with the sanitizers on"""
    exe = str(tmp_path_factory.mktemp("image_ordering") / "image_ordering_host_driver")
    cc = subprocess.run(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                         os.path.join(ROOT, "tests", "image_ordering_host_driver.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0 and not cc.stderr.strip(), cc.stderr      # no warning either
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input=driver_input(), capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and not out.stderr.strip(), out.stderr[-4000:]      # every structural check holds and the sanitizers stay silent
    return parse(out.stdout)


def test_the_header_is_std_only():
    """plain g++, every warning an error, and no HIP header among what it includes"""
    src = '#include "%s"\n' % os.path.join(ROOT, "privacy_preserving_sfm_amd", "csrc", "image_ordering.hpp")
    cc = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    deps = subprocess.run(["g++", "-std=c++17", "-M", "-x", "c++", "-"], input=src, capture_output=True, text=True).stdout.replace("\\\n", " ").split()
    ours = sorted(os.path.basename(p) for p in deps if not p.endswith(":") and os.path.realpath(p).startswith(ROOT))
    assert ours == ["ba_structure.hpp", "chol_plan.hpp", "image_ordering.hpp", "ppsfm_hip.h", "switches.hpp"], ours
    assert not [p for p in deps if "/hip/" in p or "rocm" in p]


def test_the_graphs_are_cut(driven):
    """(the structural checks ran in the driver; here: they were not vacuous) every graph takes a band cut under both grains, the paths, the ring and the
    joined cliques a cut of the graph dissector too; isolated vertices end every Cuthill-McKee order"""
    for name in graphs():
        got = driven[("graph", name)]
        assert {int(w): int(n) for w, n in got["band_cuts"]} .keys() == {6, 8}
        assert all(int(n) > 0 for w, n in got["band_cuts"] if int(w) == 8), (name, got["band_cuts"])
    # (a level structure rooted at a bridge image - the vertex of smallest degree - has nothing on its near side: the bridged cliques are cut as a band only)
    for name in ("path70", "ring70", "path70_isolated", "joined_cliques"):
        assert all(int(n) >= 2 for _, n in driven[("graph", name)]["graph_parts"]), name
    assert all(int(n) > 0 for _, n in driven[("graph", "path70")]["band_cuts"] + driven[("graph", "ring70")]["band_cuts"])
    rcm = [int(x) for x in driven[("graph", "path70_isolated")]["rcm"][0]]
    assert rcm[-7:] == [10, 21, 32, 43, 54, 65, 76]


def _closed_tiles(C, edges, NI, nv_private, pos):
    """the brute-force tile map: every column of an image against every column of its neighbours and itself, the tail and the right-hand side's row against
    everything before them, closed under the fill-in of a symbolic factorisation"""
    W6, n_red = 6 + nv_private, 6 * C + NI
    T = (n_red + 1 + 63) // 64
    cols = lambda c: W6 * pos[c] + np.arange(W6)
    nz = np.zeros((T, T), dtype=bool)
    for u, v in list(edges) + [(c, c) for c in range(C)]:
        r, c = np.meshgrid(cols(u) // 64, cols(v) // 64)
        nz[r, c] = True; nz[c, r] = True
    nz[(W6 * C) // 64:, :] = True      # (from the first tail column - or, without a tail, the right-hand side's row - down)
    nz = np.tril(nz)
    for k in range(T):
        rows = np.flatnonzero(nz[k + 1:, k]) + k + 1
        nz[np.ix_(rows, rows)] = True
    return np.tril(nz)


def test_tile_maps_against_a_brute_force_map(driven):
    for name, (C, edges) in graphs().items():
        got = driven[("graph", name)]
        rcm = np.array([int(x) for x in got["rcm"][0]])
        noo = np.empty(C, dtype=int); noo[rcm] = np.arange(C)
        assert len(got["tiles"]) == 6
        for NI, nvp, order, T, nnz, text in got["tiles"]:
            want = _closed_tiles(C, edges, int(NI), int(nvp), np.arange(C) if order == "natural" else noo)
            have = np.array([ch == "1" for ch in text]).reshape(int(T), int(T))
            assert want.shape == have.shape and np.array_equal(np.tril(have), want) and int(nnz) == want.sum(), (name, NI, nvp, order)


def test_the_three_sources_give_one_graph(driven):
    for name, sc in scenes().items():
        got = driven[("scene", name)]
        A = covisible(sc)
        want = sorted((int(i), int(j)) for i, j in zip(*np.nonzero(np.tril(A, -1))))
        assert [src for src, *_ in got["adj"]] == ["observations", "bits", "matrix"]
        for src, *flat in got["adj"]:
            assert sorted(zip(map(int, flat[0::2]), map(int, flat[1::2]))) == want, (name, src)
    assert covisible(scenes()["band150"])[17].sum() == 0 and covisible(scenes()["band150"])[19].sum() > 0      # (a constant pose is no node)


def test_the_whole_ordering_is_the_librarys(driven):
    """ChooseImageOrdering with PlanAndList as its verifier = pp_ba_plan_ordering (CholeskyChainSteps through the plan cache) on the same scene; a clique
    leaves through the dense early exit"""
    from privacy_preserving_sfm_amd.device import plan_ordering
    for name, sc in scenes().items():
        dense_exit, nnz_natural, nnz_ordered, chains, steps, verified = (int(x) for x in driven[("scene", name)]["ordering"][0])
        oon = [int(x) for x in driven[("scene", name)]["old_of_new"][0]]
        C, P, M = sc["C"], sc["P"], len(sc["obs_pose"])
        scene = dict(poses=np.zeros((C, 7)), points=np.zeros((P, 3)), intr=np.zeros((1, 4)), lines=np.zeros((M, 3)), obs_pose=sc["obs_pose"], obs_point=sc["obs_point"],
                     pose_camera=np.zeros(C, dtype=np.int32), camera_model=np.array([2], dtype=np.int32), pose_const=sc["pose_const"], point_const=sc["point_const"])
        lib_oon, info = plan_ordering(scene, linear_solver=1)
        assert (oon or list(range(C))) == lib_oon.tolist(), name
        if name == "clique83":
            assert dense_exit == 1 and not oon and nnz_natural == -1 == info["nnz_natural"] and verified == 0
        else:
            assert dense_exit == 0 and info["reordered"] and chains >= 2 and verified == 1, (name, chains, verified)
            assert (nnz_natural, nnz_ordered, chains, steps) == (info["nnz_natural"], info["nnz_used"], info["chains"], info["chain_steps"]), name
