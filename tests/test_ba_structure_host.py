"""csrc/ba_structure.hpp - the host stages of pp_ba_create: layout of the variable intrinsics, the three CSRs, the internal image order and the column
positions, the tile map, the pair lists completed / ordered / cut into chunks, every list of the variable-intrinsics path - without a device and without
the library: the header compiles with plain g++ under ASan/UBSan (tests/ba_structure_host_driver.cpp), and for a corpus that reaches every branch every
scalar and the FNV-1a digest of every array equal tests/golden/ba_structure_digests.json.  That fixture was recorded from pp_ba_create as it was BEFORE
the stages moved into the header (one function in ba_eval.hip), with a throwaway patch that hashes the same host vectors right before the upload
(docs/HISTORY.md has the patch): the header builds, list by list, what that function built.  The structure has no reference counterpart (the reference
hands the problem to ceres::Solve, src/optim/bundle_adjustment.cc:273-306); what the lists must contain, the GPU tests check through the solves."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ba_structure_digests.json")
NUM_PARAMS = {0: 3, 1: 4, 2: 4, 3: 5, 4: 8, 5: 8, 6: 12, 7: 5, 8: 4, 9: 5, 10: 12}      # CameraNumParams (csrc/camera_models.hpp)


def _tracks(C, P, track):
    """point p is seen by the images (p + t) mod C, t < track: integer arithmetic only"""
    obs_point = np.repeat(np.arange(P, dtype=np.int32), track)
    obs_pose = ((obs_point + np.tile(np.arange(track, dtype=np.int32), P)) % C).astype(np.int32)
    return dict(C=C, P=P, obs_pose=obs_pose, obs_point=obs_point, pose_camera=np.zeros(C, dtype=np.int32), camera_model=np.array([2], dtype=np.int32))


def _covisibility(case):
    cov = np.zeros((case["C"], case["C"]), dtype=np.uint8)
    for p in range(case["P"]):
        seen = case["obs_pose"][case["obs_point"] == p]
        cov[np.ix_(seen, seen)] = 1
    return cov


def corpus():
    """name -> case: the arrays of a pp_ba_problem_desc (lines are (1, 0, (o mod 7) / 4)), the image order to use, the solver and the switches"""
    out = {}
    out["1_dense_small"] = _tracks(6, 60, 6)
    out["2_dense_long_lists"] = _tracks(12, 1500, 12)
    seq = _tracks(24, 96, 3)
    out["3_sequence"] = seq
    c, p = np.arange(24), np.arange(96)
    out["3a_constant_blocks"] = dict(seq, pose_const=(c % 7 == 3).astype(np.uint8), point_const=(p % 11 == 5).astype(np.uint8),
                                     tvec_const_mask=np.where(c % 5 == 0, c % 4, 0).astype(np.uint8))
    out["3b_same_image_pair"] = dict(seq, obs_pose=np.append(seq["obs_pose"], 0).astype(np.int32), obs_point=np.append(seq["obs_point"], 0).astype(np.int32))
    out["4_sparse_tiles"] = _tracks(96, 960, 3)
    out["4_permuted"] = dict(out["4_sparse_tiles"], new_of_old=(37 * np.arange(96) % 96).astype(np.int32))
    out["4a_permuted_constant_blocks"] = dict(out["3a_constant_blocks"], new_of_old=(7 * c % 24).astype(np.int32))      # (the per-image masks move with their images)
    shared = dict(seq, camera_model=np.array([2, 2], dtype=np.int32), camera_const_mask=np.array([0b0110, 0], dtype=np.uint16))
    out["5a_shared_camera"] = shared
    own = dict(seq, pose_camera=((5 * c) % 24).astype(np.int32), camera_model=np.full(24, 2, dtype=np.int32))
    out["5b_private_wide"] = dict(own, camera_const_mask=np.full(24, 0b0110, dtype=np.uint16), nv_private=2)
    out["5b_private_general"] = dict(out["5b_private_wide"], ba_intr_wide=0)
    out["5c_private_tail"] = dict(own, camera_const_mask=np.full(24, 0b0100, dtype=np.uint16))
    out["6_iterative"] = dict(seq, iterative=1)
    out["6_iterative_shared_camera"] = dict(shared, iterative=1)
    half = seq["obs_point"] < 48
    shard = dict(seq, obs_pose=seq["obs_pose"][half], obs_point=seq["obs_point"][half], covisibility=_covisibility(seq))
    out["7_shard_of_a_group"] = shard
    out["7_permuted_shard"] = dict(shard, new_of_old=(7 * c % 24).astype(np.int32), pose_const=(c % 7 == 3).astype(np.uint8))      # (the matrix is walked in the caller's order)
    cleared = shard["covisibility"].copy()
    cleared[5, 4] = cleared[4, 5] = 0
    out["7_matrix_not_the_union"] = dict(shard, covisibility=cleared)
    return out


def case_text(name, case):
    """the case as tests/ba_structure_host_driver.cpp reads it (absent per-image arrays as zeros and camera_const_mask as all-constant: what
    privacy_preserving_sfm_amd.device._ba_desc passes to pp_ba_create)"""
    C, P, K = case["C"], case["P"], len(case["camera_model"])
    tok = ["case", name, C, P, K, len(case["obs_pose"]), case.get("iterative", 0), case.get("nv_private", 0), 1, case.get("ba_intr_wide", 1), 1, 1]
    tok += list(case["obs_pose"]) + list(case["obs_point"]) + list(case["pose_camera"]) + list(case["camera_model"]) + [NUM_PARAMS[int(m)] for m in case["camera_model"]]
    for key, n, default in (("pose_const", C, 0), ("tvec_const_mask", C, 0), ("point_const", P, 0), ("camera_const_mask", K, 0xFFFF)):
        tok += [1] + list(case.get(key, np.full(n, default)))
    for key in ("covisibility", "new_of_old"):
        tok += [0] if case.get(key) is None else [1] + list(np.asarray(case[key]).ravel())
    return " ".join(str(int(t)) if not isinstance(t, str) else t for t in tok)


def parse(text):
    """{case: {"scalars": {name: int}, "arrays": {name: [length, digest]}, "refused": text or None}} of the driver's (and the recording patch's) output"""
    cases, cur = {}, None
    for line in text.splitlines():
        tok = line.split(" ", 1)
        if tok[0] == "case":
            cur = cases.setdefault(tok[1], {"scalars": {}, "arrays": {}, "refused": None})
        elif tok[0] == "scalar":
            cur["scalars"][tok[1].split()[0]] = int(tok[1].split()[1])
        elif tok[0] == "array":
            cur["arrays"][tok[1].split()[0]] = [int(tok[1].split()[1]), tok[1].split()[2]]
        elif tok[0] == "refused":
            cur["refused"] = tok[1]
    return cases


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the driver's output for the whole corpus; built with every warning on, run with the sanitizers on"""
    exe = str(tmp_path_factory.mktemp("ba_structure") / "ba_structure_host_driver")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                         os.path.join(ROOT, "tests", "ba_structure_host_driver.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0 and not cc.stderr.strip(), cc.stderr      # no warning either
    text = "\n".join(case_text(name, case) for name, case in corpus().items()) + "\n"
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and not out.stderr.strip(), out.stderr[-4000:]      # the sanitizers stay silent
    return parse(out.stdout)


def test_every_list_is_what_pp_ba_create_built_before_the_split(built):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(built) == sorted(golden) == sorted(corpus())
    for name, want in golden.items():
        got = built[name]
        assert got["refused"] == want["refused"], name
        assert got["scalars"] == want["scalars"], name
        assert sorted(got["arrays"]) == sorted(want["arrays"]), name
        for array, digest in want["arrays"].items():
            assert got["arrays"][array] == digest, (name, array)
    assert sum(len(g["arrays"]) for g in golden.values()) == 42 * (len(golden) - 1)      # (every array of BaStructure, for every case that is not refused)


def test_the_corpus_reaches_every_branch(built):
    s = {name: got["scalars"] for name, got in built.items()}
    n = {name: {k: v[0] for k, v in got["arrays"].items()} for name, got in built.items()}
    one = s["1_dense_small"]
    assert (one["pairs_chunked"], one["chunk_len"], one["pairs_complete"], one["sparse_tiles"]) == (1, 8, 1, 0) and one["small_num_chunks"] == 15 * 8 < 1280
    two = s["2_dense_long_lists"]      # 99 000 entries in lists of 1500: chunks of 16, enough of them for the XCD order
    assert (two["num_entries"], two["pairs_chunked"], two["chunk_len"], two["small_num_chunks"]) == (99000, 1, 16, 6204) and two["small_num_chunks"] >= 1280
    three = s["3_sequence"]      # 24 images in a ring, each sharing points with two neighbours on either side: 48 lists, 276 with the empty ones
    assert (three["pairs_chunked"], three["pairs_complete"], three["num_pairs"], three["NI"]) == (0, 1, 24 * 23 // 2, 0) and n["3_sequence"]["small_chunk"] == 0
    const = s["3a_constant_blocks"]
    assert const["num_effective_pose_point"] < three["num_effective_pose_point"] and const["num_pairs"] < three["num_pairs"] and const["pairs_complete"] == 1
    same = s["3b_same_image_pair"]
    # (image 0 sees point 0 twice: both orders of the pair of its own two observations, and one more entry each with images 1 and 2)
    assert (three["num_entries"], same["pairs_complete"], same["num_pairs"], same["num_entries"]) == (96 * 3, 0, 48 + 1, 96 * 3 + 2 + 2)
    assert (s["4_sparse_tiles"]["sparse_tiles"], s["4_sparse_tiles"]["reordered"], s["4_permuted"]["reordered"]) == (1, 0, 1)
    moved, shard = s["4a_permuted_constant_blocks"], s["7_permuted_shard"]      # the same counts as in the caller's order, other arrays
    assert (moved["reordered"], moved["num_pairs"], moved["num_effective_pose_point"]) == (1, const["num_pairs"], const["num_effective_pose_point"])
    assert built["4a_permuted_constant_blocks"]["arrays"]["pose_const"] != built["3a_constant_blocks"]["arrays"]["pose_const"]
    assert (shard["reordered"], shard["pairs_complete"], shard["num_pairs"]) == (1, 1, 21 * 20 // 2) and built["7_permuted_shard"]["refused"] is None
    assert s["4_sparse_tiles"]["n_red"] == 576 and n["4_sparse_tiles"]["tile_nz"] == 10 * 10 and s["4_sparse_tiles"]["pairs_complete"] == 0
    shared = s["5a_shared_camera"]      # one block of two variable parameters (the second block is referenced by no image): factored lists + the diagonal's
    assert (shared["NI"], shared["nv_private"], shared["kk_num_groups"], shared["gen_num_groups"]) == (2, 0, 96, 96) and shared["gen_num_pairs"] == 24
    wide, general, tail = s["5b_private_wide"], s["5b_private_general"], s["5c_private_tail"]
    assert (wide["intr_wide_nv"], wide["nv_private"], wide["gen_num_pairs"], wide["n_red"]) == (2, 2, 0, 24 * 8)
    assert (general["intr_wide_nv"], general["nv_private"]) == (0, 2) and general["gen_num_pairs"] > 0
    assert (tail["nv_private"], tail["NI"], tail["nv_widest"]) == (0, 24 * 3, 3) and tail["gen_num_pairs"] > 0
    for name in ("6_iterative", "6_iterative_shared_camera"):
        assert (s[name]["iterative"], s[name]["num_pairs"], s[name]["num_entries"], n[name]["pair_start"], n[name]["pair_ij"]) == (1, 0, 0, 2, 0), name
    assert s["6_iterative_shared_camera"]["gen_num_groups"] == 96 and s["6_iterative_shared_camera"]["gen_num_pairs"] == 1 and s["6_iterative"]["gen_num_pairs"] == 0
    assert n["6_iterative_shared_camera"]["gen_entries"] == 96 + 1 + 288 and n["6_iterative_shared_camera"]["kk_entries"] == 0
    assert built["7_shard_of_a_group"]["refused"] is None and s["7_shard_of_a_group"]["num_pairs"] == 276      # (complete: the empty lists of the other shard's pairs too)
    assert built["7_matrix_not_the_union"]["refused"] == (
        "pp_ba_create: images 5 and 4 share a point of this shard but pp_ba_problem_desc::covisibility has no entry for them - the matrix must be "
        "the union over the group's shards (pp_ba_covisibility of every rank, element-wise MAX)")


def test_private_columns_are_not_the_identity(built):
    """5b: every image carries its two variable intrinsics beside its pose columns (image i's camera is block 5 i mod 24) - spos, the same with and without
    the wide blocks, is not the identity of its length"""
    a = built["5b_private_wide"]["arrays"]["spos"]
    assert a[0] == 24 * 8 and a == built["5b_private_general"]["arrays"]["spos"]
    ident = np.arange(24 * 8, dtype=np.int32).tobytes()
    h = 1469598103934665603
    for b in ident:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert a[1] != "%016x" % h
