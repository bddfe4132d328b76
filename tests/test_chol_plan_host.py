"""csrc/chol_plan.hpp - the task planner of the one-launch Cholesky factorisation - without a device and without the library: the header compiles
with plain g++ under ASan/UBSan (tests/chol_plan_host_driver.cpp), and for the structures tests/test_cholesky_task_order.py generates its chains, time,
rho1, closed map, replay verdict and 16-word task list are what the built library returns through pp_cholesky_task_list / pp_cholesky_task_plan.  The
schedule itself has no reference counterpart (it replaces the linear solve inside ceres::Solve, reference src/optim/bundle_adjustment.cc:273-306); what
a correct list is, test_cholesky_task_order.py checks with its own replay."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import test_cholesky_task_order as order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import chol_plan_digest as digest      # noqa: E402  (the corpus and the calls of the three probes)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """the driver's output for the whole corpus: ({name: fields}, the header lines); built with every warning on, run with the sanitizers on"""
    exe = str(tmp_path_factory.mktemp("chol_plan") / "chol_plan_host_driver")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                         os.path.join(ROOT, "tests", "chol_plan_host_driver.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0 and not cc.stderr.strip(), cc.stderr      # no warning either
    lines = []
    for name, T, max_chains, nz in digest.corpus():
        bits = "dense" if nz is None else "".join("1" if v else "0" for v in np.asarray(nz, dtype=np.uint8).ravel())
        lines.append("%s %d %d %s" % (name, T, max_chains, bits))
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=1500, env=env)
    assert out.returncode == 0 and not out.stderr.strip(), out.stderr[-4000:]      # the sanitizers stay silent
    head, structs, cur = {}, {}, None
    for line in out.stdout.splitlines():
        tok = line.split()
        if tok[0] in ("layout", "packed", "wsconst"):
            head[tok[0]] = tok[1:]
        elif tok[0] == "ws":
            head.setdefault("ws", []).append([int(t) for t in tok[1:]])
        elif tok[0] == "struct":
            cur = structs.setdefault(tok[1], {"T": int(tok[2]), "tasks": []})
        elif tok[0] == "end":
            cur = None
        elif tok[0] == "map":
            cur["map"] = tok[1]
        elif tok[0] in ("chains", "steps", "time", "rho1", "verified", "sparse"):
            cur[tok[0]] = [int(t) for t in tok[1:]]
        elif tok[0] == "tasks":
            cur["count"] = int(tok[1])
        else:
            cur["tasks"].append([int(t) for t in tok])
    return structs, head


@pytest.fixture
def default_switches(monkeypatch):
    for name in list(os.environ):
        if name.startswith("PPSFM_CHOL_"):
            monkeypatch.delenv(name)


def test_counter_layout_and_packed_fields(dump):
    """the layout the header gives the device's counters is the one the independent replay of test_cholesky_task_order.py spells out, and the accessors
    undo the pack functions (b = J | part << 8 | parts << 12 | target << 16, flags = first | chain << 4: csrc/chol_plan.hpp)"""
    layout = dict(zip(dump[1]["layout"][0::2], (int(v) for v in dump[1]["layout"][1::2])))
    assert (layout["cSol0"], layout["kMaxSteps"], layout["kMaxSuper"], layout["kMaxChains"]) == (order.C_SOL0, order.MAX_STEPS, order.MAX_SUPER, 16)
    assert (layout["cVer0"], layout["cSub0"]) == (order.C_VER0, order.C_SUB0)
    assert layout["cScratch0"] == order.C_SUB0 + order.MAX_SUPER * order.MAX_SUPER and layout["kPartsTwoPanels"] == 8
    assert dump[1]["packed"] == ["64", "3", "8", "1234", "1", "15", "b", str(64 | 3 << 8 | 8 << 12 | 1234 << 16), "flags", str(1 | 15 << 4)]


def test_workspace_layout(dump):
    """CholWorkspace (csrc/chol_plan.hpp), the one description of the Cholesky workspace, for T = 1 .. 160 block columns (both sides of kMaxSteps = 128):
    the parts follow each other without overlap - M[T], X[T+1], D[T+1], solved X[T+1] in 64 x 64 tiles, the counters, the pair inverses [npairs] and
    pair couplings [4 npairs] - tiles start on tile boundaries, the counter part holds kNumCounters int32, the pairs end inside the total, and the total
    is the size every caller has allocated so far, written out"""
    const = dict(zip(dump[1]["wsconst"][0::2], (int(v) for v in dump[1]["wsconst"][1::2])))
    tile = 64 * 64
    assert const["kTile"] == tile and const["kNumCounters"] * 4 <= const["kCounterDoubles"] * 8
    rows = dump[1]["ws"]
    assert [r[0] for r in rows] == list(range(1, 161))
    for T, Minv, xs, ds, xsol, counters, Pw, Zw, total, mail, npairs in rows:
        assert npairs == ((T - 3) // 2 if T >= 7 else 0), T
        starts = [Minv, xs, ds, xsol, counters, Pw, Zw]
        sizes = [T * tile, (T + 1) * tile, (T + 1) * tile, (T + 1) * tile, const["kCounterDoubles"], npairs * tile, 4 * npairs * tile]
        assert Minv == 0 and all(s % tile == 0 for s in starts), T
        assert all(a < b for a, b in zip(starts[:5], starts[1:5] + [Pw])) and Pw <= Zw, T      # increasing (Pw == Zw where there are no pairs)
        for (a, n), b in zip(zip(starts, sizes), starts[1:] + [total]):      # disjoint: every part ends where the next one starts, or before
            assert a + n <= b, T
        assert mail == counters == (4 * T + 3) * tile, T      # the mailbox slots k_potrf64 presets
        assert Pw + 5 * npairs * tile <= total, T
        assert total == (4 * T + 3) * 4096 + 8192 + (T // 2 + 1) * 5 * 4096, T


def test_header_plans_what_the_library_plans(dump, default_switches):
    from privacy_preserving_sfm_amd import _capi
    L = _capi.lib()
    structs = dump[0]
    corpus = digest.corpus()
    assert len(structs) == len(corpus)
    for name, T, max_chains, nz in corpus:
        got = structs[name]
        assert got["T"] == T and got["count"] == len(got["tasks"]) > 0, name
        mine = np.asarray(got["tasks"], dtype=np.int32).reshape(-1, 16)
        if nz is None:      # the list of a dense solve: type, k, a, b of every task
            assert np.array_equal(mine[:, :4], digest.dense_list(L, T)), name
            assert got["map"] == "dense" and got["chains"] == [1, 0, T, 0] and got["steps"] == [T], name
            continue
        tasks, m, chains, time, rho1, ok = digest.plan(L, T, nz, max_chains)
        assert np.array_equal(mine, tasks), name
        assert got["map"] == "".join("1" if v else "0" for v in m.ravel()), name
        n = int(chains[0])
        assert got["chains"] == [n] + [int(v) for v in chains[1:1 + 3 * n]], name
        assert got["time"] == list(time) and got["rho1"] == list(rho1) and got["verified"] == [ok], name
        assert got["steps"] == [int(max(time)) + 1], name
        if max_chains == 1:
            t7, m7 = digest.one_chain_list(L, T, nz)
            assert np.array_equal(mine[:, :7], t7) and np.array_equal(m7, m), name


def test_replay_verdicts(dump):
    """the host replay accepts every list of the corpus but the one whose scratch sequences outnumber the counter pool: eight chains no, one chain yes"""
    structs = dump[0]
    for name, got in structs.items():
        assert got["verified"] == [0 if name == "overflow" else 1], name
    assert structs["overflow"]["chains"][0] == 8 and structs["overflow_one_chain"]["chains"][0] == 1
    assert sum(1 for name, got in structs.items() if name.startswith("forest") and got["chains"][0] > 1) >= 4


def test_sparse_column_lists(dump):
    """the lists of the block-sparse per-column launches, recomputed here from their definition (k_column_step): launch k has a solve workgroup per
    non-zero tile (i,k), i >= k + 3, and an update workgroup per super-tile u - TriIndex(u + 1) = (I, J) in the region below (k+1,k+1) - one of whose
    tiles panel k-1 couples"""
    for name, T, max_chains, nz in digest.corpus():
        if nz is None or max_chains == 1:
            continue
        has = np.array(nz, dtype=np.uint8)
        for k in range(T):      # closed under fill-in: what the driver handed BuildSparseColumnLists
            rows = [i for i in range(k + 1, T) if has[i, k]]
            for a in rows:
                for b in rows:
                    if b <= a:
                        has[a, b] = 1
        rows, sups, row_off, sup_off = [], [], [], []
        for k in range(T - 1):
            row_off.append(len(rows)); sup_off.append(len(sups))
            rows += [i for i in range(k + 3, T) if has[i, k]]
            if k >= 1:
                k1 = k + 1
                ns = (T - k1 + 1) // 2
                for u in range(ns * (ns + 1) // 2 - 1):
                    I = (math.isqrt(8 * (u + 1) + 1) - 1) // 2
                    J = u + 1 - I * (I + 1) // 2
                    tiles = [(k1 + 2 * I + (q >> 1), k1 + 2 * J + (q & 1)) for q in range(4)]
                    if any(bi < T and bj < T and bi >= bj and has[bi, k - 1] and has[bj, k - 1] for bi, bj in tiles):
                        sups.append(u)
        row_off += [len(rows)] * 2; sup_off += [len(sups)] * 2
        got = dump[0][name]["sparse"]
        assert got[:2] == [2 * (T + 1), 2 * (T + 1) + len(rows)], name
        assert got[2:] == row_off + sup_off + rows + sups, name
