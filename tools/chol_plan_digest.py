#!/usr/bin/env python3
"""One SHA-256 per structure over what the Cholesky task planner makes of it: closed tile map, chain ranges, time, rho1, the replay's verdict and the task
words - taken through the three public probes (pp_cholesky_task_list, pp_cholesky_task_list_sparse, pp_cholesky_task_plan) and nothing else, so the
same file runs against any build of the library:

    python tools/chol_plan_digest.py [--lib path/to/libppsfm_hip.so]

The corpus (`corpus()`, shared with tests/test_chol_plan_host.py) is what tests/test_cholesky_task_order.py generates: dense lists, bands, arrows,
dissected maps, several-chain leaves, random forests, the scratch-counter overflow case.  It is walked once under the default switches and once under each
of a few planner switches (PPSFM_CHOL_CHAINS=1, PPSFM_CHOL_TWO_PANELS=0, PPSFM_CHOL_WHOLE_FROM=6, PPSFM_CHOL_SLOPE=0.5), a fresh process each; two builds
plan alike exactly when their outputs are equal line for line.  (A dense list comes through pp_cholesky_task_list, which shows type, k, a, b of a task;
every mapped structure shows all 16 words.)  No GPU is needed."""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SETTINGS = [{}, {"PPSFM_CHOL_CHAINS": "1"}, {"PPSFM_CHOL_TWO_PANELS": "0"}, {"PPSFM_CHOL_WHOLE_FROM": "6"}, {"PPSFM_CHOL_SLOPE": "0.5"}]
DENSE_T = [4, 5, 6, 7, 8, 13, 24, 47, 48, 63, 64, 94, 128]


def corpus(forests_per_seed=12):
    """-> [(name, T, max_chains, tile map or None)]; None: the dense list of T block columns; max_chains 0: as many as the structure has"""
    import test_cholesky_task_order as g
    out = [("dense%d" % T, T, 0, None) for T in DENSE_T]
    maps = [("densemap%d" % T, T, np.tril(np.ones((T, T), dtype=np.uint8))) for T in (4, 47, 48, 128)]
    maps += [("band1_8", 8, g._band(8, 1)), ("band1_24", 24, g._band(24, 1)), ("band4_47", 47, g._band(47, 4)), ("band9_47", 47, g._band(47, 9)),
             ("band6_128", 128, g._band(128, 6)), ("arrow48", 48, g._arrow(48, 3, 2)), ("arrow64", 64, g._arrow(64, 3, 2)),
             ("dissected47", 47, g._dissected(47, 3, 4)), ("dissected94", 94, g._dissected(94, 3, 4)),
             ("two_leaves", 47, g._leaves(47, [21, 21], 3, 5)), ("uneven_leaves", 47, g._leaves(47, [9, 30], 4, 8)),
             ("four_leaves", 47, g._leaves(47, [9, 9, 9, 9], 2, 11)), ("two_level", 47, g._two_level(47, 6, 2, 5, 13)),
             ("odd_boundaries", 40, g._leaves(40, [7, 11, 13], 3, 9)), ("overflow", 128, g._leaves(128, [10] * 8, 2, 48))]
    for name, T, nz in maps:
        out += [(name, T, 0, nz), (name + "_one_chain", T, 1, nz)]
    for seed in range(8):
        rng = np.random.default_rng(1000 + seed)
        for i in range(forests_per_seed):
            T = int(rng.integers(12, 100))
            out.append(("forest%d_%d" % (seed, i), T, 0, g._random_forest(rng, T)))
    return out


def load(path=None):
    if path is None:
        from privacy_preserving_sfm_amd import _capi
        return _capi.lib()
    L = C.CDLL(path)
    u8p, i32p, i64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    L.pp_cholesky_task_list.argtypes = [C.c_int32, i32p, C.c_int64, i64p]
    L.pp_cholesky_task_list_sparse.argtypes = [C.c_int32, u8p, u8p, i32p, C.c_int64, i64p]
    L.pp_cholesky_task_plan.argtypes = [C.c_int32, u8p, C.c_int32, u8p, i32p, C.c_int64, i64p, i32p, i32p, i32p, i32p]
    return L


_u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
_i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))


def dense_list(L, T):
    n = C.c_int64(0)
    assert L.pp_cholesky_task_list(T, None, 0, C.byref(n)) == 0
    buf = np.zeros(4 * n.value, dtype=np.int32)
    assert L.pp_cholesky_task_list(T, _i32(buf), n.value, C.byref(n)) == 0
    return buf.reshape(-1, 4)


def one_chain_list(L, T, nz):
    n = C.c_int64(0)
    nz = np.ascontiguousarray(nz, dtype=np.uint8)
    m = np.zeros((T, T), dtype=np.uint8)
    assert L.pp_cholesky_task_list_sparse(T, _u8(nz), _u8(m), None, 0, C.byref(n)) == 0
    buf = np.zeros(7 * n.value, dtype=np.int32)
    assert L.pp_cholesky_task_list_sparse(T, _u8(nz), _u8(m), _i32(buf), n.value, C.byref(n)) == 0
    return buf.reshape(-1, 7), m


def plan(L, T, nz, max_chains):
    """-> (tasks [n, 16], closed map, chains [49], time, rho1, verified)"""
    n, ok = C.c_int64(0), C.c_int32(0)
    nz = np.ascontiguousarray(nz, dtype=np.uint8)
    m, chains = np.zeros((T, T), dtype=np.uint8), np.zeros(49, dtype=np.int32)
    time, rho1 = np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int32)
    assert L.pp_cholesky_task_plan(T, _u8(nz), max_chains, _u8(m), None, 0, C.byref(n), _i32(chains), _i32(time), _i32(rho1), C.byref(ok)) == 0
    buf = np.zeros(16 * n.value, dtype=np.int32)
    assert L.pp_cholesky_task_plan(T, _u8(nz), max_chains, _u8(m), _i32(buf), n.value, C.byref(n), _i32(chains), _i32(time), _i32(rho1), C.byref(ok)) == 0
    return buf.reshape(-1, 16), m, chains, time, rho1, int(ok.value)


def digest(L, T, max_chains, nz):
    h = hashlib.sha256()
    if nz is None:
        tasks = dense_list(L, T)
        h.update(tasks.tobytes())
        return h.hexdigest(), len(tasks), 1, -1
    tasks, m, chains, time, rho1, ok = plan(L, T, nz, max_chains)
    for part in (m, chains, time, rho1, np.int32(ok), tasks):
        h.update(np.ascontiguousarray(part).tobytes())
    if max_chains == 1:
        t7, m7 = one_chain_list(L, T, nz)
        h.update(m7.tobytes()); h.update(t7.tobytes())
    return h.hexdigest(), len(tasks), int(chains[0]), ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=None, help="the shared library to probe (default: this tree's)")
    ap.add_argument("--one", action="store_true", help="walk the corpus once, under the environment as it is")
    args = ap.parse_args()
    if args.one:
        L = load(args.lib)
        for name, T, max_chains, nz in corpus():
            sha, ntasks, nchains, ok = digest(L, T, max_chains, nz)
            print("%-26s T %3d tasks %6d chains %2d verified %2d %s" % (name, T, ntasks, nchains, ok, sha), flush=True)
        return 0
    base = {k: v for k, v in os.environ.items() if not k.startswith("PPSFM_CHOL_")}
    for setting in SETTINGS:
        print("# " + (" ".join("%s=%s" % kv for kv in setting.items()) or "default switches"), flush=True)
        cmd = [sys.executable, os.path.abspath(__file__), "--one"] + (["--lib", args.lib] if args.lib else [])
        rc = subprocess.call(cmd, env=dict(base, **setting))
        if rc:
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
