"""The chunked Schur assembly (k_schur_self_chunks + k_schur_chunk_reduce, csrc/ba_schur.hip) at the boundaries of its chunks.

make_ba_scene(3, n, 3): every point is seen by all three images, so every pair list has exactly n entries (one per point).  The generator holds
pose 0 constant (the gauge), and a constant image gets no list: the scene as generated has ONE list, images (2, 1); with every pose variable it has the
three lists (1, 0), (2, 0), (2, 1) and the chunk ranges of several pairs side by side.  Both are run.

Chunk length (ChunkPairLists, csrc/ba_structure.hpp): these scenes have 3n <= 65536 entries in all, so a longest list above 12 entries is
`latency_bound` - the lists are cut into chunks of L = 8 (the general length, 16, is never taken at these sizes; its multiples are listed too) - and a list
of up to 12 entries is not cut at all.  n = 8 therefore takes the per-list gather under either setting of the switch, every other n the chunks:
n = 9: 8 + 1; 16: two full chunks; 17: 8 + 8 + 1; 32, 33: the same at four chunks; 65: the first length above the other threshold (longest > 64),
nine chunks - the reduction's eight-at-a-time loop and its remainder.  Which path a handle took shows in the pool: a chunked handle holds three device
blocks more (test_gpu_resource_ownership.py::test_chunked_pair_lists)."""
import ctypes as C

import numpy as np
import pytest

from cholesky_reference import var_cols as _var_cols
from privacy_preserving_sfm_amd import _capi, synthetic
from privacy_preserving_sfm_amd.device import BAProblem

pytestmark = pytest.mark.gpu

L = 8      # chunk length of a latency-bound handle


def _pair_list_lengths(sc):
    """entries of the pair list of every two variable images i > j: the observation pairs (one of i, one of j) of a shared variable point"""
    C_, P = len(sc["pose_const"]), len(sc["point_const"])
    count = np.zeros((P, C_), dtype=np.int64)
    np.add.at(count, (sc["obs_point"], sc["obs_pose"]), 1)
    count[np.asarray(sc["point_const"]) != 0] = 0
    var = np.flatnonzero(np.asarray(sc["pose_const"]) == 0)
    return {(int(i), int(j)): int((count[:, i] * count[:, j]).sum()) for i in var for j in var if j < i}


def _live_device_blocks():
    dev = C.c_int64(-1)
    assert _capi.lib().pp_pool_stats(C.byref(dev), None, None) == 0 and dev.value >= 0
    return dev.value


@pytest.mark.parametrize("free_gauge", [False, True])
@pytest.mark.parametrize("n", [L, L + 1, 2 * L, 2 * L + 1, 4 * L, 4 * L + 1, 65])
def test_chunk_boundaries_match_oracle_and_the_unchunked_gather(oracle, monkeypatch, n, free_gauge):
    sc = synthetic.make_ba_scene(3, n, 3, seed=500 + n, model=2)
    if free_gauge:
        sc["pose_const"] = np.zeros_like(np.ascontiguousarray(sc["pose_const"]))
    lengths = _pair_list_lengths(sc)
    assert lengths == ({(1, 0): n, (2, 0): n, (2, 1): n} if free_gauge else {(2, 1): n})
    cols = _var_cols(sc)
    out, held = {}, {}
    for chunked in ("1", "0"):
        with monkeypatch.context() as m:
            m.setenv("PPSFM_BA_CHUNKED_PAIRS", chunked)
            before = _live_device_blocks()
            pb = BAProblem(sc)
            try:
                out[chunked] = [pb.reduced_system(radius) for radius in (1e4, 0.5)]
                held[chunked] = _live_device_blocks() - before
            finally:
                pb.close()
    assert held["1"] == held["0"] + (3 if n > 12 else 0), held      # the chunks, the first chunk of every pair, the chunks' partial blocks
    for k, radius in enumerate((1e4, 0.5)):
        ref = oracle.ba_reduced_system(sc, radius)
        assert len(cols) == ref["nc"]
        scale, rscale = np.abs(ref["S"]).max(), np.abs(ref["rhs"]).max()
        for chunked in ("1", "0"):
            S, rhs = out[chunked][k]
            assert np.allclose(S[np.ix_(cols, cols)], ref["S"], rtol=1e-9, atol=1e-11 * scale), (chunked, radius)
            assert np.allclose(rhs[cols], ref["rhs"], rtol=1e-9, atol=1e-11 * rscale), (chunked, radius)
        (S1, rhs1), (S0, rhs0) = out["1"][k], out["0"][k]
        assert np.allclose(S1, S0, rtol=1e-9, atol=1e-11 * scale) and np.allclose(rhs1, rhs0, rtol=1e-9, atol=1e-11 * rscale), radius
