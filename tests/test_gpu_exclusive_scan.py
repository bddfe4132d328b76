"""The library's one exclusive scan (csrc/scan.hpp: BlockExclusiveScan, LaunchExclusiveScan) through pp_debug_exclusive_scan, against numpy.cumsum:
EXACT equality, every element and the total - the sums are integer, so no tolerance applies.

The sizes straddle the code's own edges:
  64 / 256 / 1024   a wavefront, the tile kernels' workgroup, the direct kernel's workgroup (a span of one element per thread up to 1024, two above)
  4096              kScanDirect: up to here one launch of the direct kernel, above it tile sums -> the direct kernel over them -> the tiles
  5120              a tile edge (kScanTile = 1024) above kScanDirect
  1 048 576         1024 tiles: the direct kernel over the tile sums at one span element per thread; 1 048 577 and 1 049 603 (= 1024 * 1025 + 3) give 1025
                    and 1026 tiles, spans of two
The largest input is 4 MB (8 MB as int64)."""
import ctypes as C

import numpy as np
import pytest

from privacy_preserving_sfm_amd import _capi

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 5119, 5120, 5121, 1048576, 1048577, 1049603]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _scan(arrays):
    """the n + 1 outputs of pp_debug_exclusive_scan for one or two arrays of the same dtype and length"""
    n, dtype = len(arrays[0]), arrays[0].dtype
    outs = [np.full(n + 1, -1, dtype=dtype) for _ in arrays]
    args = [_ptr(arrays[0]), _ptr(outs[0])] + ([_ptr(arrays[1]), _ptr(outs[1])] if len(arrays) == 2 else [None, None])
    L = _capi.lib()
    rc = L.pp_debug_exclusive_scan(0, dtype.itemsize, n, *args)
    assert rc == _capi.PP_OK, L.pp_last_error()
    return outs


def _expected(a):
    out = np.zeros(len(a) + 1, dtype=a.dtype)
    np.cumsum(a, out=out[1:])
    return out


@pytest.mark.parametrize("n", SIZES)
def test_int32_one_job(n):
    a = np.random.default_rng(n).integers(0, 8, size=n, dtype=np.int32)
    (out,) = _scan([a])
    assert np.array_equal(out, _expected(a))


@pytest.mark.parametrize("n", [1, 4096, 4097, 1049603])
def test_int32_two_jobs_do_not_mix(n):
    rng = np.random.default_rng(1000 + n)
    a = rng.integers(0, 8, size=n, dtype=np.int32)
    b = rng.integers(0, 3, size=n, dtype=np.int32) * 5 + 1      # another total, another content
    out_a, out_b = _scan([a, b])
    assert np.array_equal(out_a, _expected(a))
    assert np.array_equal(out_b, _expected(b))


@pytest.mark.parametrize("n", [1, 65, 1025, 4097, 1049603])
def test_int64_beyond_32_bits(n):
    a = np.random.default_rng(2000 + n).integers(0, 2 ** 33, size=n, dtype=np.int64, endpoint=True)
    (out,) = _scan([a])
    want = _expected(a)
    assert np.array_equal(out, want)
    assert n < 65 or want[16:].min() > 2 ** 32      # (the prefixes do leave 32 bits)


def test_bad_arguments_are_refused_and_the_next_call_works():
    L = _capi.lib()
    a = np.arange(5, dtype=np.int32)
    out = np.zeros(6, dtype=np.int32)
    for elem_bytes, n, out_ptr in [(2, 5, _ptr(out)), (4, -1, _ptr(out)), (4, 5, None)]:
        assert L.pp_debug_exclusive_scan(0, elem_bytes, n, _ptr(a), out_ptr, None, None) == _capi.PP_ERR_INVALID
        assert b"pp_debug_exclusive_scan" in L.pp_last_error()
        assert np.array_equal(_scan([a])[0], [0, 0, 1, 3, 6, 10])
