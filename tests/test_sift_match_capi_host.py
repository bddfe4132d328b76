"""CPU-only checks of the C ABI of K17 (pp_sift_*): the symbols are exported and declared, the structs have the layout and the defaults the header states,
null arguments and options SiftMatchingOptions::Check refuses are PP_ERR_INVALID - an error code, not an abort - before a handle is read,
pp_sift_match_thresholds (host only) gives the integers tests/sift_match_reference.py derives from the float rules, and there is no CPU path: without a
device pp_sift_create is PP_ERR_HIP.  Everything that needs a device runs in tests/test_gpu_sift_match.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sift_match_reference as ref
from privacy_preserving_sfm_amd import _capi, device, feature_matching

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["pp_sift_match_options_default", "pp_sift_create", "pp_sift_destroy", "pp_sift_match_pairs", "pp_sift_top2", "pp_sift_match_thresholds"]
I64P = C.POINTER(C.c_int64)


def test_the_symbols_are_exported_and_declared():
    L = _capi.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppsfm_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert name in _capi.exported_symbols() and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert "pp_sift_match_options" in text and "pp_sift_match_report" in text and "pp_sift_handle" in text


def test_the_struct_sizes_and_defaults_match_the_header():
    assert C.sizeof(_capi.SiftMatchOptions) == 2 * 8 + 2 * 4 + 8
    assert _capi.SiftMatchOptions.cross_check.offset == 16 and _capi.SiftMatchOptions.workspace_bytes.offset == 24
    assert C.sizeof(_capi.SiftMatchReport) == 8 + 2 * 4 + 2 * 8
    assert _capi.SiftMatchReport.num_batches.offset == 12 and _capi.SiftMatchReport.device_ms.offset == 16
    o = device.sift_match_options()
    assert (o.max_ratio, o.max_distance, o.cross_check, o.min_num_matches, o.workspace_bytes) == (0.8, 0.7, 1, 15, 0)      # feature/sift.h:117-145
    m = feature_matching.SiftMatchingOptions()
    assert (m.max_ratio, m.max_distance, m.cross_check, m.min_num_matches, m.max_num_matches) == (0.8, 0.7, True, 15, 32768) and m.Check()
    with pytest.raises(AttributeError):
        device.sift_match_options(max_num_matches=5)      # not a field: the brute-force rule never reads it


def test_the_mirror_has_the_methods():
    for name in ("match_pairs", "top2", "close"):
        assert callable(getattr(device.SiftMatcher, name))
    for name in ("MatchSiftFeatures", "exhaustive_image_pairs", "FeatureMatcher", "build_correspondence_graph"):
        assert callable(getattr(feature_matching, name))


def _match(h, o, rep, start, out, pairs=None, num=1, cap=4):
    pr = (C.c_int32 * 2)(0, 0) if pairs is None else pairs
    return _capi.lib().pp_sift_match_pairs(h, o, num, pr, rep, start, out, cap)


def test_null_arguments_are_refused_before_a_handle_is_read():
    L = _capi.lib()
    o, rep = device.sift_match_options(), _capi.SiftMatchReport()
    rep.num_matches = 77
    start, out = (C.c_int64 * 2)(5, 5), (C.c_int32 * 8)()
    bogus = C.c_void_p(1)      # never dereferenced: the cases below are refused on the other arguments first
    assert _match(None, C.byref(o), C.byref(rep), start, out) == _capi.PP_ERR_INVALID
    assert b"pp_sift_match_pairs" in L.pp_last_error()
    assert _match(bogus, None, C.byref(rep), start, out) == _capi.PP_ERR_INVALID
    assert _match(bogus, C.byref(o), None, start, out) == _capi.PP_ERR_INVALID
    assert _match(bogus, C.byref(o), C.byref(rep), None, out) == _capi.PP_ERR_INVALID
    assert _match(bogus, C.byref(o), C.byref(rep), start, None) == _capi.PP_ERR_INVALID      # capacity 4 without a buffer
    assert L.pp_sift_match_pairs(bogus, C.byref(o), 1, None, C.byref(rep), start, out, 4) == _capi.PP_ERR_INVALID
    assert _match(bogus, C.byref(o), C.byref(rep), start, out, cap=-1) == _capi.PP_ERR_INVALID
    assert rep.num_matches == 77 and list(start) == [5, 5]      # untouched
    i3 = (C.c_int32 * 3)()
    assert L.pp_sift_top2(None, 0, 0, i3, i3, i3) == _capi.PP_ERR_INVALID
    assert L.pp_sift_top2(bogus, 0, 0, None, i3, i3) == _capi.PP_ERR_INVALID
    assert L.pp_sift_top2(bogus, 0, 0, i3, None, i3) == _capi.PP_ERR_INVALID
    assert L.pp_sift_top2(bogus, 0, 0, i3, i3, None) == _capi.PP_ERR_INVALID
    h = C.c_void_p()
    s0 = (C.c_int64 * 1)(0)
    assert L.pp_sift_create(0, None, None, 0, C.byref(h)) == _capi.PP_ERR_INVALID
    assert L.pp_sift_create(0, s0, None, 0, None) == _capi.PP_ERR_INVALID
    assert L.pp_sift_destroy(None) == _capi.PP_OK
    L.pp_sift_match_options_default(None)      # tolerated
    d_min, count = C.c_int32(), C.c_int64()
    assert L.pp_sift_match_thresholds(None, C.byref(d_min), None, 0, C.byref(count)) == _capi.PP_ERR_INVALID
    assert L.pp_sift_match_thresholds(C.byref(o), None, None, 0, C.byref(count)) == _capi.PP_ERR_INVALID
    assert L.pp_sift_match_thresholds(C.byref(o), C.byref(d_min), None, 0, None) == _capi.PP_ERR_INVALID


@pytest.mark.parametrize("field,value", [("max_ratio", 0.0), ("max_ratio", -0.5), ("max_ratio", float("nan")), ("max_distance", 0.0), ("max_distance", -1.0),
                                         ("min_num_matches", -1), ("workspace_bytes", -1)])
def test_bad_options_are_refused(field, value):
    L = _capi.lib()
    o, rep = device.sift_match_options(**{field: value}), _capi.SiftMatchReport()
    start, out = (C.c_int64 * 2)(), (C.c_int32 * 8)()
    assert _match(C.c_void_p(1), C.byref(o), C.byref(rep), start, out) == _capi.PP_ERR_INVALID      # before the handle is read
    d_min, count = C.c_int32(), C.c_int64()
    assert L.pp_sift_match_thresholds(C.byref(o), C.byref(d_min), None, 0, C.byref(count)) == _capi.PP_ERR_INVALID
    assert not feature_matching.SiftMatchingOptions(**{field: value}).Check() if field != "workspace_bytes" else True


def test_bad_descriptor_offsets_are_refused():
    L = _capi.lib()
    h = C.c_void_p()
    d = (C.c_uint8 * 256)()
    assert L.pp_sift_create(-1, (C.c_int64 * 1)(0), d, 0, C.byref(h)) == _capi.PP_ERR_INVALID
    assert L.pp_sift_create(2, (C.c_int64 * 3)(1, 1, 2), d, 0, C.byref(h)) == _capi.PP_ERR_INVALID      # does not start at 0
    assert L.pp_sift_create(2, (C.c_int64 * 3)(0, 2, 1), d, 0, C.byref(h)) == _capi.PP_ERR_INVALID      # decreases
    assert L.pp_sift_create(1, (C.c_int64 * 2)(0, 2), None, 0, C.byref(h)) == _capi.PP_ERR_INVALID      # rows without data
    assert not h.value


@pytest.mark.parametrize("ratio,distance", [(0.8, 0.7), (1.5, 0.7), (0.8, 3.0), (0.8, 1e-3), (1e-3, 0.7)])
def test_the_thresholds_equal_the_reference(ratio, distance):
    d_min, table = device.sift_match_thresholds(device.sift_match_options(max_ratio=ratio, max_distance=distance))
    r_d_min, r_table = ref.thresholds(ratio, distance)
    assert d_min == r_d_min and np.array_equal(table, r_table)
    rng = np.random.default_rng(7)
    best = rng.integers(1, ref.MAX_DIST + 1, size=20000)
    best[::2] = rng.integers(1, ref.CLAMP + 1000, size=10000)
    second = (rng.uniform(size=20000) * (best + 1)).astype(np.int64)
    by_table = (best >= d_min) & (np.minimum(second, ref.CLAMP) <= table[np.maximum(np.minimum(best, ref.CLAMP) - d_min, 0)])
    assert np.array_equal(by_table, ref.accept(best, second, ratio, distance))


def test_the_default_thresholds():
    d_min, table = device.sift_match_thresholds()
    assert d_min == 200499 and len(table) == 61646


def test_a_table_capacity_below_the_count_is_refused():
    L = _capi.lib()
    o = device.sift_match_options()
    d_min, count = C.c_int32(-5), C.c_int64(-5)
    small = (C.c_int32 * 4)(9, 9, 9, 9)
    assert L.pp_sift_match_thresholds(C.byref(o), C.byref(d_min), small, 4, C.byref(count)) == _capi.PP_ERR_INVALID
    assert list(small) == [9, 9, 9, 9] and d_min.value == -5


def test_no_cpu_path_without_a_device():
    n = C.c_int()
    _capi.lib().pp_device_count(C.byref(n))
    if n.value:
        return      # (tests/test_gpu_sift_match.py runs the calls)
    with pytest.raises(_capi.PPError) as e:
        device.SiftMatcher([np.zeros((3, 128), dtype=np.uint8)])
    assert e.value.code == _capi.PP_ERR_HIP
    with pytest.raises(_capi.PPError):
        feature_matching.MatchSiftFeatures(feature_matching.SiftMatchingOptions(), np.zeros((3, 128), dtype=np.uint8), np.zeros((2, 128), dtype=np.uint8))
