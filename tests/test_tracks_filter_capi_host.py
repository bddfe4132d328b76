"""CPU-only checks of the C ABI of K14 (pp_tracks_filter_points / pp_tracks_filter_negative_depth / pp_tracks_filter_images): the three symbols are exported
and declared, the report has the layout the header states, and a null argument or bad options are PP_ERR_INVALID - an error code, not an abort - before any
device work and before the handle is read (tracks_filter.hip pins that order; the cases here pass a handle that must never be dereferenced).  Without a
device no filter call can get further than that: the handle it needs cannot be created (PP_ERR_HIP), which is all the last test shows; the calls themselves
run in tests/test_gpu_tracks_filter.py."""
import ctypes as C
import os
import re

import pytest

import tracks_filter_scenes as scenes
from privacy_preserving_sfm_amd import _capi
from privacy_preserving_sfm_amd.device import TracksProblem
from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pp_tracks_filter_points", "pp_tracks_filter_negative_depth", "pp_tracks_filter_images")


def test_the_three_symbols_are_exported_and_declared():
    L = _capi.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppsfm_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert name in _capi.exported_symbols() and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert "pp_tracks_filter_report" in text
    assert C.sizeof(_capi.TracksFilterReport) == 4 * 8 + 2 * 4 + 3 * 8


def test_null_arguments_and_bad_options_are_invalid_before_any_device_work():
    L = _capi.lib()
    o, rep = _capi.FilterOptions(4.0, 1.5), _capi.TracksFilterReport()
    order, out = (C.c_int32 * 1)(0), (C.c_int32 * 1)(0)
    bogus = C.c_void_p(1)      # never dereferenced: every case below is refused on its other arguments first
    assert L.pp_tracks_filter_points(None, C.byref(o), None, None, None, C.byref(rep), None, None, 0, None) == _capi.PP_ERR_INVALID
    assert b"pp_tracks_filter_points" in L.pp_last_error()
    assert L.pp_tracks_filter_points(bogus, C.byref(o), None, None, None, None, None, None, 0, None) == _capi.PP_ERR_INVALID          # no report
    assert L.pp_tracks_filter_points(bogus, C.byref(o), None, None, None, C.byref(rep), None, None, 4, None) == _capi.PP_ERR_INVALID  # capacity without arrays
    assert L.pp_tracks_filter_points(bogus, C.byref(o), None, None, None, C.byref(rep), None, None, -1, None) == _capi.PP_ERR_INVALID
    assert L.pp_tracks_filter_points(bogus, None, None, None, None, C.byref(rep), None, None, 0, None) == _capi.PP_ERR_INVALID        # no options
    for bad in (_capi.FilterOptions(-1.0, 1.5), _capi.FilterOptions(4.0, -0.5), _capi.FilterOptions(float("nan"), 1.5)):
        assert L.pp_tracks_filter_points(bogus, C.byref(bad), None, None, None, C.byref(rep), None, None, 0, None) == _capi.PP_ERR_INVALID
        assert b"bad options" in L.pp_last_error()
    sub = (C.c_uint8 * 4)(1, 1, 1, 1)
    assert L.pp_tracks_filter_points(bogus, C.byref(o), None, sub, sub, C.byref(rep), None, None, 0, None) == _capi.PP_ERR_INVALID    # both subsets
    assert b"both" in L.pp_last_error()
    assert L.pp_tracks_filter_negative_depth(None, order, 1, C.byref(rep), None, None, 0) == _capi.PP_ERR_INVALID
    assert L.pp_tracks_filter_negative_depth(bogus, order, 1, None, None, None, 0) == _capi.PP_ERR_INVALID
    assert L.pp_tracks_filter_images(None, order, 1, out, C.byref(rep), None, None, 0) == _capi.PP_ERR_INVALID
    assert L.pp_tracks_filter_images(bogus, order, 1, None, C.byref(rep), None, None, 0) == _capi.PP_ERR_INVALID                      # no room for the images
    assert L.pp_tracks_filter_images(bogus, order, 1, out, None, None, None, 0) == _capi.PP_ERR_INVALID


def test_no_cpu_path_without_a_device():
    n = C.c_int()
    _capi.lib().pp_device_count(C.byref(n))
    if n.value:
        return      # (tests/test_gpu_tracks_filter.py runs the calls)
    rec, graph, _, _ = scenes.one_bad_of_five()
    flat = IncrementalTriangulator(graph, rec).flatten()[0]
    with pytest.raises(_capi.PPError) as e:
        TracksProblem(flat)
    assert e.value.code == _capi.PP_ERR_HIP
