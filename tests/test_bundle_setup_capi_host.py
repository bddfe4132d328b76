"""CPU-only checks of the C ABI of K16 (pp_tracks_bundle_setup): the symbol is exported and declared, the structs have the layout the header states, and
a null handle, config or report is PP_ERR_INVALID - an error code, not an abort - before the handle is read.  Everything that needs the handle's state runs
in tests/test_gpu_bundle_setup.py."""
import ctypes as C
import os
import re

import pytest

from privacy_preserving_sfm_amd import _capi
from privacy_preserving_sfm_amd.bundle_adjustment import BundleAdjuster
from privacy_preserving_sfm_amd.device import TracksProblem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_exported_and_declared():
    L = _capi.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppsfm_hip.h")).read(), flags=re.S)
    assert "pp_tracks_bundle_setup" in _capi.exported_symbols() and hasattr(L, "pp_tracks_bundle_setup")
    assert re.search(r"\bpp_tracks_bundle_setup\s*\(", text)
    assert "pp_bundle_config" in text and "pp_bundle_setup_report" in text
    assert re.search(r"PP_BUNDLE_IMAGE\s*=\s*1\b", text) and re.search(r"PP_BUNDLE_CONST_POSE\s*=\s*2\b", text)
    assert (_capi.PP_BUNDLE_IMAGE, _capi.PP_BUNDLE_CONST_POSE) == (1, 2)


def test_the_struct_sizes_match_the_header():
    assert C.sizeof(_capi.BundleConfig) == 6 * 8 + 2 * 4            # six pointers, two counts
    assert C.sizeof(_capi.BundleSetupReport) == 2 * 8 + 4 * 4 + 8 + 3 * 8
    assert _capi.BundleSetupReport.bad_line.offset == 32 and _capi.BundleSetupReport.device_ms.offset == 40
    assert _capi.BundleConfig.num_variable_points.offset == 48


def test_the_mirror_has_the_methods():
    assert callable(getattr(TracksProblem, "bundle_setup")) and callable(getattr(BundleAdjuster, "flatten_on"))


def _call(h, cfg, rep):
    M, P, Cn, K = 4, 4, 2, 1
    d, i, u8, u16 = (C.c_double * (3 * M))(), C.c_int32 * M, C.c_uint8 * M, C.c_uint16 * K
    return _capi.lib().pp_tracks_bundle_setup(h, cfg, rep, d, i(), i(), i(), M, (C.c_int32 * Cn)(), (C.c_uint8 * Cn)(), (C.c_uint8 * Cn)(), (C.c_int32 * Cn)(),
                                              i(), u8(), (C.c_double * (3 * P))(), P, (C.c_int32 * K)(), u16())


def test_null_arguments_are_refused_before_the_handle_is_read():
    L = _capi.lib()
    flags = (C.c_uint8 * 2)(1, 1)
    cfg = _capi.BundleConfig(C.cast(flags, _capi.c_u8p), None, None, None, None, None, 0, 0)
    rep = _capi.BundleSetupReport()
    rep.num_obs = 77
    bogus = C.c_void_p(1)      # never dereferenced: the cases below are refused on the other arguments first
    assert _call(None, C.byref(cfg), C.byref(rep)) == _capi.PP_ERR_INVALID
    assert b"pp_tracks_bundle_setup" in L.pp_last_error()
    assert _call(bogus, None, C.byref(rep)) == _capi.PP_ERR_INVALID
    assert _call(bogus, C.byref(cfg), None) == _capi.PP_ERR_INVALID
    assert rep.num_obs == 77      # untouched


def test_no_cpu_path_without_a_device():
    import bundle_setup_worlds as bsw
    from privacy_preserving_sfm_amd.incremental_triangulator import CorrespondenceGraph, IncrementalTriangulator
    n = C.c_int()
    _capi.lib().pp_device_count(C.byref(n))
    if n.value:
        return      # (tests/test_gpu_bundle_setup.py runs the calls)
    tri = IncrementalTriangulator(CorrespondenceGraph(), bsw.world(2, 3, 2))
    with pytest.raises(_capi.PPError) as e:
        tri._open(tri.Options())
    assert e.value.code == _capi.PP_ERR_HIP
