"""CPU-only checks of the C ABI of K21 (pp_sift_extract*): the symbols are exported and declared, the structs have the layout and the defaults the
header states, null arguments and every option the check refuses are PP_ERR_INVALID - an error code, not an abort - before a handle is read and with
the outputs untouched, the Python options refuse what the covariant extractor would need, and there is no CPU path: without a device
pp_sift_extractor_create is PP_ERR_HIP.  Everything that needs a device runs in tests/test_gpu_sift_extract.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from privacy_preserving_sfm_amd import _capi, device, feature_extraction as fe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["pp_sift_extract_options_default", "pp_sift_extractor_create", "pp_sift_extractor_destroy", "pp_sift_extract", "pp_sift_extract_stage",
           "pp_sift_extract_candidates", "pp_sift_extract_features"]
F32P, I64P = C.POINTER(C.c_float), C.POINTER(C.c_int64)


def test_the_symbols_are_exported_and_declared():
    L = _capi.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppsfm_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert name in _capi.exported_symbols() and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert "pp_sift_extract_options" in text and "pp_sift_extract_report" in text and "pp_sift_extractor_handle" in text


def test_the_struct_sizes_and_defaults_match_the_header():
    assert C.sizeof(_capi.SiftExtractOptions) == 4 * 4 + 2 * 8 + 4 * 4
    assert _capi.SiftExtractOptions.peak_threshold.offset == 16 and _capi.SiftExtractOptions.max_num_orientations.offset == 32
    assert C.sizeof(_capi.SiftExtractReport) == 4 * 4 + 11 * 8 + 4 * 32 * 4 + 7 * 8
    assert _capi.SiftExtractReport.num_keypoints.offset == 16 and _capi.SiftExtractReport.octave_width.offset == 104
    assert _capi.SiftExtractReport.phase_ms.offset == 104 + 512 and _capi.SiftExtractReport.total_ms.offset == 104 + 512 + 48
    o = device.sift_extract_options()
    assert (o.max_num_features, o.first_octave, o.num_octaves, o.octave_resolution) == (8192, -1, 4, 3)      # feature/sift.h:57-112
    assert (o.peak_threshold, o.edge_threshold, o.max_num_orientations, o.upright, o.normalization, o.phase_timings) == (0.02 / 3, 10.0, 2, 0, 0, 0)
    p = fe.SiftExtractionOptions()
    assert (p.max_num_features, p.first_octave, p.num_octaves, p.octave_resolution, p.peak_threshold, p.edge_threshold) == (8192, -1, 4, 3, 0.02 / 3, 10.0)
    assert (p.max_num_orientations, p.upright, p.normalization, p.max_image_size) == (2, False, "L1_ROOT", 3200) and p.Check()
    q = p.device_options()
    assert all(getattr(q, f) == getattr(o, f) for f, _ in _capi.SiftExtractOptions._fields_)
    assert fe.SiftExtractionOptions(normalization="L2", upright=True, darkness_adaptivity=True).device_options().normalization == _capi.SIFT_L2
    with pytest.raises(AttributeError):
        device.sift_extract_options(max_image_size=5)      # not a field: the caller supplies the array
    with pytest.raises(AttributeError):
        fe.SiftExtractionOptions(no_such_option=1)


def test_the_python_options_refuse_the_covariant_extractor():
    for kw in (dict(estimate_affine_shape=True), dict(domain_size_pooling=True)):
        with pytest.raises(ValueError):
            fe.SiftExtractionOptions(**kw).device_options()
    with pytest.raises(ValueError):
        fe.SiftExtractionOptions(normalization="L3").device_options()
    for kw in (dict(max_num_features=0), dict(octave_resolution=0), dict(peak_threshold=0.0), dict(edge_threshold=0.0), dict(max_num_orientations=0),
               dict(max_image_size=0), dict(domain_size_pooling=True, dsp_num_scales=0)):
        assert not fe.SiftExtractionOptions(**kw).Check()
        with pytest.raises(ValueError):
            fe.ExtractSiftFeatures(np.zeros((8, 8), dtype=np.uint8), fe.SiftExtractionOptions(**kw))      # before a handle is made


def _extract(h, o, grey, rep, cap, kp, desc, num, w=16, h_=12):
    return _capi.lib().pp_sift_extract(h, o, w, h_, grey, rep, cap, kp, desc, num)


def _buffers():
    grey = (C.c_uint8 * (16 * 12))()
    kp = (C.c_float * 16)(*([7.0] * 16))
    desc = (C.c_uint8 * 512)(*([9] * 512))
    return grey, kp, desc, C.c_int64(-5), _capi.SiftExtractReport()


def test_null_arguments_are_refused_before_a_handle_is_read():
    L = _capi.lib()
    o = device.sift_extract_options()
    grey, kp, desc, num, rep = _buffers()
    rep.num_features = 77
    bogus = C.c_void_p(1)      # never dereferenced: the cases below are refused on the other arguments first
    assert _extract(bogus, None, grey, C.byref(rep), 4, kp, desc, C.byref(num)) == _capi.PP_ERR_INVALID
    assert b"pp_sift_extract" in L.pp_last_error()
    assert _extract(bogus, C.byref(o), None, C.byref(rep), 4, kp, desc, C.byref(num)) == _capi.PP_ERR_INVALID
    assert _extract(bogus, C.byref(o), grey, None, 4, kp, desc, C.byref(num)) == _capi.PP_ERR_INVALID
    assert _extract(bogus, C.byref(o), grey, C.byref(rep), 4, None, desc, C.byref(num)) == _capi.PP_ERR_INVALID
    assert _extract(bogus, C.byref(o), grey, C.byref(rep), 4, kp, desc, None) == _capi.PP_ERR_INVALID
    assert _extract(bogus, C.byref(o), grey, C.byref(rep), -1, kp, desc, C.byref(num)) == _capi.PP_ERR_INVALID
    assert _extract(None, C.byref(o), grey, C.byref(rep), 4, kp, None, C.byref(num)) == _capi.PP_ERR_INVALID      # good options, no handle
    assert b"null handle" in L.pp_last_error()
    assert rep.num_features == 77 and num.value == -5 and list(kp) == [7.0] * 16 and list(desc) == [9] * 512      # untouched
    f1, i3, w, hh = (C.c_float * 4)(), (C.c_int32 * 3)(), C.c_int32(), C.c_int32()
    assert L.pp_sift_extract_stage(None, 0, 0, 0, f1, 4, C.byref(w), C.byref(hh)) == _capi.PP_ERR_INVALID
    assert L.pp_sift_extract_candidates(None, 0, i3, 1, C.byref(num)) == _capi.PP_ERR_INVALID
    assert L.pp_sift_extract_features(None, None, None, None, 0, C.byref(num)) == _capi.PP_ERR_INVALID
    assert L.pp_sift_extractor_create(0, None) == _capi.PP_ERR_INVALID
    assert L.pp_sift_extractor_destroy(None) == _capi.PP_OK
    L.pp_sift_extract_options_default(None)      # tolerated


BAD = [("max_num_features", 0), ("max_num_features", -3), ("octave_resolution", 0), ("octave_resolution", 33), ("peak_threshold", 0.0),
       ("peak_threshold", float("nan")), ("edge_threshold", 0.0), ("edge_threshold", float("nan")), ("max_num_orientations", 0), ("max_num_orientations", 5),
       ("normalization", 2), ("normalization", -1), ("num_octaves", 0), ("num_octaves", 33), ("first_octave", -9), ("first_octave", 9), ("first_octave", 5)]


@pytest.mark.parametrize("field,value", BAD)
def test_bad_options_are_refused(field, value):
    o = device.sift_extract_options(**{field: value})
    grey, kp, desc, num, rep = _buffers()
    assert _extract(C.c_void_p(1), C.byref(o), grey, C.byref(rep), 4, kp, desc, C.byref(num)) == _capi.PP_ERR_INVALID      # before the handle is read
    assert num.value == -5 and list(kp) == [7.0] * 16 and list(desc) == [9] * 512


@pytest.mark.parametrize("w,h,first_octave", [(0, 12, -1), (16, 0, -1), (-16, 12, -1), (20000, 14000, -1), (40000, 30000, 0), (2 ** 20, 2, 0), (16, 12, 2)])
def test_bad_sizes_are_refused(w, h, first_octave):
    """non-positive sizes, a first octave of 2^30 pixels or more, a last octave (first_octave + 3) without a pixel: the image is never read"""
    o = device.sift_extract_options(first_octave=first_octave)
    grey, kp, desc, num, rep = _buffers()
    assert _extract(C.c_void_p(1), C.byref(o), grey, C.byref(rep), 4, kp, desc, C.byref(num), w=w, h_=h) == _capi.PP_ERR_INVALID
    assert num.value == -5


def test_no_cpu_path_without_a_device():
    n = C.c_int()
    _capi.lib().pp_device_count(C.byref(n))
    if n.value:
        return      # (tests/test_gpu_sift_extract.py runs the calls)
    with pytest.raises(_capi.PPError) as e:
        device.SiftExtractor()
    assert e.value.code == _capi.PP_ERR_HIP
    with pytest.raises(_capi.PPError):
        fe.ExtractSiftFeatures(np.zeros((16, 16), dtype=np.uint8))
