"""K21 on the device: pp_sift_extract for every golden image and option variant against the recording of the reference's CPU extractor
(tests/golden/sift), with NO tolerance and in the same order: every Gaussian, DoG and gradient level through the stage reader against its digest and
sampled rows, the candidates, the keypoints, angles and raw descriptors by their bits, the uint8 descriptors against the project's rule
(sift_extract_goldens.finish_descriptors), the range max_num_features keeps.  Workspace reuse: the same image twice, and after a larger image on the
same handle, gives the same bytes.  The capacity rule: too small leaves the outputs untouched and reports the need."""
import ctypes as C

import numpy as np
import pytest

import sift_extract_goldens as G
from privacy_preserving_sfm_amd import _capi, feature_extraction as fe
from privacy_preserving_sfm_amd.device import SiftExtractor, sift_extract_options

pytestmark = pytest.mark.gpu
KIND = {"gauss": _capi.SIFT_STAGE_GAUSSIAN, "dog": _capi.SIFT_STAGE_DOG, "grad": _capi.SIFT_STAGE_GRADIENT}


@pytest.fixture(scope="module")
def extractor():
    ex = SiftExtractor()
    yield ex
    ex.close()


def _options(c, **kw):
    return sift_extract_options(**dict(c["options"], **kw))


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_every_stage_and_the_result_equal_the_recording(extractor, name):
    c = G.case(name)
    rec = G.recording(c)
    kp, desc, rep = extractor.extract(G.image(c), _options(c))
    for key, kind, o, s in G.stage_names(rec):
        G.check_stage(rec, key, extractor.stage(KIND[kind], o, s), sampled=name in ("blobs", "odd", "tiny"))
    assert rep.num_octaves == len(rec["octave_counts"])
    for q, (o, w, h, ncand, nkeys) in enumerate(rec["octave_counts"]):
        assert (rep.octave_width[q], rep.octave_height[q], rep.octave_candidates[q], rep.octave_keypoints[q]) == (w, h, ncand, nkeys)
        G.assert_same_bits(extractor.candidates(o), rec["cand_%d" % o], "candidates of octave %d" % o)
    raw, octave_level, angles = extractor.features()
    G.check_result(c, kp, desc, raw, octave_level, angles, rep.first_level_to_keep)
    assert rep.num_features == len(kp) == c["cut"][2] and rep.num_features_found == len(rec["keypoints"]) and rep.num_levels == len(rec["levels"])
    assert rep.num_keypoints == int(rec["levels"][:, 2].sum()) and rep.num_descriptors_skipped == 0


def test_the_report_names_the_cases_of_the_large_image(extractor):
    c = G.case("blobs")
    _, _, rep = extractor.extract(G.image(c), _options(c, phase_timings=1))
    assert rep.num_features >= 100 and rep.num_two_orientations > 0 and rep.num_moved > 0 and rep.num_rejected_edge > 0 and rep.num_rejected_peak > 0
    assert rep.num_windows_cut > 0
    assert all(ms > 0 for ms in rep.phase_ms) and rep.device_ms >= sum(rep.phase_ms) * 0.99 and rep.total_ms >= rep.device_ms


def test_the_same_bytes_again_and_after_a_larger_image():
    small, large = G.case("odd"), G.case("blobs")
    ex = SiftExtractor()
    try:
        first = ex.extract(G.image(small), _options(small))
        again = ex.extract(G.image(small), _options(small))
        ex.extract(G.image(large), _options(large))
        after = ex.extract(G.image(small), _options(small))
        level = ex.stage(_capi.SIFT_STAGE_GRADIENT, 1, 2)
    finally:
        ex.close()
    for other in (again, after):
        assert first[0].tobytes() == other[0].tobytes() and first[1].tobytes() == other[1].tobytes()
    G.check_stage(G.recording(small), "grad 1 2", level, sampled=True)
    rec = G.recording(small)
    G.check_result(small, after[0], after[1], rec["raw"], rec["octave_level"], rec["angles"], after[2].first_level_to_keep)


def test_keypoints_without_descriptors(extractor):
    c = G.case("odd")
    kp, desc, rep = extractor.extract(G.image(c), _options(c), want_descriptors=False)
    assert desc is None and rep.num_windows_cut == 0
    G.assert_same_bits(kp, G.recording(c)["keypoints"], "keypoints")
    assert not extractor.features()[0].any()


def test_a_capacity_too_small_leaves_the_outputs_untouched(extractor):
    c = G.case("odd")
    need = c["cut"][2]
    im = np.ascontiguousarray(G.image(c))
    o = _options(c)
    for cap in (0, need - 1):
        kp, desc = np.full((need, 4), 7.0, dtype=np.float32), np.full((need, 128), 9, dtype=np.uint8)
        num, rep = C.c_int64(-1), _capi.SiftExtractReport()
        rc = _capi.lib().pp_sift_extract(extractor._h, C.byref(o), c["width"], c["height"], _capi.ptr(im, _capi.c_u8p), C.byref(rep), cap,
                                         _capi.ptr(kp, C.POINTER(C.c_float)), _capi.ptr(desc, _capi.c_u8p), C.byref(num))
        assert rc == _capi.PP_ERR_INVALID and num.value == need == rep.num_features
        assert np.all(kp == 7.0) and np.all(desc == 9)
    kp, desc, _ = extractor.extract(G.image(c), o, capacity=need)      # exactly enough
    assert len(kp) == need
    kp2, desc2, _ = extractor.extract(G.image(c), sift_extract_options(**dict(c["options"], max_num_features=1 << 20)))      # the first guess is cut at 2^16
    assert kp2.tobytes() == kp.tobytes() and desc2.tobytes() == desc.tobytes()


def test_the_stage_readers_refuse_what_is_not_there(extractor):
    fresh = SiftExtractor()
    try:
        with pytest.raises(_capi.PPError):
            fresh.stage(_capi.SIFT_STAGE_GAUSSIAN, 0, 0)      # no extraction yet
        with pytest.raises(_capi.PPError):
            fresh.features()
    finally:
        fresh.close()
    c = G.case("tiny")
    extractor.extract(G.image(c), _options(c))
    for kind, o, s in ((_capi.SIFT_STAGE_GAUSSIAN, 3, 0), (_capi.SIFT_STAGE_GAUSSIAN, -2, 0), (_capi.SIFT_STAGE_GAUSSIAN, 0, 5), (_capi.SIFT_STAGE_DOG, 0, 4),
                       (_capi.SIFT_STAGE_GRADIENT, 0, 3), (_capi.SIFT_STAGE_GRADIENT, 0, -1), (3, 0, 0)):
        with pytest.raises(_capi.PPError):
            extractor.stage(kind, o, s)
    assert extractor.stage(_capi.SIFT_STAGE_GAUSSIAN, 2, 4).shape == (3, 5) and extractor.stage(_capi.SIFT_STAGE_GRADIENT, 2, 2).shape == (3, 5, 2)
    with pytest.raises(_capi.PPError):
        extractor.candidates(3)


def test_the_python_layer_returns_the_reference_types():
    c = G.case("tiny")
    keypoints, descriptors = fe.ExtractSiftFeatures(G.image(c), fe.SiftExtractionOptions())
    rec = G.recording(c)
    assert len(keypoints) == len(rec["keypoints"]) == len(descriptors) and descriptors.dtype == np.uint8
    want = fe.FeatureKeypoint(*rec["keypoints"][0])
    got = keypoints[0]
    assert (got.x, got.y, got.a11, got.a12, got.a21, got.a22) == (want.x, want.y, want.a11, want.a12, want.a21, want.a22)
