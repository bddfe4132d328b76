"""K24 on the device: pp_sift_extract_to_matcher - the cut before the orientations and the descriptors, the kept features described by
k_sift_describe_kept straight into a pp_sift_handle.  With NO tolerance against pp_sift_extract_batch on another handle: keypoints, offsets, the
descriptor rows the matcher holds (pp_sift_get_descriptors), and what the matcher computes from them (top2 and match_pairs against a SiftMatcher built
from the batch call's arrays - this is what sees the rows' offsets).  The descriptor rows also against the recordings of the reference's CPU extractor
(tests/golden/sift) through the rule of tests/sift_extract_goldens.py, which does not depend on the code under test.  The four report counts that
cover the kept features only are ExtractOnHost's, restricted to the kept suffix by tests/sift_extract_kept_host_driver.cpp."""
import ctypes as C
import itertools

import numpy as np
import pytest

import sift_extract_goldens as G
from privacy_preserving_sfm_amd import _capi, feature_extraction as fe, feature_matching as fm
from privacy_preserving_sfm_amd.bundle_adjustment import Camera, Image
from privacy_preserving_sfm_amd.device import SiftExtractor, SiftMatcher, sift_extract_options, sift_match_options
from test_gpu_sift_extract_batch import COUNTS, IMAGES, SIX, _value
from test_sift_extract_kept_host import build_driver, kept_lines

pytestmark = pytest.mark.gpu

KEPT_ONLY = ("num_features_found", "num_two_orientations", "num_windows_cut", "num_descriptors_skipped")
FILES = {"blobs": G.case("blobs")["image"], "odd": G.case("odd")["image"], "tiny": G.case("tiny")["image"], "constant": G.case("constant")["image"],
         "chain_a": G.CHAIN["image_a"], "chain_b": G.CHAIN["image_b"]}
# the option sets: name -> (options that differ from the defaults, the recorded case of `odd` under them)
CONFIGS = {"max_20": (dict(max_num_features=20), "odd"), "max_36": (dict(max_num_features=36), "odd"), "max_49": (dict(max_num_features=49), "odd"),
           "max_8192": (dict(max_num_features=8192), "odd"), "upright": (dict(upright=1), "odd_upright"),
           "one_orientation": (dict(max_num_orientations=1), "odd_one_orientation"), "l2": (dict(normalization=1), "odd_l2"),
           "first_octave_0": (dict(first_octave=0), "odd_first_octave_0")}
PAIRS = list(itertools.permutations(range(len(SIX)), 2))


def _counts(rep):
    return {f: _value(rep, f) for f in COUNTS}


@pytest.fixture(scope="module")
def extractor():
    ex = SiftExtractor()
    yield ex
    ex.close()


@pytest.fixture(scope="module")
def batch():
    """pp_sift_extract_batch of the six images on a handle of its own, per option set: [(keypoints, descriptors, counts)], computed once"""
    ex = SiftExtractor()
    cache = {}

    def run(config):
        if config not in cache:
            out = ex.extract_batch([IMAGES[n] for n in SIX], sift_extract_options(**CONFIGS[config][0]))
            cache[config] = [(kp, desc, _counts(rep)) for kp, desc, rep in out]
            for kp, desc, _ in cache[config]:
                kp.setflags(write=False); desc.setflags(write=False)
        return cache[config]

    yield run
    ex.close()


@pytest.fixture(scope="module")
def host_counts(tmp_path_factory):
    """the kept-only counts of the six images under max_num_features 20, 36 and 49, from ExtractOnHost (the driver built plainly: no sanitizer here)"""
    exe = build_driver(tmp_path_factory.mktemp("sift_kept_gpu"), sanitize=False)
    keys = [(name, m) for name in SIX for m in (20, 36, 49)]
    sizes = {name: IMAGES[name].shape for name in SIX}
    lines = kept_lines(exe, [(FILES[name], sizes[name][1], sizes[name][0], dict(G.case("odd")["options"], max_num_features=m)) for name, m in keys])
    return {key: fields for key, (_, fields, _) in zip(keys, lines)}


def _recorded(name, config, count):
    """the last `count` (keypoints, descriptors) of the recording of image `name` under the option set, or None where there is no recording"""
    options, odd_case = CONFIGS[config]
    if name == "odd":
        c = G.case(odd_case)
    elif name in ("blobs", "tiny", "constant") and set(options) <= {"max_num_features", "normalization"}:
        c = G.case(name)      # (the recording holds every feature before the cut and the float descriptor before the last normalisation)
    else:
        return None
    rec = G.recording(c)
    total = len(rec["keypoints"])
    return rec["keypoints"][total - count:], G.finish_descriptors(rec["raw"], options.get("normalization", 0))[total - count:]


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_six_images_into_a_matcher(extractor, batch, host_counts, config):
    options = CONFIGS[config][0]
    want = batch(config)
    keypoints, reports, brep, matcher = extractor.extract_to_matcher([IMAGES[n] for n in SIX], sift_extract_options(**options))
    reference = SiftMatcher([desc for _, desc, _ in want])
    try:
        assert matcher.num_images == 6 and matcher.num_features == [len(kp) for kp, _, _ in want] == reference.num_features
        assert brep.num_images == 6 and brep.num_sub_batches == 1 and brep.num_features == sum(matcher.num_features) and brep.total_ms >= brep.device_ms > 0
        for i, name in enumerate(SIX):
            kp, desc, counts = want[i]
            got = matcher.descriptors(i)
            assert keypoints[i].dtype == np.float32 and keypoints[i].tobytes() == kp.tobytes(), name + ": keypoints"
            assert got.dtype == np.uint8 and got.shape == desc.shape and got.tobytes() == desc.tobytes(), name + ": descriptors"
            recorded = _recorded(name, config, len(kp))
            if recorded is not None:
                G.assert_same_bits(keypoints[i], recorded[0], name + ": keypoints against the recording")
                assert np.array_equal(got, recorded[1]), name + ": descriptors against the recording"
            # ---- the report: the batch call's, except the four counts that follow the features
            mine = _counts(reports[i])
            print(config, name, {f: (mine[f], counts[f]) for f in KEPT_ONLY})
            assert {f: v for f, v in mine.items() if f not in KEPT_ONLY} == {f: v for f, v in counts.items() if f not in KEPT_ONLY}, name
            assert mine["num_features_found"] == mine["num_features"] == len(kp)
            if counts["first_level_to_keep"] == 0:      # nothing cut: every count is the batch call's
                assert mine == counts, name
            if "max_num_features" in options and options["max_num_features"] < 8192:
                h = host_counts[(name, options["max_num_features"])]
                assert [mine[f] for f in KEPT_ONLY] == [h["found"], h["two_orientations"], h["windows_cut"], h["skipped"]], name
                assert mine["first_level_to_keep"] == h["first_level"]
            assert (reports[i].device_ms, reports[i].total_ms, list(reports[i].phase_ms)) == (0.0, 0.0, [0.0] * 5)
        if config == "max_8192":
            assert all(_counts(reports[i]) == want[i][2] for i in range(6))
        if config == "max_20":
            assert matcher.num_features[:4] == [28, 42, 2, 0] and reports[0].first_level_to_keep == 6 and reports[1].first_level_to_keep == 4
        # ---- what the matcher computes from the rows: the one-way scan of every ordered pair, and the matches with and without the cross-check
        for a, b in PAIRS:
            for x, y in zip(matcher.top2(a, b), reference.top2(a, b)):
                assert np.array_equal(x, y), (SIX[a], SIX[b])
        for cross_check in (1, 0):
            o = sift_match_options(cross_check=cross_check, min_num_matches=0)
            rep, got = matcher.match_pairs(PAIRS, o)
            ref_rep, ref = reference.match_pairs(PAIRS, o)
            assert rep.num_matches == ref_rep.num_matches and all(np.array_equal(x, y) for x, y in zip(got, ref))
            if config == "max_8192":
                assert rep.num_matches > 84
    finally:
        matcher.close()
        reference.close()


def _rows(extractor, names, **kw):
    keypoints, reports, brep, matcher = extractor.extract_to_matcher([IMAGES[n] for n in names], sift_extract_options(max_num_features=36), **kw)
    try:
        return {n: (keypoints[i].tobytes(), matcher.descriptors(i).tobytes(), _counts(reports[i])) for i, n in enumerate(names)}, brep, matcher.num_features
    finally:
        matcher.close()


def test_the_result_does_not_depend_on_the_split(extractor, batch):
    want = batch("max_36")
    whole, brep, _ = _rows(extractor, SIX)
    assert brep.num_sub_batches == 1
    for i, name in enumerate(SIX):
        assert whole[name][:2] == (want[i][0].tobytes(), want[i][1].tobytes()), name
    split, brep, sizes = _rows(extractor, SIX, workspace_bytes=1)      # every image alone: the store grows group by group
    assert brep.num_sub_batches == 6 and sizes == [len(kp) for kp, _, _ in want] and split == whole
    backwards, _, _ = _rows(extractor, SIX[::-1])
    assert backwards == whole
    backwards_split, brep, _ = _rows(extractor, SIX[::-1], workspace_bytes=1)      # (the image without a feature is now the third group)
    assert brep.num_sub_batches == 6 and backwards_split == whole
    for name in ("odd", "constant"):
        alone, brep, sizes = _rows(extractor, [name])
        assert alone[name] == whole[name] and brep.num_images == 1 and sizes == [len(want[SIX.index(name)][0])]
    again, _, _ = _rows(extractor, SIX)      # two calls in a row on one extractor (after smaller ones in the same workspace)
    twice, _, _ = _rows(extractor, SIX)
    assert again == twice == whole


def test_the_extractor_after_the_call():
    ex = SiftExtractor()
    try:
        ex.extract(IMAGES["odd"])
        assert len(ex.candidates(0)) > 0
        ex.extract_batch([IMAGES["tiny"], IMAGES["odd"]])
        assert len(ex.batch_features(1)[2]) == 101
        keypoints, _, _, matcher = ex.extract_to_matcher([IMAGES["tiny"], IMAGES["odd"]])
        matcher.close()
        assert [len(k) for k in keypoints] == [2, 101]
        for reader in (lambda: ex.stage(_capi.SIFT_STAGE_GAUSSIAN, 0, 0), lambda: ex.candidates(0), ex.features, lambda: ex.batch_features(0)):
            with pytest.raises(_capi.PPError) as e:
                reader()
            assert e.value.code == _capi.PP_ERR_INVALID
        c = G.case("odd")
        kp, desc, rep = ex.extract(IMAGES["odd"])      # the next single extraction: its readers work again
        raw, octave_level, angles = ex.features()
        G.check_result(c, kp, desc, raw, octave_level, angles, rep.first_level_to_keep)
        assert len(ex.candidates(0)) == rep.octave_candidates[1]
    finally:
        ex.close()


def test_a_matcher_outlives_its_extractor_and_an_empty_one_matches():
    ex = SiftExtractor()
    keypoints, reports, brep, empty = ex.extract_to_matcher([IMAGES["constant"]])
    _, _, _, matcher = ex.extract_to_matcher([IMAGES["chain_a"], IMAGES["chain_b"]])
    ex.close()
    try:
        assert empty.num_features == [0] and len(keypoints[0]) == 0 and brep.num_features == 0 and reports[0].num_keypoints == 0
        assert empty.descriptors(0).shape == (0, 128)
        for cross_check in (1, 0):
            rep, out = empty.match_pairs([(0, 0)], sift_match_options(cross_check=cross_check, min_num_matches=0))
            assert rep.num_matches == 0 and len(out) == 1 and len(out[0]) == 0
        assert all(len(a) == 0 for a in empty.top2(0, 0))
        rep, out = matcher.match_pairs([(0, 1)])
        assert len(out[0]) == 84      # (tests/test_gpu_sift_extract_chain.py: the reference's features under the reference's rule give 84)
    finally:
        empty.close()
        matcher.close()


def test_a_capacity_too_small_leaves_no_matcher(extractor):
    names = ["odd", "constant", "tiny"]
    ims = [np.ascontiguousarray(IMAGES[n]) for n in names]
    table = (_capi.SiftBatchImage * 3)()
    for i, im in enumerate(ims):
        table[i].width, table[i].height, table[i].grey = im.shape[1], im.shape[0], _capi.ptr(im, _capi.c_u8p)
    o = sift_extract_options()
    need = 101 + 0 + 2
    for cap in (0, need - 1, need):
        brep, reps, offsets = _capi.SiftBatchReport(), (_capi.SiftExtractReport * 3)(), np.full(4, -1, dtype=np.int64)
        kp, handle = np.full((need, 4), 7.0, dtype=np.float32), C.c_void_p(0x5A5A)
        rc = _capi.lib().pp_sift_extract_to_matcher(extractor._h, C.byref(o), 3, table, 0, C.byref(brep), reps, cap, _capi.ptr(kp, C.POINTER(C.c_float)),
                                                    _capi.ptr(offsets, C.POINTER(C.c_int64)), C.byref(handle))
        assert list(offsets) == [0, 101, 101, 103] and brep.num_features == need and [r.num_features for r in reps] == [101, 0, 2]
        if cap < need:
            assert rc == _capi.PP_ERR_INVALID and handle.value is None and np.all(kp == 7.0)
        else:
            assert rc == _capi.PP_OK and handle.value
            matcher = SiftMatcher.from_handle(handle, offsets)
            assert matcher.num_features == [101, 0, 2] and len(matcher.descriptors(2)) == 2
            matcher.close()
    with pytest.raises(_capi.PPError):
        extractor.extract_to_matcher([IMAGES[n] for n in names], capacity=need - 1)
    keypoints, _, _, matcher = extractor.extract_to_matcher([IMAGES[n] for n in names], sift_extract_options(max_num_features=1 << 20))      # the retry
    matcher.close()
    assert [len(k) for k in keypoints] == [101, 0, 2]


def test_the_descriptor_reader_on_any_handle():
    given = [np.arange(3 * 128, dtype=np.uint8).reshape(3, 128), np.zeros((0, 128), dtype=np.uint8), np.full((130, 128), 255, dtype=np.uint8)]
    m = SiftMatcher(given)
    try:
        for i, d in enumerate(given):
            assert np.array_equal(m.descriptors(i), d)
        out, num = np.full((130, 128), 9, dtype=np.uint8), C.c_int64(-5)
        L = _capi.lib()
        assert L.pp_sift_get_descriptors(m._h, 2, _capi.ptr(out, _capi.c_u8p), 129, C.byref(num)) == _capi.PP_ERR_INVALID and num.value == 130 and np.all(out == 9)
        for image in (-1, 3):
            assert L.pp_sift_get_descriptors(m._h, image, _capi.ptr(out, _capi.c_u8p), 130, C.byref(num)) == _capi.PP_ERR_INVALID
        assert L.pp_sift_get_descriptors(m._h, 1, None, 0, C.byref(num)) == _capi.PP_OK and num.value == 0
    finally:
        m.close()


def test_phase_timings(extractor):
    _, _, brep, matcher = extractor.extract_to_matcher([IMAGES["blobs"], IMAGES["odd"]], sift_extract_options(phase_timings=1))
    matcher.close()
    assert all(ms > 0 for ms in brep.phase_ms) and brep.device_ms >= sum(brep.phase_ms) * 0.99 and brep.total_ms >= brep.device_ms


def test_the_chain_through_the_matcher():
    """extract_features_to_lines(to_matcher=True), then Match: the 84 matches and the lines of the default route"""
    w, h = G.CHAIN["width"], G.CHAIN["height"]
    bitmaps = {1: IMAGES["chain_a"], 2: IMAGES["chain_b"]}
    cameras = {1: Camera(1, 1, [120.0, 120.0, w / 2.0, h / 2.0], w, h)}

    def images():
        return [Image(2, 1, [1, 0, 0, 0], [0, 0, 0], gravity=[0.0, 1.0, 0.0]), Image(1, 1, [1, 0, 0, 0], [0, 0, 0], gravity=[0.0, 1.0, 0.0])]      # (not in id order)

    images_a, images_b = images(), images()
    a = fe.extract_features_to_lines(images_a, cameras, bitmaps, fe.SiftExtractionOptions())
    b = fe.extract_features_to_lines(images_b, cameras, bitmaps, fe.SiftExtractionOptions(), to_matcher=True)
    assert "descriptors" not in b and "matcher" not in a and isinstance(b["matcher"], fm.FeatureMatcher)
    default = fm.FeatureMatcher(fm.SiftMatchingOptions(), a["descriptors"])
    try:
        assert b["matcher"].image_ids_ == [1, 2]
        want, got = default.Match([(1, 2), (2, 1)]), b["matcher"].Match([(1, 2), (2, 1)])
        assert list(got) == list(want) == [(1, 2)] and np.array_equal(got[(1, 2)], want[(1, 2)]) and len(got[(1, 2)]) == 84
        swapped = b["matcher"].Match([(2, 1)])
        assert np.array_equal(swapped[(2, 1)], default.Match([(2, 1)])[(2, 1)])
    finally:
        default.close()
        b["matcher"].close()
    assert a["num_lines"] == b["num_lines"] and all(a["keypoints"][k].tobytes() == b["keypoints"][k].tobytes() for k in (1, 2))
    assert a["lines"]["num_lines"] == b["lines"]["num_lines"]
    for x, y in zip(images_a, images_b):
        assert x.image_id == y.image_id and len(x.lines) == len(y.lines) == a["num_lines"][x.image_id] > 15
        assert all(p.Line().tobytes() == q.Line().tobytes() and p.IsAligned() == q.IsAligned() for p, q in zip(x.lines, y.lines))
    two = SiftMatcher([np.zeros((1, 128), dtype=np.uint8)] * 2)
    try:
        for ids in ([1], [1, 1]):      # one distinct id per image of the matcher
            with pytest.raises(ValueError):
                fm.FeatureMatcher.from_matcher(fm.SiftMatchingOptions(), ids, two)
    finally:
        two.close()
