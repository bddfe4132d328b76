"""K23 on the device: pp_sift_extract_batch - the images of a batch through the octaves in lock-step, their descriptors by k_sift_describe_wave, one
wavefront per feature.  With NO tolerance: every image of a batch against the recording of the reference's CPU extractor (tests/golden/sift) where it
has one, and byte for byte against pp_sift_extract of that image alone on another handle - keypoints, descriptors, the float descriptors before the
last normalisation, the report's counts.  The result does not depend on the batch: alone, twice, reversed, split into sub-batches, after a larger batch
on the same handle."""
import ctypes as C

import numpy as np
import pytest

import sift_extract_goldens as G
from privacy_preserving_sfm_amd import _capi, feature_extraction as fe
from privacy_preserving_sfm_amd.bundle_adjustment import Camera, Image
from privacy_preserving_sfm_amd.device import SiftExtractor, sift_extract_options
from test_sift_describe_wave_host import SMALL, small_image

pytestmark = pytest.mark.gpu

COUNTS = [f for f, _ in _capi.SiftExtractReport._fields_ if f not in ("phase_ms", "device_ms", "total_ms", "reserved_")]


def _chain(which):
    return np.fromfile(G.GOLDEN + "/" + G.CHAIN[which], dtype=np.uint8).reshape(G.CHAIN["height"], G.CHAIN["width"])


IMAGES = {"blobs": G.image(G.case("blobs")), "odd": G.image(G.case("odd")), "tiny": G.image(G.case("tiny")), "constant": G.image(G.case("constant")),
          "chain_a": _chain("image_a"), "chain_b": _chain("image_b")}
SIX = ["blobs", "odd", "tiny", "constant", "chain_a", "chain_b"]


@pytest.fixture(scope="module")
def batcher():
    ex = SiftExtractor()
    yield ex
    ex.close()


@pytest.fixture(scope="module")
def single():
    """the single call on a handle of its own: the on-device reference of the batch"""
    ex = SiftExtractor()
    cache = {}

    def extract(name, image=None, want_descriptors=True, **options):
        key = (name, want_descriptors, tuple(sorted(options.items())))
        if key not in cache:
            kp, desc, rep = ex.extract(IMAGES[name] if image is None else image, sift_extract_options(**options), want_descriptors=want_descriptors)
            raw, octave_level, angles = ex.features()
            cache[key] = (kp, desc, {f: _value(rep, f) for f in COUNTS}, raw.copy(), octave_level.copy(), angles.copy())
        return cache[key]

    yield extract
    ex.close()


def _value(rep, field):
    v = getattr(rep, field)
    return list(v) if hasattr(v, "__len__") else v


def _same(got, want, what, features=None):
    """(keypoints, descriptors, report) of one image of a batch against the single call's"""
    kp, desc, rep = got
    assert kp.dtype == np.float32 and kp.tobytes() == want[0].tobytes(), what + ": keypoints"
    if want[1] is None:
        assert desc is None, what
    else:
        assert desc.dtype == np.uint8 and desc.tobytes() == want[1].tobytes(), what + ": descriptors"
    assert {f: _value(rep, f) for f in COUNTS} == want[2], what + ": report"
    assert (rep.device_ms, rep.total_ms, list(rep.phase_ms)) == (0.0, 0.0, [0.0] * 5)
    if features is not None:
        for a, b, part in zip(features, want[3:], ("raw", "octave_level", "angles")):
            assert a.tobytes() == b.tobytes(), what + ": " + part


def test_six_images_of_six_sizes_in_one_batch(batcher, single):
    out = batcher.extract_batch([IMAGES[n] for n in SIX])
    brep = batcher.last_batch_report
    assert len(out) == 6 and brep.num_images == 6 and brep.num_sub_batches == 1 and brep.workspace_bytes > 0
    assert brep.num_features == sum(len(kp) for kp, _, _ in out) and list(brep.phase_ms) == [0.0] * 5 and brep.total_ms >= brep.device_ms > 0
    for i, name in enumerate(SIX):
        features = batcher.batch_features(i)
        _same(out[i], single(name), name, features)
        if name in G.CASE_NAMES:
            kp, desc, rep = out[i]
            G.check_result(G.case(name), kp, desc, features[0], features[1], features[2], rep.first_level_to_keep)
            assert rep.num_features == len(kp) == G.case(name)["cut"][2] and rep.num_descriptors_skipped == 0
    assert len(out[SIX.index("constant")][0]) == 0 and len(out[0][0]) == 225 and out[0][2].num_windows_cut == 116 and out[0][2].num_two_orientations == 24
    with pytest.raises(_capi.PPError):
        batcher.batch_features(6)


def test_the_offsets_of_the_c_call(batcher):
    ims = [np.ascontiguousarray(IMAGES[n]) for n in SIX]
    table = (_capi.SiftBatchImage * 6)()
    for i, im in enumerate(ims):
        table[i].width, table[i].height, table[i].grey = im.shape[1], im.shape[0], _capi.ptr(im, _capi.c_u8p)
    o = sift_extract_options()
    brep, reps, offsets = _capi.SiftBatchReport(), (_capi.SiftExtractReport * 6)(), np.full(7, -1, dtype=np.int64)
    kp, desc = np.zeros((4096, 4), dtype=np.float32), np.zeros((4096, 128), dtype=np.uint8)
    _capi.check(_capi.lib().pp_sift_extract_batch(batcher._h, C.byref(o), 6, table, 0, C.byref(brep), reps, 4096, _capi.ptr(kp, C.POINTER(C.c_float)),
                                                  _capi.ptr(desc, _capi.c_u8p), _capi.ptr(offsets, C.POINTER(C.c_int64))))
    assert offsets[0] == 0 and all(offsets[i + 1] - offsets[i] == reps[i].num_features for i in range(6)) and offsets[6] == brep.num_features
    k = SIX.index("constant")
    assert offsets[k] == offsets[k + 1] and offsets[1] == 225
    assert not kp[offsets[6]:].any() and not desc[offsets[6]:].any()      # nothing behind the last feature


VARIANTS = {"first_octave_0": ("odd_first_octave_0", dict(first_octave=0)), "upright": ("odd_upright", dict(upright=1)),
            "one_orientation": ("odd_one_orientation", dict(max_num_orientations=1)), "l2": ("odd_l2", dict(normalization=1)),
            "cut_between_levels": ("odd_cut_between_levels", dict(max_num_features=36)), "cut_at_level_boundary": ("odd_cut_at_level_boundary", dict(max_num_features=49))}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_the_option_variants(batcher, single, variant):
    case_name, options = VARIANTS[variant]
    c = G.case(case_name)
    assert all(c["options"][k] == v for k, v in options.items())
    out = batcher.extract_batch([IMAGES["odd"], IMAGES["blobs"]], sift_extract_options(**options))
    for i, name in enumerate(("odd", "blobs")):
        _same(out[i], single(name, **options), name, batcher.batch_features(i))
    raw, octave_level, angles = batcher.batch_features(0)
    G.check_result(c, out[0][0], out[0][1], raw, octave_level, angles, out[0][2].first_level_to_keep)
    if "max_num_features" in options:      # the cut is per image
        assert len(out[0][0]) == c["cut"][2] < out[0][2].num_features_found and out[1][2].first_level_to_keep > 0


def test_alone_twice_and_reversed(batcher, single):
    alone = batcher.extract_batch([IMAGES["odd"]])
    _same(alone[0], single("odd"), "a batch of one", batcher.batch_features(0))
    twice = batcher.extract_batch([IMAGES["blobs"], IMAGES["blobs"]])
    for i in range(2):
        _same(twice[i], single("blobs"), "the same image twice", batcher.batch_features(i))
    backwards = batcher.extract_batch([IMAGES[n] for n in reversed(SIX)])
    for i, name in enumerate(reversed(SIX)):
        _same(backwards[i], single(name), "reversed: " + name, batcher.batch_features(i))


def test_the_result_does_not_depend_on_the_split(batcher, single):
    whole = batcher.extract_batch([IMAGES[n] for n in SIX], workspace_bytes=0)
    assert batcher.last_batch_report.num_sub_batches == 1
    split = batcher.extract_batch([IMAGES[n] for n in SIX], workspace_bytes=1)
    assert batcher.last_batch_report.num_sub_batches == 6
    for i, name in enumerate(SIX):
        _same(split[i], single(name), name, batcher.batch_features(i))
        assert split[i][0].tobytes() == whole[i][0].tobytes() and split[i][1].tobytes() == whole[i][1].tobytes()
    # two sub-batches of three: what the first three need is the target
    batcher.extract_batch([IMAGES[n] for n in SIX[:3]])
    need = batcher.last_batch_report.workspace_bytes
    halves = batcher.extract_batch([IMAGES[n] for n in SIX], workspace_bytes=need)
    assert batcher.last_batch_report.num_sub_batches == 2 and batcher.last_batch_report.workspace_bytes == need
    for i, name in enumerate(SIX):
        _same(halves[i], single(name), name, batcher.batch_features(i))


def test_keypoints_without_descriptors(batcher, single):
    out = batcher.extract_batch([IMAGES["odd"], IMAGES["blobs"]], want_descriptors=False)
    for i, name in enumerate(("odd", "blobs")):
        _same(out[i], single(name, want_descriptors=False), name)
        assert out[i][1] is None and out[i][2].num_windows_cut == 0
        raw, octave_level, angles = batcher.batch_features(i)
        assert len(raw) == out[i][2].num_features_found > 0 and not raw.any()
    G.assert_same_bits(out[0][0], G.recording(G.case("odd"))["keypoints"], "keypoints")


def test_a_capacity_too_small_leaves_the_outputs_untouched(batcher, single):
    names = ["odd", "constant", "tiny"]
    ims = [np.ascontiguousarray(IMAGES[n]) for n in names]
    table = (_capi.SiftBatchImage * 3)()
    for i, im in enumerate(ims):
        table[i].width, table[i].height, table[i].grey = im.shape[1], im.shape[0], _capi.ptr(im, _capi.c_u8p)
    o = sift_extract_options()
    need = 101 + 0 + 2

    def call(cap):
        brep, reps, offsets = _capi.SiftBatchReport(), (_capi.SiftExtractReport * 3)(), np.full(4, -1, dtype=np.int64)
        kp, desc = np.full((need, 4), 7.0, dtype=np.float32), np.full((need, 128), 9, dtype=np.uint8)
        rc = _capi.lib().pp_sift_extract_batch(batcher._h, C.byref(o), 3, table, 0, C.byref(brep), reps, cap, _capi.ptr(kp, C.POINTER(C.c_float)),
                                               _capi.ptr(desc, _capi.c_u8p), _capi.ptr(offsets, C.POINTER(C.c_int64)))
        return rc, brep, reps, offsets, kp, desc

    for cap in (0, need - 1):
        rc, brep, reps, offsets, kp, desc = call(cap)
        assert rc == _capi.PP_ERR_INVALID and list(offsets) == [0, 101, 101, 103] and brep.num_features == need and brep.num_images == 3
        assert [r.num_features for r in reps] == [101, 0, 2] and reps[0].num_octaves == 4
        assert np.all(kp == 7.0) and np.all(desc == 9)
    rc, brep, reps, offsets, kp, desc = call(need)      # exactly enough
    assert rc == _capi.PP_OK and list(offsets) == [0, 101, 101, 103]
    assert kp[:101].tobytes() == single("odd")[0].tobytes() and desc[101:].tobytes() == single("tiny")[1].tobytes()
    out = batcher.extract_batch([IMAGES[n] for n in names], sift_extract_options(max_num_features=1 << 20), capacity=None)
    assert [len(kp) for kp, _, _ in out] == [101, 0, 2]
    with pytest.raises(_capi.PPError):
        batcher.extract_batch([IMAGES[n] for n in names], capacity=need - 1)


def test_the_handle_after_a_batch():
    ex = SiftExtractor()
    try:
        with pytest.raises(_capi.PPError):
            ex.batch_features(0)      # no batch yet
        large = ex.extract_batch([IMAGES[n] for n in SIX])
        for reader in (lambda: ex.stage(_capi.SIFT_STAGE_GAUSSIAN, 0, 0), lambda: ex.candidates(0), ex.features):
            with pytest.raises(_capi.PPError):
                reader()
        small = ex.extract_batch([IMAGES["tiny"], IMAGES["odd"]])      # a smaller batch in the workspace of the larger one
        assert small[0][0].tobytes() == large[2][0].tobytes() and small[0][1].tobytes() == large[2][1].tobytes()
        assert small[1][0].tobytes() == large[1][0].tobytes() and small[1][1].tobytes() == large[1][1].tobytes()
        c = G.case("odd")
        raw, octave_level, angles = ex.batch_features(1)
        G.check_result(c, small[1][0], small[1][1], raw, octave_level, angles, small[1][2].first_level_to_keep)
        kp, desc, rep = ex.extract(IMAGES["odd"])      # a single extraction: its readers work again, the batch is gone
        raw, octave_level, angles = ex.features()
        G.check_result(c, kp, desc, raw, octave_level, angles, rep.first_level_to_keep)
        G.check_stage(G.recording(c), "grad 1 2", ex.stage(_capi.SIFT_STAGE_GRADIENT, 1, 2), sampled=True)
        assert len(ex.candidates(0)) == rep.octave_candidates[1]
        with pytest.raises(_capi.PPError):
            ex.batch_features(0)
    finally:
        ex.close()


def test_phase_timings_of_the_batch(batcher):
    batcher.extract_batch([IMAGES["blobs"], IMAGES["odd"]], sift_extract_options(phase_timings=1))
    rep = batcher.last_batch_report
    assert all(ms > 0 for ms in rep.phase_ms) and rep.device_ms >= sum(rep.phase_ms) * 0.99 and rep.total_ms >= rep.device_ms


def test_windows_of_less_than_one_chunk(batcher, single):
    """descriptor windows of 40 pixels (and keypoints with two of them): less than the 64 lanes of the wavefront that describes them"""
    options = {k: SMALL["options"][k] for k in ("first_octave", "num_octaves")}
    out = batcher.extract_batch([small_image(), IMAGES["tiny"], small_image()], sift_extract_options(**options))
    for i in (0, 2):
        _same(out[i], single(SMALL["name"], image=small_image(), **options), SMALL["name"], batcher.batch_features(i))
        assert len(out[i][0]) == 4 and out[i][2].num_windows_cut == 4 and out[i][2].num_two_orientations == 2
    _same(out[1], single("tiny", **options), "tiny", batcher.batch_features(1))


def test_the_python_layer(single):
    found = fe.ExtractSiftFeaturesBatch([IMAGES["tiny"], IMAGES["odd"]], fe.SiftExtractionOptions())
    assert len(found) == 2
    for (keypoints, descriptors), name in zip(found, ("tiny", "odd")):
        rec = G.recording(G.case(name))
        assert len(keypoints) == len(rec["keypoints"]) == len(descriptors) and descriptors.dtype == np.uint8
        want, got = fe.FeatureKeypoint(*rec["keypoints"][0]), keypoints[0]
        assert isinstance(got, fe.FeatureKeypoint)
        assert (got.x, got.y, got.a11, got.a12, got.a21, got.a22) == (want.x, want.y, want.a11, want.a12, want.a21, want.a22)
        assert descriptors.tobytes() == single(name)[1].tobytes()
    arrays = fe.ExtractSiftFeaturesBatch([IMAGES["tiny"]], as_arrays=True)
    assert arrays[0][0].tobytes() == single("tiny")[0].tobytes()
    with pytest.raises(ValueError):
        fe.ExtractSiftFeaturesBatch([IMAGES["tiny"]], fe.SiftExtractionOptions(max_num_features=0))

    w, h = G.CHAIN["width"], G.CHAIN["height"]
    bitmaps = {1: IMAGES["chain_a"], 2: IMAGES["chain_b"]}
    cameras = {1: Camera(1, 1, [120.0, 120.0, w / 2.0, h / 2.0], w, h)}
    results = []
    for batched in (True, False):
        images = [Image(1, 1, [1, 0, 0, 0], [0, 0, 0], gravity=[0.0, 1.0, 0.0]), Image(2, 1, [1, 0, 0, 0], [0, 0, 0], gravity=[0.0, 1.0, 0.0])]
        results.append((fe.extract_features_to_lines(images, cameras, bitmaps, fe.SiftExtractionOptions(), batched=batched), images))
    (a, images_a), (b, images_b) = results
    for image_id, name in ((1, "chain_a"), (2, "chain_b")):
        assert a["keypoints"][image_id].tobytes() == b["keypoints"][image_id].tobytes() == single(name)[0].tobytes()
        assert a["descriptors"][image_id].tobytes() == b["descriptors"][image_id].tobytes() == single(name)[1].tobytes()
        assert a["num_lines"][image_id] == b["num_lines"][image_id] == len(single(name)[0]) > 15
    for x, y in zip(images_a, images_b):
        assert len(x.lines) == len(y.lines) == a["num_lines"][x.image_id]
        assert all(p.Line().tobytes() == q.Line().tobytes() and p.IsAligned() == q.IsAligned() for p, q in zip(x.lines, y.lines))
