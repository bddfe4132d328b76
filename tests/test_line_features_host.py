"""The host side of the line-feature generation (K19) without a device: ImageToWorld of csrc/camera_models.hpp through pp_camera_image_to_world against
the oracle's WorldToImage for all eleven models, the numpy mirror of feature_extraction.py against both, the aligned-count rule against the reference's
loop run literally, the counter-based generator, and the small functions around the line generation (FeatureKeypoint, ScaleKeypoints, MaskKeypoints,
LoadSiftFeaturesFromTextFile).

Bounds.  A numpy restatement of the reference's Newton iteration reaches 5e-11 normalised units with synthetic.default_intrinsics, about 5e-8 px at
f = 1010: the round trip is held to 1e-6 px, 20 times that.  The mirror and the C function restate the same iteration; they are compared at 1e-9
normalised units, and for every parameter set the mirror alone first shows that one more Newton step moves no result by more than 1e-10 (4.7e-11 at worst
for the default sets), which leaves the 1e-9 a 10x margin over what a different rounding of the last step can do."""
import ctypes as C

import numpy as np
import pytest

from privacy_preserving_sfm_amd import _capi, synthetic
from privacy_preserving_sfm_amd import feature_extraction as fe
from privacy_preserving_sfm_amd.bundle_adjustment import Camera, Image

F, CX, CY = 1000.0, 640.0, 480.0
# one stronger parameter set per distortion family
STRONG = {
    2: [F, CX, CY, -0.2], 3: [F, CX, CY, -0.2, 0.05], 4: [F, 1010.0, CX, CY, -0.2, 0.05, 0.005, -0.003],
    5: [F, 1010.0, CX, CY, 0.05, -0.01, 0.005, -0.001], 6: [F, 1010.0, CX, CY, -0.2, 0.05, 0.005, -0.003, 0.01, 0.05, -0.01, 0.002],
    7: [F, 1010.0, CX, CY, 0.9], 8: [F, CX, CY, -0.1], 9: [F, CX, CY, -0.1, 0.02],
    10: [F, 1010.0, CX, CY, -0.1, 0.02, 0.003, -0.002, 0.002, -0.001, 0.003, -0.002],
}


def _default(model):
    return synthetic.default_intrinsics(model)[:synthetic.NUM_PARAMS[model]]


@pytest.fixture(scope="module")
def keypoints():
    rng = np.random.default_rng(19)
    return np.stack([rng.uniform(0, 1280, 2000), rng.uniform(0, 960, 2000)], axis=1).astype(np.float32)


def _c_image_to_world(model, params, xy):
    return Camera(0, model, params).ImageToWorld(np.asarray(xy, dtype=np.float64))


def _oracle_pixels(oracle, model, params, uv):
    return np.array([oracle.world_to_image(model, np.asarray(params, dtype=np.float64), a, b) for a, b in uv])


@pytest.mark.parametrize("model", range(11))
def test_round_trip_against_the_oracle(oracle, keypoints, model):
    p = _default(model)
    xy = keypoints.astype(np.float64)
    uv = _c_image_to_world(model, p, xy)
    err = np.abs(_oracle_pixels(oracle, model, p, uv) - xy).max()
    print("model %d: round trip %.3g px" % (model, err))
    assert err <= 1e-6
    # and our own forward map on the host is the oracle's
    assert np.abs(Camera(0, model, p).WorldToImage(uv) - xy).max() <= 1e-6


@pytest.mark.parametrize("model,params", [(m, _default(m)) for m in range(11)] + sorted(STRONG.items()),
                         ids=["default-%d" % m for m in range(11)] + ["strong-%d" % m for m in sorted(STRONG)])
def test_the_mirror(oracle, keypoints, model, params):
    xy = keypoints.astype(np.float64)
    uv, iterations = fe.image_to_world(model, params, xy)
    # the precondition, by the mirror alone: every keypoint converges, and a step later it is where it was
    assert iterations.max() < fe.UNDISTORT_MAX_ITERATIONS
    later, _ = fe.image_to_world(model, params, xy, extra_iterations=1)
    moved = np.abs(later - uv).max()
    print("model %d: %d iterations at most, one step later %.3g" % (model, iterations.max(), moved))
    assert moved <= 1e-10
    if model in (0, 1, 7):
        assert iterations.max() == 0
    assert np.abs(_c_image_to_world(model, params, xy) - uv).max() <= 1e-9
    assert np.abs(_oracle_pixels(oracle, model, params, uv) - xy).max() <= 1e-6


def test_fov_branches(oracle):
    rng = np.random.default_rng(7)
    far = np.stack([rng.uniform(0, 1280, 200), rng.uniform(0, 960, 200)], axis=1)
    near = np.array([CX, CY]) + rng.uniform(-5, 5, (200, 2))                       # radius^2 < 1e-4 in normalised units
    for omega, xy, branch in ((0.005, far, "omega"), (0.3, near, "radius"), (0.3, far, "general"), (0.9, far, "general")):
        p = [F, 1010.0, CX, CY, omega]
        uv = _c_image_to_world(7, p, xy)
        r2 = (uv ** 2).sum(axis=1)
        if branch == "omega":
            assert omega * omega < 1e-4
        elif branch == "radius":
            assert omega * omega >= 1e-4 and np.all((((xy - [CX, CY]) / [F, 1010.0]) ** 2).sum(axis=1) < 1e-4)
        else:
            assert omega * omega >= 1e-4 and np.mean(r2 >= 1e-4) > 0.9
        bound = 1e-6
        if branch == "omega":
            # The reference's Undistortion uses in this branch the SAME factor 1 + e, e = omega^2 (r^2 / 3 - 1 / 12), as its Distortion (camera_models.h:1154
            # and :1193): there the two are no inverses of each other, the round trip is off by the factor (1 + e)^2 = 1 + 2 e + e^2.  That is the
            # reference's own error; the literal restatement has it too, and is held to 3 e of the largest distance from the principal point.
            e = omega * omega * np.maximum(1.0 / 12.0, np.abs(r2 / 3.0 - 1.0 / 12.0)).max()
            bound = 3.0 * e * np.abs(xy - [CX, CY]).max()
            lifted = (xy - [CX, CY]) / [F, 1010.0]
            factor = (omega * omega * (lifted ** 2).sum(axis=1)) / 3.0 - omega * omega / 12.0 + 1.0
            assert np.abs(uv - lifted * factor[:, None]).max() <= 1e-15      # the closed form itself
        err = np.abs(_oracle_pixels(oracle, 7, p, uv) - xy).max()
        print("FOV %s branch: round trip %.3g px (bound %.3g)" % (branch, err, bound))
        assert err <= bound, branch
        assert np.abs(fe.image_to_world(7, p, xy)[0] - uv).max() <= 1e-9, branch


def test_camera_entry_points_refuse_bad_arguments():
    L = _capi.lib()
    p = _capi.f64(synthetic.default_intrinsics(2))
    xy = np.zeros((1, 2))
    assert L.pp_camera_image_to_world(11, _capi.dp(p), 1, _capi.dp(xy), _capi.dp(xy)) == _capi.PP_ERR_INVALID
    assert L.pp_camera_world_to_image(-1, _capi.dp(p), 1, _capi.dp(xy), _capi.dp(xy)) == _capi.PP_ERR_INVALID
    assert L.pp_camera_image_to_world(2, None, 1, _capi.dp(xy), _capi.dp(xy)) == _capi.PP_ERR_INVALID
    assert L.pp_camera_image_to_world(2, _capi.dp(p), 0, None, None) == _capi.PP_OK


def _reference_loop(N, ratio):
    """extraction.cc:454-458 on the set's size"""
    size = 0
    with np.errstate(all="ignore"):
        while np.float64(size) / np.float64(N) < ratio:
            size += 1
    return size


def test_the_aligned_count():
    for N in range(41):
        for ratio in (0.0, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.999, 1.0):
            want = _reference_loop(N, ratio)
            assert fe.aligned_count(N, ratio) == want
            flags = fe.aligned_flags(5, 3, N, ratio)
            assert flags.shape == (N,) and int(flags.sum()) == want
            assert not fe.aligned_flags(5, 3, N, ratio, has_gravity=False).any()
    for ratio in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            fe.aligned_count(10, ratio)


def test_the_aligned_set_is_nested_and_spread():
    keys = fe.align_keys(1, 2, np.arange(5000))
    assert len(np.unique(keys)) == 5000 and np.array_equal(keys & np.uint64(0xFFFFFFFF), np.arange(5000, dtype=np.uint64))
    a, b = fe.aligned_flags(1, 2, 5000, 0.25), fe.aligned_flags(1, 2, 5000, 0.5)
    assert np.all(b[a]) and a.sum() == 1250 and b.sum() == 2500
    # a uniform subset: each half of the index range holds about half of it (4 standard errors of a hypergeometric count)
    assert abs(int(a[:2500].sum()) - 625) <= 4 * np.sqrt(1250 * 0.25 * 0.75)


def test_the_generator():
    idx = np.arange(100000)
    d = fe.draws(11, 4, idx)
    assert d.shape == (100000, 3) and d.dtype == np.float64
    assert np.array_equal(d, fe.draws(11, 4, idx))                       # the same seed: the same draws
    assert np.array_equal(d[500:600], fe.draws(11, 4, idx[500:600]))     # a draw is a function of its own index
    assert not np.array_equal(d, fe.draws(12, 4, idx)) and not np.array_equal(d, fe.draws(11, 5, idx))
    assert d.min() >= -1.0 and d.max() < 1.0
    n = len(idx)
    for c in range(3):
        # uniform in [-1, 1): mean 0 with variance 1/3; x^2 has mean 1/3 and variance 1/5 - 1/9 = 4/45
        assert abs(d[:, c].mean()) <= 4 * np.sqrt(1.0 / 3.0 / n)
        assert abs(d[:, c].var() - 1.0 / 3.0) <= 4 * np.sqrt(4.0 / 45.0 / n)
    assert np.abs(np.corrcoef(d.T) - np.eye(3)).max() <= 4 / np.sqrt(n)


def _images(counts, seed=3):
    rng = np.random.default_rng(seed)
    images, cameras, kps = [], {}, {}
    for k, n in enumerate(counts):
        model = k % 11
        cameras[k] = Camera(k, model, _default(model), 1280, 960)
        g = rng.normal(size=3)
        images.append(Image(10 + k, k, [1, 0, 0, 0], [0, 0, 0], gravity=None if k == 1 else g / np.linalg.norm(g)))
        kps[10 + k] = np.stack([rng.uniform(0, 1280, n), rng.uniform(0, 960, n)], axis=1).astype(np.float32)
    return images, cameras, kps


def test_an_images_lines_do_not_depend_on_the_batch():
    images, cameras, kps = _images([40, 30, 0, 65])
    whole = fe.generate_line_features(images, cameras, kps, 0.3, seed=9)
    assert whole["num_lines"] == 135 and whole["num_images_without_gravity"] == 1
    assert whole["num_aligned"] == sum(_reference_loop(n, 0.3) for n in (40, 0, 65)) and whole["num_degenerate"] == 0 and whole["num_newton_exhausted"] == 0
    assert [len(im.lines) for im in images] == [40, 30, 0, 65]
    assert all(l.Point3DId() == -1 for im in images for l in im.lines)
    assert not any(l.IsAligned() for l in images[1].lines)                      # no gravity: random lines only
    alone = fe.generate_line_features(images[3:], cameras, kps, 0.3, seed=9)
    reverse = fe.generate_line_features(images[::-1], cameras, kps, 0.3, seed=9)
    for rep in (alone, reverse):
        assert np.array_equal(rep["lines"][13], whole["lines"][13]) and np.array_equal(rep["aligned"][13], whole["aligned"][13])
    # what a line is: unit head, through the undistorted keypoint, orthogonal to its direction
    for im in images:
        k = im.image_id
        line, uv, d = whole["lines"][k], whole["uv"][k], whole["dirs"][k]
        if len(line) == 0:
            continue
        assert np.abs(np.linalg.norm(line[:, :2], axis=1) - 1).max() <= 1e-12
        assert np.abs(line[:, 0] * uv[:, 0] + line[:, 1] * uv[:, 1] + line[:, 2]).max() <= 1e-12 * np.abs(line).max()
        assert np.abs((line * d).sum(axis=1)).max() <= 1e-12 * np.linalg.norm(line, axis=1).max() * np.linalg.norm(d, axis=1).max()
        if im.HasGravity():
            assert np.array_equal(d[whole["aligned"][k]], np.tile(im.GravityDirection(), (int(whole["aligned"][k].sum()), 1)))
    with pytest.raises(ValueError):
        fe.generate_line_features(images, cameras, kps, 1.1)


def test_feature_keypoint():
    k = fe.FeatureKeypoint(3.5, 4.25)
    assert (k.x, k.y, k.a11, k.a12, k.a21, k.a22) == (3.5, 4.25, 1, 0, 0, 1) and all(isinstance(v, np.float32) for v in (k.x, k.a11))
    k = fe.FeatureKeypoint(1, 2, 2.0, np.pi / 2)
    assert abs(k.a11) < 1e-6 and abs(k.a12 + 2) < 1e-6 and abs(k.a21 - 2) < 1e-6 and abs(k.a22) < 1e-6
    assert abs(k.ComputeScale() - 2) < 1e-6 and abs(k.ComputeOrientation() - np.pi / 2) < 1e-6 and abs(k.ComputeShear()) < 1e-6
    k = fe.FeatureKeypoint.FromParameters(1, 2, 2.0, 3.0, 0.3, 0.2)
    assert abs(k.ComputeScaleX() - 2) < 1e-6 and abs(k.ComputeScaleY() - 3) < 1e-6 and abs(k.ComputeScale() - 2.5) < 1e-6
    assert abs(k.ComputeOrientation() - 0.3) < 1e-6 and abs(k.ComputeShear() - 0.2) < 1e-6
    k.Rescale(2.0)
    assert (k.x, k.y) == (2, 4) and abs(k.ComputeScaleX() - 4) < 1e-6 and abs(k.ComputeScaleY() - 6) < 1e-6
    k = fe.FeatureKeypoint(1, 2, 1, 2, 3, 4)
    k.Rescale(2.0, 0.5)
    assert (k.x, k.y, k.a11, k.a12, k.a21, k.a22) == (2, 1, 2, 1, 6, 2)
    with pytest.raises(ValueError):
        k.Rescale(0.0, 1.0)
    with pytest.raises(ValueError):
        fe.FeatureKeypoint(0, 0, -1.0, 0.0)


def test_scale_keypoints():
    cam = Camera(1, 0, [F, CX, CY], 1280, 960)
    kps = [fe.FeatureKeypoint(10, 20), fe.FeatureKeypoint(100, 50, 2.0, 0.0)]
    fe.ScaleKeypoints((1280, 960), cam, kps)                    # the same size: untouched
    assert (kps[0].x, kps[0].y, kps[1].a11) == (10, 20, 2)
    fe.ScaleKeypoints((640, 320), cam, kps)                     # x2 and x3
    assert (kps[0].x, kps[0].y) == (20, 60) and (kps[1].x, kps[1].y, kps[1].a11, kps[1].a22) == (200, 150, 4, 6)
    assert np.array_equal(fe.FeatureKeypointsToPointsVector(kps), np.array([[20, 60], [200, 150]], dtype=np.float32))


def test_mask_keypoints():
    mask = np.full((6, 8), 255, dtype=np.uint8)                  # 8 wide, 6 high
    mask[2, 3] = 0
    kps = [fe.FeatureKeypoint(0.5, 0.5), fe.FeatureKeypoint(3.9, 2.9),      # on the zero pixel (3, 2)
           fe.FeatureKeypoint(8.0, 1.0),                                     # x = 8: outside
           fe.FeatureKeypoint(7.99, 5.99), fe.FeatureKeypoint(2.0, 6.5),    # the last pixel; y = 6: outside
           fe.FeatureKeypoint(-0.5, 1.0),                                    # truncates to 0: inside, as in the reference
           fe.FeatureKeypoint(-1.5, 1.0)]                                    # truncates to -1: outside
    desc = np.arange(7 * 4, dtype=np.uint8).reshape(7, 4)
    kept, d = fe.MaskKeypoints(mask, kps, desc)
    assert [float(k.x) for k in kept] == [0.5, float(np.float32(7.99)), -0.5]
    assert np.array_equal(d, desc[[0, 3, 5]])
    kept, d = fe.MaskKeypoints(np.zeros((6, 8), dtype=np.uint8), kps, desc)
    assert kept == [] and d.shape == (0, 4)
    kept, d = fe.MaskKeypoints(np.stack([mask, 0 * mask, 0 * mask], axis=2), kps, desc)      # colour: the red channel decides
    assert len(kept) == 3


def test_load_sift_features_from_text_file(tmp_path):
    rng = np.random.default_rng(0)
    desc = rng.integers(0, 256, (5, 128))
    rows = [(10.5, 20.25, 2.0, 0.5), (0.0, 0.0, 1.0, 0.0), (1279.5, 959.5, 3.5, -1.0), (5.0, 6.0, 0.0, 3.0), (7.125, 8.5, 1.5, 1.5)]
    path = tmp_path / "features.txt"
    with open(path, "w") as f:
        f.write("5 128\n")
        for r, d in zip(rows, desc):
            f.write(" ".join("%r" % v for v in r) + " " + " ".join("%d" % v for v in d) + "\n")
    assert len(open(path).read().splitlines()) == 6
    kps, got = fe.LoadSiftFeaturesFromTextFile(str(path))
    assert got.dtype == np.uint8 and np.array_equal(got, desc)
    for k, r in zip(kps, rows):
        want = fe.FeatureKeypoint(*r)
        assert (k.x, k.y, k.a11, k.a12, k.a21, k.a22) == (want.x, want.y, want.a11, want.a12, want.a21, want.a22)
        assert abs(k.ComputeScale() - r[2]) < 1e-5
    with open(path, "w") as f:
        f.write("1 64\n")
    with pytest.raises(ValueError):
        fe.LoadSiftFeaturesFromTextFile(str(path))
