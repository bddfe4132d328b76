"""The observation model of synthetic.make_ba_scene: pixel noise on the lines, outlier observations, float32 storage - what the
mapper hands its global bundle adjustment instead of exact lines (reference src/base/database.cc:55-73 for the storage, the
outlier recipe of make_ransac_scene).  CPU only; residuals are the oracle's (reference src/base/cost_functions.h:62-100)."""
import numpy as np

from privacy_preserving_sfm_amd import synthetic

CFG2 = dict(num_cams=100, num_points=5000, track=8, seed=0xC0FFEE + 2, model=2)


def test_defaults_equal_explicit_zeros_array_for_array():
    for kw in (dict(num_cams=20, num_points=500, track=4, seed=0xC0FFEE + 1, model=2), dict(num_cams=30, num_points=400, track=5, seed=5, model=4, window=10, sort="pose")):
        a = synthetic.make_ba_scene(**kw)
        b = synthetic.make_ba_scene(line_noise_px=0.0, outlier_obs=0.0, quantise_float32=False, **kw)
        assert a.keys() == b.keys()
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k
        assert a["outlier_mask"].dtype == np.uint8 and a["outlier_mask"].shape == (len(a["obs_pose"]),) and not a["outlier_mask"].any()


def test_observation_model_leaves_the_rest_of_the_scene_alone():
    """the new random numbers come from a second generator: everything but the lines is what the exact scene has"""
    a = synthetic.make_ba_scene(**CFG2)
    b = synthetic.make_ba_scene(line_noise_px=0.5, outlier_obs=0.05, quantise_float32=True, **CFG2)
    for k in a:
        if k not in ("lines", "outlier_mask") and isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["lines"], b["lines"])


def test_outlier_share_and_inlier_floor():
    for share in (0.05, 0.013, 0.3):
        sc = synthetic.make_ba_scene(outlier_obs=share, **CFG2)
        M = len(sc["obs_pose"])
        mask = sc["outlier_mask"].astype(bool)
        assert abs(mask.mean() - share) <= 1.0 / M                                      # to one observation's rounding
        inliers = np.bincount(sc["obs_point"][~mask], minlength=5000)
        assert inliers.min() >= 2                                                      # every point keeps two inlier observations
        assert not mask[sc["obs_pose"] <= 1].any()                                     # the gauge images are not starved
        exact = synthetic.make_ba_scene(**CFG2)
        assert np.array_equal(sc["lines"][~mask], exact["lines"][~mask]) and not np.any(np.all(sc["lines"][mask] == exact["lines"][mask], axis=1))
    # pose-sorted scenes carry the mask with the observations
    a = synthetic.make_ba_scene(outlier_obs=0.05, **CFG2)
    b = synthetic.make_ba_scene(outlier_obs=0.05, sort="pose", **CFG2)
    order = np.lexsort((a["obs_point"], a["obs_pose"]))
    assert np.array_equal(b["outlier_mask"], a["outlier_mask"][order]) and np.array_equal(b["lines"], a["lines"][order])


def test_lines_are_unit_normalised():
    for kw in (dict(line_noise_px=0.5), dict(outlier_obs=0.05), dict(quantise_float32=True), dict(line_noise_px=0.5, outlier_obs=0.05, quantise_float32=True)):
        sc = synthetic.make_ba_scene(**CFG2, **kw)
        assert np.abs(np.hypot(sc["lines"][:, 0], sc["lines"][:, 1]) - 1.0).max() <= 4e-16, kw


def test_quantised_lines_round_trip_through_float32():
    """(a,b,c) are float32 values divided by their (a,b) norm in double: times that norm they are float32 values again, to 1 ulp"""
    sc = synthetic.make_ba_scene(line_noise_px=0.5, outlier_obs=0.05, quantise_float32=True, **CFG2)
    exact = synthetic.make_ba_scene(line_noise_px=0.5, outlier_obs=0.05, **CFG2)
    stored = exact["lines"].astype(np.float32)                                          # what the database holds
    norm = np.linalg.norm(stored[:, :2].astype(np.float64), axis=1, keepdims=True)
    back = (sc["lines"] * norm).astype(np.float32)
    ulp = np.spacing(np.abs(stored))
    assert np.all(np.abs(back.astype(np.float64) - stored.astype(np.float64)) <= ulp)
    assert np.abs(sc["lines"] - exact["lines"]).max() <= 2.0 ** -23 and not np.array_equal(sc["lines"], exact["lines"])


def test_inlier_residuals_at_ground_truth_have_the_noise_of_the_model(oracle):
    """40k observations, 0.5 px per axis: the signed pixel distance of the true projection from its line is N(0, 0.5) - the isotropic noise
    projected on the line normal (sampling error of the standard deviation at 38k inliers: 0.4 %); outliers are far off."""
    sigma = 0.5
    sc = synthetic.make_ba_scene(line_noise_px=sigma, outlier_obs=0.05, quantise_float32=True, **CFG2)
    assert len(sc["obs_pose"]) == 40000
    gt = dict(sc, poses=sc["gt_poses"], points=sc["gt_points"])
    _, r = oracle.ba_cost(gt)
    r = r.reshape(-1, 2)
    signed = r[:, 0] * sc["lines"][:, 0] + r[:, 1] * sc["lines"][:, 1]                  # the residual vector lies along the line normal (a,b)
    inl = ~sc["outlier_mask"].astype(bool)
    std = signed[inl].std()
    print("inlier residual std %.4f px (model %.2f), outlier rms %.1f px" % (std, sigma, np.sqrt((signed[~inl] ** 2).mean())))
    assert abs(std - sigma) <= 0.1 * sigma
    assert abs(signed[inl].mean()) <= 0.02 * sigma
    assert np.sqrt((signed[~inl] ** 2).mean()) > 50 * sigma
    # and without the model the same figure is rounding noise
    _, r0 = oracle.ba_cost(dict(synthetic.make_ba_scene(**CFG2), poses=sc["gt_poses"], points=sc["gt_points"]))
    assert np.abs(r0).max() < 1e-9
