"""The global refinement loop's LOGIC on the CPU (reference src/controllers/incremental_mapper.cc:102-124, src/sfm/incremental_mapper.cc:893-939,
src/base/reconstruction.cc:302-397): tests/refinement_oracle.py runs it with the oracle's solver and filters on a small noisy scene, and
Reconstruction.Normalize is checked against a restatement written here.  No GPU."""
import numpy as np

import refinement_oracle
from privacy_preserving_sfm_amd import synthetic
from privacy_preserving_sfm_amd.bundle_adjustment import (BundleAdjuster, GlobalBundleAdjustmentConfig, GlobalBundleAdjustmentOptions, IncrementalMapperOptions,
                                                          Reconstruction)


def _obs_refs(scene):
    """(image_id, line_idx) of every observation of a flat scene, as Reconstruction.from_scene numbers them"""
    count, refs = {}, []
    for c in scene["obs_pose"]:
        k = count.get(int(c), 0)
        count[int(c)] = k + 1
        refs.append((int(c), k))
    return refs


def _normalize_numpy(poses, points, extent=10.0, p0=0.1, p1=0.9):
    """Reconstruction::Normalize(use_images = true) restated directly: reconstruction.cc:316-396"""
    C = poses.shape[0]
    R = np.array([synthetic.quat_to_rot(q / np.linalg.norm(q)) for q in poses[:, :4]])
    centres = np.array([-R[c].T @ poses[c, 4:] for c in range(C)])
    xs = [sorted(np.float32(v) for v in centres[:, a]) for a in range(3)]          # float casts, one sort per axis (:333-352)
    i0 = int(p0 * (C - 1)) if C > 3 else 0                                           # :354-357
    i1 = int(p1 * (C - 1)) if C > 3 else C - 1
    lo = np.array([float(xs[a][i0]) for a in range(3)]); hi = np.array([float(xs[a][i1]) for a in range(3)])
    mean = np.array([sum(float(v) for v in xs[a][i0:i1 + 1]) for a in range(3)]) / (i1 - i0 + 1)      # :362-368
    old = np.linalg.norm(hi - lo)
    scale = 1.0 if old < np.finfo(float).eps else extent / old
    out = poses.copy()
    for c in range(C):
        out[c, 4:] = synthetic.quat_to_rot(poses[c, :4]) @ -((centres[c] - mean) * scale)              # tvec = q * -centre (:382-390)
    return out, (points - mean) * scale, mean, scale


def test_normalize_equals_the_numpy_restatement():
    for C, seed in ((20, 3), (3, 4), (101, 5)):
        sc = synthetic.make_ba_scene(C, 200, 3, seed=seed, model=2)
        rng = np.random.default_rng(seed)
        sc["poses"][:, 4:] += rng.normal(0, 0.5, (C, 3))                # (off the circle: the percentiles pick different images per axis)
        rec = Reconstruction.from_scene(sc)
        rec.Normalize()
        poses, points, _ = refinement_oracle.parameters(rec)
        want_poses, want_points, mean, scale = _normalize_numpy(sc["poses"], sc["points"])
        assert np.abs(mean).max() > 1e-3 and abs(scale - 1.0) > 1e-3
        assert np.allclose(poses, want_poses, rtol=1e-13, atol=1e-13) and np.allclose(points, want_points, rtol=1e-13, atol=1e-13)
        assert np.array_equal(poses[:, :4], sc["poses"][:, :4])
        # the robust box of the projection centres now has the asked diagonal (to float32: the box is read from float coordinates)
        R = np.array([synthetic.quat_to_rot(q) for q in poses[:, :4]])
        centres = np.sort(np.array([-R[c].T @ poses[c, 4:] for c in range(C)]), axis=0)
        i0, i1 = (int(0.1 * (C - 1)), int(0.9 * (C - 1))) if C > 3 else (0, C - 1)
        assert abs(np.linalg.norm(centres[i1] - centres[i0]) - 10.0) < 1e-5
    one = Reconstruction.from_scene(synthetic.make_ba_scene(2, 20, 2, seed=1, model=2))
    del one.images[1]
    before = one.images[0].tvec.copy()
    one.Normalize()                                                      # fewer than two images: nothing happens (:311-314)
    assert np.array_equal(one.images[0].tvec, before)


def test_normalize_leaves_every_line_residual_unchanged(oracle):
    """a similarity transform of cameras and points cannot change a reprojection: 1e-9 relative on every residual of a noisy scene"""
    sc = synthetic.make_ba_scene(20, 500, 4, seed=0xC0FFEE + 1, model=2, **refinement_oracle.NOISY)
    rec = Reconstruction.from_scene(sc)
    scene0 = rec._filter_scene()[0]
    r0 = oracle.ba_eval(scene0)[0]
    rec.Normalize(extent=3.0, p0=0.2, p1=0.7)
    rec.Normalize()
    scene1 = rec._filter_scene()[0]
    r1 = oracle.ba_eval(scene1)[0]
    assert np.abs(scene1["points"] - scene0["points"]).max() > 0.1
    assert np.abs(r0).max() > 100 and np.abs(r1 - r0).max() <= 1e-9 * np.abs(r0).max()


def test_global_bundle_adjustment_options_preset():
    few, many = GlobalBundleAdjustmentOptions(9), GlobalBundleAdjustmentOptions(10)
    so = many.solver_options
    assert (so.function_tolerance, so.gradient_tolerance, so.parameter_tolerance, so.max_num_iterations, so.max_linear_solver_iterations) == (0.0, 1.0, 0.0, 50, 100)
    assert many.loss_function_type == many.TRIVIAL and not (many.refine_focal_length or many.refine_principal_point or many.refine_extra_params)
    so = few.solver_options
    assert (so.function_tolerance, so.gradient_tolerance, so.parameter_tolerance, so.max_num_iterations, so.max_linear_solver_iterations) == (0.0, 0.1, 0.0, 100, 200)
    mo = IncrementalMapperOptions()
    assert (mo.ba_global_max_refinements, mo.ba_global_max_refinement_change, mo.filter_max_reproj_error, mo.filter_min_tri_angle) == (5, 0.0005, 4.0, 1.5)


def test_oracle_refinement_loop_terminates_and_removes_planted_outliers(oracle):
    """cfg-1 size, 0.5 px noise, 5 % outliers, float32 lines.  Measured: two rounds; under the TRIVIAL loss of the global preset the planted
    outliers (338 px rms) dominate round 1's solve, so its filter removes them AND most of the inlier observations they dragged along
    (1740 of 2000; a point with one observation over 4 px loses its whole 4-track, reconstruction.cc:689-700); round 2 changes nothing."""
    sc = synthetic.make_ba_scene(20, 500, 4, seed=0xC0FFEE + 1, model=2, **refinement_oracle.NOISY)
    refs = _obs_refs(sc)
    rec = Reconstruction.from_scene(sc)
    options = IncrementalMapperOptions()
    rep = refinement_oracle.iterative_global_refinement(rec, options)
    print("rounds %d, filtered %s, changed %s, iterations %s" % (rep["num_rounds"], rep["num_filtered"], rep["changed"], [s.num_iterations for s in rep["summaries"]]))
    assert 1 <= rep["num_rounds"] <= options.ba_global_max_refinements                                  # it terminates ...
    assert rep["changed"][-1] < options.ba_global_max_refinement_change                                 # ... because a round changed too little, not on the round limit
    assert all(c >= options.ba_global_max_refinement_change for c in rep["changed"][:-1])
    planted = set(refs[o] for o in np.flatnonzero(sc["outlier_mask"]))
    assert len(planted) == 100
    assert len(planted & set(rep["obs_deleted"][0])) >= 0.9 * len(planted)                              # round 1 removes the planted outliers
    left = refinement_oracle.observations(rec)
    assert len(planted & left) <= 0.1 * len(planted)
    assert rep["num_filtered"][0] == len(rep["obs_deleted"][0]) and len(left) == 2000 - sum(len(d) for d in rep["obs_deleted"])
    # what is left is a consistent reconstruction: every remaining point has a track of three or more, every residual is under the threshold
    assert all(len(p.track) >= 3 for p in rec.points3D.values()) and len(left) == sum(len(p.track) for p in rec.points3D.values())
    r = oracle.ba_eval(rec._filter_scene()[0])[0]
    assert np.hypot(r[0::2], r[1::2]).max() <= options.filter_max_reproj_error


def test_gauge_and_filter_bookkeeping_that_both_loops_share():
    """The oracle loop of tests/refinement_oracle.py takes the gauge configuration and the deletion of what a filter reports from the package: checked
    here on their own.  sfm/incremental_mapper.cc:906-926: every image in the problem, the first pose constant, tvec[0] of the second constant, nothing else."""
    sc = synthetic.make_ba_scene(6, 30, 3, seed=9, model=2)
    rec = Reconstruction.from_scene(sc)
    config = GlobalBundleAdjustmentConfig(rec)
    assert sorted(config.Images()) == list(range(6)) and config.NumConstantPoses() == 1 and config.HasConstantPose(0)
    assert config.NumConstantTvecs() == 1 and config.ConstantTvec(1) == [0] and config.NumPoints() == 0 and config.NumConstantCameras() == 0
    scene, pose_index, point_index, cam_index = BundleAdjuster(GlobalBundleAdjustmentOptions(6), config).flatten(rec)
    assert [pose_index[i] for i in range(6)] == list(range(6))
    assert list(scene["pose_const"]) == [1, 0, 0, 0, 0, 0] and list(scene["tvec_const_mask"]) == [0, 1, 0, 0, 0, 0]
    assert not scene["point_const"].any() and list(scene["camera_const_mask"]) == [0xFFFF] and scene["loss_type"] == 0
    assert len(scene["obs_pose"]) == 90 and len(point_index) == 30
    # deleting what a filter reports: observation 4 (of point 1) and point 2 with its whole track
    fscene, aligned, cam_size, point_ids, obs_ref = rec._filter_scene()
    assert np.array_equal(fscene["obs_point"], np.repeat(np.arange(30), 3)) and point_ids == list(range(30))
    od = np.zeros(90, dtype=bool); pd = np.zeros(30, dtype=bool); pe = np.full(30, -1.0)
    od[4] = True; od[6:9] = True; pd[2] = True; pe[1] = 0.5
    before = refinement_oracle.observations(rec)
    rec._apply_points_filter(fscene, point_ids, obs_ref, od, pd, pe)
    gone = before - refinement_oracle.observations(rec)
    assert gone == set(obs_ref[o] for o in (4, 6, 7, 8))
    assert 2 not in rec.points3D and len(rec.points3D) == 29 and len(rec.points3D[1].track) == 2 and obs_ref[4] not in rec.points3D[1].track
    assert rec.points3D[1].error == 0.5 and rec.ComputeNumObservations() == 86
    assert all(not rec.images[i].lines[k].HasPoint3D() for (i, k) in gone)
