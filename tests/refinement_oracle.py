"""The mapper's global refinement loop with the CPU ORACLE doing the arithmetic - TEST INFRASTRUCTURE (shared by
tests/test_oracle_global_refinement.py and tests/test_gpu_global_refinement.py).

The loop's logic is restated here step by step (reference src/controllers/incremental_mapper.cc:52-70, 102-124 and
src/sfm/incremental_mapper.cc:893-939) on the package's host data model: the bookkeeping (which observations exist, which blocks
are constant, deleting what a filter reports, Normalize) is the package's host code, every number comes from oracle_lib
(`ba_solve`, `filter_negative_depth`, `filter_points3d`).  The device never runs here.
"""
import numpy as np

import oracle_lib
from privacy_preserving_sfm_amd.bundle_adjustment import (BundleAdjuster, GlobalBundleAdjustmentConfig, GlobalBundleAdjustmentOptions,
                                                          IncrementalMapperOptions)

NOISY = dict(line_noise_px=0.5, outlier_obs=0.05, quantise_float32=True)      # the observation model of every noisy scene of the suite


def oracle_options(solver_options, **kw):
    so = solver_options
    return oracle_lib.BAOptionsC.defaults(max_num_iterations=so.max_num_iterations, function_tolerance=so.function_tolerance,
                                          gradient_tolerance=so.gradient_tolerance, parameter_tolerance=so.parameter_tolerance,
                                          max_num_consecutive_invalid_steps=so.max_num_consecutive_invalid_steps,
                                          max_linear_solver_iterations=so.max_linear_solver_iterations, **kw)


def observations(rec):
    return set((iid, idx) for iid, image in rec.images.items() for idx, line in enumerate(image.lines) if line.HasPoint3D())


def adjust_global_bundle(rec, ba_options):
    """AdjustGlobalBundle: -> (success, oracle summary or None, trace or None)"""
    scene, aligned, cam_size, point_ids, obs_ref = rec._filter_scene()
    _, neg = oracle_lib.filter_negative_depth(scene)
    for o, (iid, idx) in enumerate(obs_ref):
        if neg[o]:
            rec.DeleteObservation(iid, idx)
    flat = BundleAdjuster(ba_options, GlobalBundleAdjustmentConfig(rec)).flatten(rec)
    if flat is None:
        return False, None, None
    poses, points, intr, summary, trace = oracle_lib.ba_solve(flat[0], oracle_options(ba_options.solver_options))
    if summary.termination not in (2, 4):            # FAILURE / USER_FAILURE: nothing is written back
        BundleAdjuster.write_back(rec, flat, poses, points, intr)
    rec.Normalize()
    return True, summary, trace


def filter_all_points(rec, max_reproj_error, min_tri_angle):
    """FilterAllPoints3D: -> (num_filtered, smallest relative distance of an observation's pixel error from max_reproj_error)"""
    scene, aligned, cam_size, point_ids, obs_ref = rec._filter_scene()
    r = oracle_lib.ba_eval(scene)[0].reshape(-1, 2)
    margin = float(np.abs(np.hypot(r[:, 0], r[:, 1]) - max_reproj_error).min() / max_reproj_error)
    nf, od, pd, pe = oracle_lib.filter_points3d(scene, max_reproj_error, min_tri_angle, cam_size, aligned)
    rec._apply_points_filter(scene, point_ids, obs_ref, od, pd, pe)
    return nf, margin


def iterative_global_refinement(rec, mapper_options=None):
    """IterativeGlobalRefinement without CompleteAndMergeTracks / FilterImages: dict(num_rounds, summaries, traces, num_filtered, changed,
    obs_deleted, point_deleted (sorted lists per round), margin (the smallest threshold margin over the rounds))"""
    options = mapper_options or IncrementalMapperOptions()
    rep = dict(num_rounds=0, summaries=[], traces=[], num_filtered=[], changed=[], obs_deleted=[], point_deleted=[], margin=np.inf)
    for _ in range(options.ba_global_max_refinements):
        num_observations = rec.ComputeNumObservations()
        _, summary, trace = adjust_global_bundle(rec, GlobalBundleAdjustmentOptions(len(rec.RegImageIds()), options))
        obs_before, points_before = observations(rec), set(rec.points3D)
        nf, margin = filter_all_points(rec, options.filter_max_reproj_error, options.filter_min_tri_angle)
        changed = float(nf) / num_observations
        rep["num_rounds"] += 1
        rep["summaries"].append(summary); rep["traces"].append(trace)
        rep["num_filtered"].append(nf); rep["changed"].append(changed)
        rep["obs_deleted"].append(sorted(obs_before - observations(rec)))
        rep["point_deleted"].append(sorted(points_before - set(rec.points3D)))
        rep["margin"] = min(rep["margin"], margin)
        if changed < options.ba_global_max_refinement_change:
            break
    return rep


def parameters(rec):
    """(poses [C,7], points [P,3], point ids) in id order"""
    image_ids, point_ids = sorted(rec.images), sorted(rec.points3D)
    poses = np.array([np.concatenate([rec.images[i].qvec, rec.images[i].tvec]) for i in image_ids])
    points = np.array([rec.points3D[p].xyz for p in point_ids])
    return poses, points, point_ids
