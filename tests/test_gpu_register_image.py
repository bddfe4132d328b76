"""pp_tracks_find_next_images / pp_tracks_estimate_image_pose / pp_tracks_register_image (K13) on the device against the plain-Python transcription
(tests/register_image_reference.py) on the scenes of tests/register_image_scenes.py.

Everything here is EXACT.  The search, the counts, the ranking and the commit are integer decisions.  The pose is BITWISE equal to the existing
EstimateAbsolutePoseFromLines (privacy_preserving_sfm_amd.estimators: pp_pose_create + pp_pose_ransac) called on the arrays the transcription builds
on the host: the same kernels on the same numbers in the same order, so no tolerance is needed or allowed.

One scene per `failure` code - except PP_REG_NAN, which no input reaches: every entry of a model enters every residual (each of the three rows is
used), so a model with a NaN entry has no inlier and the pose.cc:65 site (PP_REG_NO_INLIERS) is taken before pose.cc:89; the conversion to a quaternion
takes square roots of 1 + trace resp. 1 + 2 R_ii - trace >= 1 - trace / 3 > 0 only.  That gate is exercised on the host (tests/test_register_replay_host.py)."""
import ctypes as C

import numpy as np
import pytest

import mixed_models as mm
import register_image_reference as ref
import register_image_scenes as scenes
from privacy_preserving_sfm_amd import _capi, estimators
from privacy_preserving_sfm_amd.bundle_adjustment import Camera
from privacy_preserving_sfm_amd.device import TracksProblem, local_bundle_options, next_image_options, ransac_options, tracks_image_options
from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator

pytestmark = pytest.mark.gpu

ONE_TRIAL = dict(max_error=0.012, min_inlier_ratio=0.25, confidence=0.99999, min_num_trials=0, max_num_trials=1)      # the search scenes have no geometry
MAPPER_RANSAC = dict(min_inlier_ratio=0.25, confidence=0.99999, min_num_trials=100, max_num_trials=10000)              # :673-681


def _flatten(rec, graph):
    flat, point_ids, line_ref = IncrementalTriangulator(graph, rec).flatten()
    assert sorted(rec.images) == list(range(len(rec.images))) and point_ids == list(range(len(point_ids)))      # id = index in these scenes
    return flat, line_ref


def _same_state(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("line_point", "points", "deleted", "track_start", "track_line"))


def _threshold(camera, px):
    out = C.c_double()
    _capi.check(_capi.lib().pp_camera_image_to_world_threshold(camera.model_id, _capi.dp(_capi.f64(camera.params)), float(px), C.cast(C.byref(out), _capi.c_dp)))
    return out.value


def _corrs_as_ids(corrs, line_ref, image):
    assert all(line_ref[l][0] == image for l in corrs[:, 0])
    return [(line_ref[l][1], int(p)) for l, p in corrs]


@pytest.mark.parametrize("scene", scenes.SEARCH_SCENES, ids=lambda f: f.__name__)
def test_search_counts_and_ranking(scene):
    w, wants = scene()
    flat, line_ref = _flatten(w.rec, w.graph)
    m = ref.Mapper(w.rec, w.graph)
    pb = TracksProblem(flat)
    try:
        before = pb.state()
        o = next_image_options(abs_pose_min_num_inliers=1)
        for want in wants:
            q = want["image"]
            out = [pb.estimate_image_pose(q, ransac_options(seed=0, **ONE_TRIAL), o) for _ in range(2)]
            rep, pose, corrs, mask = out[0]
            assert _corrs_as_ids(corrs, line_ref, q) == want["tri_corrs"] == m.search(ref.Options(), q)[0]
            assert (rep.num_visible, rep.num_corrs) == (want["visible"], len(want["tri_corrs"]))
            if len(want["tri_corrs"]) < 6:
                assert rep.failure == (_capi.REG_FEW_CORRS if want["visible"] else _capi.REG_FEW_VISIBLE)
            rep2, pose2, corrs2, mask2 = out[1]      # a second call returns the same
            assert np.array_equal(corrs, corrs2) and np.array_equal(pose, pose2) and np.array_equal(mask, mask2) and rep.failure == rep2.failure
        for method in (0, 1):
            rep, ranked, vis, obs = pb.find_next_images(next_image_options(abs_pose_min_num_inliers=1, image_selection_method=method))
            for iid in sorted(w.rec.images):      # every image, registered or not
                assert vis[iid] == ref.num_visible_points3D(w.rec, w.graph, w.rec.images[iid]), iid
                assert obs[iid] == ref.num_observations(w.graph, w.rec.images[iid]), iid
            assert ranked.tolist() == m.find_next_images(ref.Options(abs_pose_min_num_inliers=1, image_selection_method=method))
            assert rep.num_ranked == rep.num_first_bucket == len(ranked)
        for want in wants:
            assert vis[want["image"]] == want["visible"] and obs[want["image"]] == want["observed"]
        assert _same_state(before, pb.state())
    finally:
        pb.close()


def test_the_visibility_gate_comes_before_the_search():
    w, (want,) = scenes.visible_but_unusable()
    flat, line_ref = _flatten(w.rec, w.graph)
    pb = TracksProblem(flat)
    try:
        rep, _, corrs, _ = pb.estimate_image_pose(want["image"], ransac_options(seed=0, **ONE_TRIAL), next_image_options(abs_pose_min_num_inliers=9))
        assert (rep.failure, rep.num_visible, rep.num_corrs, len(corrs)) == (_capi.REG_FEW_VISIBLE, 8, 0, 0)
        rep, _, corrs, _ = pb.estimate_image_pose(want["image"], ransac_options(seed=0, **ONE_TRIAL), next_image_options(abs_pose_min_num_inliers=8))
        assert (rep.failure, rep.num_visible, rep.num_corrs) == (_capi.REG_FEW_CORRS, 8, 0)      # (e): visible, and nothing usable
    finally:
        pb.close()


def test_ranking_scene():
    w, want = scenes.ranking()
    flat, _ = _flatten(w.rec, w.graph)
    Cn = len(w.rec.images)
    trials, filtered = np.zeros(Cn, dtype=np.int32), np.zeros(Cn, dtype=np.uint8)
    for k, v in want["num_reg_trials"].items():
        trials[k] = v
    filtered[want["filtered"]] = 1
    m = ref.Mapper(w.rec, w.graph)
    m.num_reg_trials, m.filtered_images = dict(want["num_reg_trials"]), set(want["filtered"])
    pb = TracksProblem(flat)
    try:
        for method, key in ((0, "num"), (1, "ratio")):
            rep, ranked, vis, obs = pb.find_next_images(next_image_options(image_selection_method=method, **want["options"]), trials, filtered)
            assert ranked.tolist() == want[key] == m.find_next_images(ref.Options(image_selection_method=method, **want["options"]))
            assert (rep.num_ranked, rep.num_first_bucket, rep.num_unregistered) == (6, 4, 9)
            for q in want["visible"]:
                assert (vis[q], obs[q]) == (want["visible"][q], want["observed"][q])
        rep, ranked, _, _ = pb.find_next_images(next_image_options(image_selection_method=1, **want["options"]))      # no trials, nothing filtered
        assert ranked.tolist() == ref.Mapper(w.rec, w.graph).find_next_images(ref.Options(image_selection_method=1, **want["options"]))
        with pytest.raises(_capi.PPError) as e:
            pb.find_next_images(next_image_options(abs_pose_min_num_inliers=0))
        assert e.value.code == _capi.PP_ERR_INVALID
        bad = trials.copy(); bad[4] = -1
        with pytest.raises(_capi.PPError) as e:
            pb.find_next_images(next_image_options(), bad)
        assert e.value.code == _capi.PP_ERR_INVALID
    finally:
        pb.close()


def _pose_case(world_kw, options_kw, relabel=None):
    """-> (rec, graph, info, flat, line_ref, mapper, what the existing estimator gives on the transcription's arrays)"""
    rec, graph, info = scenes.pose_world(**world_kw)
    if relabel is not None:
        flat0, _ = _flatten(rec, graph)
        mixed = mm.mix_camera_models(dict(flat0, camera_const_mask=np.zeros(flat0["intr"].shape[0], dtype=np.uint16)), relabel)
        for k in sorted(rec.cameras):
            model = int(mixed["camera_model"][k])
            rec.cameras[k] = Camera(k, model, mixed["intr"][k, : _capi.lib().pp_camera_num_params(model)], width=1280, height=960)
    flat, line_ref = _flatten(rec, graph)
    return rec, graph, info, flat, line_ref


def _existing_estimator(rec, m, options, image):
    """the transcription's arrays through the existing RANSAC mirror -> (site, pose7 or None, report)"""
    tri_corrs, tri_lines2D, tri_points3D = m.search(options, image)
    o = estimators.RANSACOptions()
    o.max_error = _threshold(rec.cameras[rec.images[image].camera_id], options.abs_pose_max_error)
    o.min_inlier_ratio, o.confidence, o.min_num_trials, o.max_num_trials = 0.25, 0.99999, 100, 10000
    report = estimators.RANSAC(o, seed=0).Estimate(tri_lines2D, tri_points3D)
    mask = report.inlier_mask if report.success else np.zeros(len(tri_corrs), dtype=np.uint8)
    site, q, t, n, _ = ref.estimate_absolute_pose_from_lines(lambda *a: (report.support.num_inliers, mask, report.model), o, tri_lines2D, tri_points3D)
    if site == ref.OK and n < options.abs_pose_min_num_inliers:
        site = ref.FEW_INLIERS
    pose = None if q is None else np.concatenate([q, t])
    return site, pose, report, mask, tri_corrs, o.max_error


@pytest.mark.parametrize("name", sorted(scenes.POSE_SCENES) + ["mixed_models"])
def test_pose_is_bitwise_the_existing_estimator(name):
    relabel = None
    if name == "mixed_models":
        world_kw, options_kw, planted, relabel = dict(n=50, outliers=10, aligned=5, seed=11), dict(abs_pose_min_num_inliers=30), 0, (1, 2, 4)
    else:
        world_kw, options_kw, planted = scenes.POSE_SCENES[name]
    rec, graph, info, flat, line_ref = _pose_case(world_kw, options_kw, relabel)
    if relabel is not None:
        assert sorted(set(flat["camera_model"].tolist())) == [1, 2, 4]
    image = info["image"]
    options = ref.Options(**options_kw)
    m = ref.Mapper(rec, graph)
    pb = TracksProblem(flat)
    try:
        before = pb.state()
        max_error = _threshold(rec.cameras[rec.images[image].camera_id], options.abs_pose_max_error)
        rep, pose, corrs, mask = pb.estimate_image_pose(image, ransac_options(max_error=max_error, seed=0, **MAPPER_RANSAC),
                                                        next_image_options(**options_kw), flat["line_aligned"])
        assert _same_state(before, pb.state())
    finally:
        pb.close()
    print("%s: failure %d visible %d corrs %d trials %d inliers %d aligned inliers %d, device %.3f ms replay %.3f ms total %.3f ms" %
          (name, rep.failure, rep.num_visible, rep.num_corrs, rep.num_trials, rep.num_inliers, rep.num_aligned_inliers, rep.device_ms, rep.replay_ms, rep.total_ms))
    assert rep.failure == planted
    assert rep.num_visible == ref.num_visible_points3D(rec, graph, rec.images[image])
    if planted == ref.FEW_VISIBLE:
        assert rep.num_corrs == 0 and not mask.any()
        return
    site, want_pose, report, want_mask, tri_corrs, want_error = _existing_estimator(rec, m, options, image)
    assert want_error == max_error
    assert _corrs_as_ids(corrs, line_ref, image) == tri_corrs
    if planted == ref.FEW_CORRS:
        assert not mask.any() and rep.num_trials == 0
        return
    assert site == planted
    assert (rep.num_trials, rep.num_inliers) == (report.num_trials, report.support.num_inliers)
    assert np.array_equal(mask, want_mask)
    assert rep.num_aligned_inliers == int(sum(1 for i, (idx, _) in enumerate(tri_corrs) if mask[i] and rec.images[image].lines[idx].IsAligned()))
    if want_pose is not None:
        assert np.array_equal(pose, want_pose)      # the same doubles
    if planted == 0:
        assert np.array_equal(mask.astype(bool), info["inliers"])      # exactly the planted inliers
        err = min(np.abs(pose - info["pose"]).max(), np.abs(pose * np.array([-1] * 4 + [1] * 3) - info["pose"]).max())
        print("  distance from the true pose %.3e" % err)
    if planted == ref.NO_INLIERS:
        assert rep.num_inliers == 0 and not mask.any()


def _register_on_both(rec, graph, image, pose, tri_corrs, mask, flat, line_ref):
    """the device commit on a handle over `flat`, the transcription's commit on `rec` -> (events of both, handle, fresh handle over the updated rec)"""
    rows = np.array([(line_ref.index((image, idx)), pid) for idx, pid in tri_corrs], dtype=np.int32).reshape(-1, 2)
    pb = TracksProblem(flat)
    events = pb.register_image(image, pose, rows, mask)
    m = ref.Mapper(rec, graph)
    rec.images[image].qvec, rec.images[image].tvec = np.array(pose[:4]), np.array(pose[4:])
    want_events = m.commit(image, tri_corrs, list(mask))
    fresh_flat, fresh_ref = _flatten(rec, graph)
    assert fresh_ref == line_ref
    return [(int(p), line_ref[int(l)]) for p, l in events], want_events, pb, TracksProblem(fresh_flat), fresh_flat


@pytest.mark.parametrize("scene", scenes.COMMIT_SCENES, ids=lambda f: f.__name__)
def test_commit_rule(scene):
    w, want = scene()
    flat, line_ref = _flatten(w.rec, w.graph)
    pose = scenes.QUERY_POSE.copy()
    got, want_events, pb, pf, fresh_flat = _register_on_both(w.rec, w.graph, want["image"], pose, want["tri_corrs"], want["inlier_mask"], flat, line_ref)
    try:
        assert got == want_events == want["events"]
        assert _same_state(pb.state(), pf.state())
        assert fresh_flat["image_registered"][want["image"]] == 1
        a, b = pb.find_next_images(next_image_options(abs_pose_min_num_inliers=1)), pf.find_next_images(next_image_options(abs_pose_min_num_inliers=1))
        assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])) and want["image"] not in a[1].tolist()
    finally:
        pb.close(); pf.close()


def test_register_equals_a_fresh_handle_for_the_later_calls():
    """found_50 with its planted inliers: after the commit, TriangulateImage and FindLocalBundle of the new image give the same on the handle and on a
    handle created from the transcription's updated reconstruction - the pose, the projection matrix, the centre and image_registered all arrived"""
    world_kw, options_kw, _ = scenes.POSE_SCENES["found_50"]
    rec, graph, info = scenes.pose_world(**world_kw)
    # a few FREE lines in the registered images that correspond to lines of the new image: work for TriangulateImage
    flat, line_ref = _flatten(rec, graph)
    image = info["image"]
    tri_corrs = ref.Mapper(rec, graph).search(ref.Options(**options_kw), image)[0]
    mask = info["inliers"].astype(np.uint8)
    got, want_events, pb, pf, fresh_flat = _register_on_both(rec, graph, image, info["pose"], tri_corrs, mask, flat, line_ref)
    try:
        assert got == want_events and len(got) == int(mask.sum())
        assert _same_state(pb.state(), pf.state())
        lb = [p.find_local_bundle(image, local_bundle_options(local_ba_num_images=3)) for p in (pb, pf)]
        assert np.array_equal(lb[0][1], lb[1][1]) and len(lb[0][1]) == 2 and all(np.array_equal(lb[0][2][k], lb[1][2][k]) for k in ("image", "count", "tri_angle"))
        assert lb[0][0].num_points3D == int(mask.sum())
        tri = [p.triangulate_image(image, tracks_image_options(), fresh_flat["line_aligned"]) for p in (pb, pf)]
        assert np.array_equal(tri[0][1], tri[1][1]) and tri[0][0].num_changed == tri[1][0].num_changed
        assert _same_state(pb.state(), pf.state())
        with pytest.raises(_capi.PPError) as e:      # registered now: the reference CHECKs it
            pb.estimate_image_pose(image, ransac_options(seed=0, **ONE_TRIAL), next_image_options())
        assert e.value.code == _capi.PP_ERR_INVALID
    finally:
        pb.close(); pf.close()


def test_invalid_arguments_leave_the_handle_as_it_was():
    w, want = scenes.commit_two_lines_one_point()
    w.rec.points3D[len(w.rec.points3D)] = type(w.rec.points3D[0])(np.array([0.0, 0.0, 5.0]))      # a point without a track: deleted
    flat, line_ref = _flatten(w.rec, w.graph)
    q, dead = want["image"], len(flat["points"]) - 1
    L, P, Cn = len(line_ref), len(flat["points"]), len(w.rec.images)
    good = np.array([(line_ref.index((q, idx)), pid) for idx, pid in want["tri_corrs"]], dtype=np.int32)
    other = line_ref.index((scenes.HOST_A, 0))
    pose = scenes.QUERY_POSE.copy()
    nan_pose, inf_pose = pose.copy(), pose.copy()
    nan_pose[5], inf_pose[0] = np.nan, np.inf
    r = ransac_options(seed=0, **ONE_TRIAL)
    pb = TracksProblem(flat)
    try:
        assert pb.state()["deleted"][dead] == 1
        state, ranked = pb.state(), pb.find_next_images(next_image_options(abs_pose_min_num_inliers=1))
        calls = [lambda: pb.register_image(Cn, pose, good), lambda: pb.register_image(-1, pose, good),
                 lambda: pb.register_image(scenes.HOST_A, pose, np.zeros((0, 2))),      # registered already
                 lambda: pb.register_image(q, pose, np.concatenate([good, [[other, 0]]])),      # a line of another image
                 lambda: pb.register_image(q, pose, [[L, 0]]), lambda: pb.register_image(q, pose, [[-1, 0]]),
                 lambda: pb.register_image(q, pose, [[good[0, 0], P]]), lambda: pb.register_image(q, pose, [[good[0, 0], -1]]),
                 lambda: pb.register_image(q, pose, [[good[0, 0], dead]], [0]),      # a deleted point, even where the mask drops it
                 lambda: pb.register_image(q, nan_pose, good), lambda: pb.register_image(q, inf_pose, good),
                 lambda: pb.estimate_image_pose(Cn, r), lambda: pb.estimate_image_pose(-1, r), lambda: pb.estimate_image_pose(scenes.HOST_A, r),
                 lambda: pb.estimate_image_pose(q, r, next_image_options(abs_pose_min_num_inliers=0)),
                 lambda: pb.estimate_image_pose(q, ransac_options(seed=0, **dict(ONE_TRIAL, max_error=0.0)))]
        for k, call in enumerate(calls):
            with pytest.raises(_capi.PPError) as e:
                call()
            assert e.value.code == _capi.PP_ERR_INVALID, k
            again = pb.find_next_images(next_image_options(abs_pose_min_num_inliers=1))
            assert _same_state(state, pb.state()) and all(np.array_equal(x, y) for x, y in zip(ranked[1:], again[1:])), k
        events = pb.register_image(q, pose, good, want["inlier_mask"])      # and the handle still works
        assert [(int(p), line_ref[int(l)]) for p, l in events] == want["events"]
    finally:
        pb.close()
