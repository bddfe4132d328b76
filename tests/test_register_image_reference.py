"""The transcription of FindNextImages / RegisterNextImage (tests/register_image_reference.py) against the expectations the scenes of
tests/register_image_scenes.py carry, all worked out by hand from the reference's text: the 2D-3D search with its per-line set of seen points and
its three filters, NumVisiblePoints3D / NumObservations, the two rank functions with the buckets and the tie rule, the gates in order, the commit
rule.  The pose estimator is a canned RANSAC report here; no device runs."""
import numpy as np
import pytest

import register_image_reference as ref
import register_image_scenes as scenes


@pytest.mark.parametrize("scene", scenes.SEARCH_SCENES, ids=lambda f: f.__name__)
def test_search_and_counts(scene):
    w, wants = scene()
    m = ref.Mapper(w.rec, w.graph)
    for want in wants:
        image = w.rec.images[want["image"]]
        tri_corrs, tri_lines2D, tri_points3D = m.search(ref.Options(), want["image"])
        assert tri_corrs == want["tri_corrs"]
        assert len(tri_lines2D) == len(tri_points3D) == len(tri_corrs)
        for (line_idx, pid), l, X in zip(tri_corrs, tri_lines2D, tri_points3D):
            assert l is image.lines[line_idx] and np.array_equal(X, w.rec.points3D[pid].xyz)
        assert ref.num_visible_points3D(w.rec, w.graph, image) == want["visible"]
        assert ref.num_observations(w.graph, image) == want["observed"]


def test_long_lists_hold_what_the_docstrings_say():
    w, (want,) = scenes.dedup_across_chunks()
    assert len(w.graph.FindCorrespondences(want["image"], 0)) == 72 and len(want["tri_corrs"]) == 70
    w, (want,) = scenes.list_lengths()
    lengths = [len(w.graph.FindCorrespondences(want["image"], i)) for i in range(8)]
    assert lengths == [0, 1, 64, 65, 130, 256, 257, 300]
    per_line = [sum(1 for c in want["tri_corrs"] if c[0] == i) for i in range(8)]
    assert per_line == [0, 1, 64, 65, 130, 256, 257, 298]


@pytest.mark.parametrize("scene", scenes.COMMIT_SCENES, ids=lambda f: f.__name__)
def test_commit_rule(scene):
    w, want = scene()
    m = ref.Mapper(w.rec, w.graph)
    assert m.search(ref.Options(), want["image"])[0] == want["tri_corrs"]
    events = m.commit(want["image"], want["tri_corrs"], want["inlier_mask"])
    assert events == want["events"]
    assert w.rec.images[want["image"]].registered is True
    for pid, (iid, idx) in events:
        assert w.rec.images[iid].lines[idx].Point3DId() == pid and (iid, idx) in w.rec.points3D[pid].track
    free = [idx for idx, l in enumerate(w.rec.images[want["image"]].lines) if not l.HasPoint3D()]
    assert free == [idx for idx in range(len(w.rec.images[want["image"]].lines)) if idx not in [e[1][1] for e in events]]
    assert m.modified_point3D_ids == [e[0] for e in events]
    assert m.num_reg_images_per_camera[0] == 3      # the two registered hosts of camera 0 and the new image


def test_ranking_buckets_and_ties():
    w, want = scenes.ranking()
    m = ref.Mapper(w.rec, w.graph)
    m.num_reg_trials = dict(want["num_reg_trials"])
    m.filtered_images = set(want["filtered"])
    for q in want["visible"]:
        assert ref.num_visible_points3D(w.rec, w.graph, w.rec.images[q]) == want["visible"][q]
        assert ref.num_observations(w.graph, w.rec.images[q]) == want["observed"][q]
    assert m.find_next_images(ref.Options(image_selection_method=ref.MAX_VISIBLE_POINTS_NUM, **want["options"])) == want["num"]
    assert m.find_next_images(ref.Options(image_selection_method=ref.MAX_VISIBLE_POINTS_RATIO, **want["options"])) == want["ratio"]
    # one more trial for image 11 and it is out; a trial for image 5 moves it to the second bucket
    m.num_reg_trials[11] = 3
    m.num_reg_trials[5] = 1
    assert m.find_next_images(ref.Options(image_selection_method=ref.MAX_VISIBLE_POINTS_RATIO, **want["options"])) == [7, 4, 6, 5, 9]


def _canned(num_inliers, mask, model):
    return lambda options, lines2D, points3D: (num_inliers, mask, model)


def _pose_model():
    from privacy_preserving_sfm_amd import synthetic
    pose = scenes.QUERY_POSE.copy()
    pose[:4] /= np.linalg.norm(pose[:4])
    return pose, np.concatenate([synthetic.quat_to_rot(pose[:4]), pose[4:, None]], axis=1)


def test_gates_in_the_reference_order():
    """every `return false` site with a canned estimator, and the trial count incremented before the first gate"""
    pose, model = _pose_model()
    threshold = lambda camera, px: px / camera.params[0]
    refine_ok = lambda *a: True

    def run(world_kw, options_kw, ransac, refine=refine_ok):
        rec, graph, info = scenes.pose_world(**world_kw)
        m = ref.Mapper(rec, graph)
        estimate = lambda o, l, X: ref.estimate_absolute_pose_from_lines(ransac(len(l)), o, l, X)
        ok = m.register_next_image(ref.Options(**options_kw), info["image"], estimate, refine, threshold)
        assert m.num_reg_trials == {info["image"]: 1}
        return ok, m, rec, info

    all_in = lambda n: _canned(n, [1] * n, model)
    ok, m, rec, info = run(dict(n=20, outliers=0, seed=4), dict(abs_pose_min_num_inliers=21), all_in)
    assert not ok and m.last["failure"] == ref.FEW_VISIBLE and m.last["tri_corrs"] == []
    ok, m, rec, info = run(dict(n=20, outliers=0, extra_unusable=10, seed=5), dict(abs_pose_min_num_inliers=25), all_in)
    assert not ok and m.last["failure"] == ref.FEW_CORRS and m.last["num_visible"] == 30 and len(m.last["tri_corrs"]) == 20
    ok, m, rec, info = run(dict(n=5, outliers=0, seed=5), dict(abs_pose_min_num_inliers=4), all_in)
    assert not ok and m.last["failure"] == ref.FEW_CORRS      # five correspondences pass the option and fail the `< 6`
    ok, m, rec, info = run(dict(n=40, seed=6), dict(abs_pose_min_num_inliers=10), lambda n: _canned(0, [], model))
    assert not ok and m.last["failure"] == ref.NO_INLIERS
    # 50 inliers, 46 aligned: 46 > 45.0; with 45 aligned 45 > 45.0 is false and the image registers
    ok, m, rec, info = run(dict(n=50, outliers=0, aligned=46, seed=7), dict(abs_pose_min_num_inliers=30), all_in)
    assert not ok and m.last["failure"] == ref.ALIGNED
    ok, m, rec, info = run(dict(n=50, outliers=0, aligned=45, seed=7), dict(abs_pose_min_num_inliers=30), all_in)
    assert ok and m.last["failure"] == ref.OK
    nan_model = model.copy(); nan_model[1, 3] = np.nan
    ok, m, rec, info = run(dict(n=40, seed=6), dict(abs_pose_min_num_inliers=10), lambda n: _canned(n, [1] * n, nan_model))
    assert not ok and m.last["failure"] == ref.NAN
    ok, m, rec, info = run(dict(n=50, outliers=30, seed=8), dict(abs_pose_min_num_inliers=30), lambda n: _canned(20, [1] * 20 + [0] * (n - 20), model))
    assert not ok and m.last["failure"] == ref.FEW_INLIERS
    assert np.allclose(rec.images[info["image"]].qvec, pose[:4]) and not ref.is_registered(rec.images[info["image"]])      # the pose is written before :725
    ok, m, rec, info = run(dict(n=50, outliers=10, seed=1), dict(abs_pose_min_num_inliers=30), all_in, refine=lambda *a: False)
    assert not ok and m.last["failure"] == ref.REFINEMENT and not ref.is_registered(rec.images[info["image"]])


def test_success_commits_and_sets_the_ransac_options():
    pose, model = _pose_model()
    rec, graph, info = scenes.pose_world(n=50, outliers=10, seed=1)
    m = ref.Mapper(rec, graph)
    mask = info["inliers"].astype(int).tolist()
    estimate = lambda o, l, X: ref.estimate_absolute_pose_from_lines(_canned(40, mask, model), o, l, X)
    assert m.register_next_image(ref.Options(), 3, estimate, lambda *a: True, lambda camera, px: px / camera.params[0])
    o = m.last["ransac_options"]
    assert (o.max_error, o.min_inlier_ratio, o.min_num_trials, o.max_num_trials, o.confidence) == (12.0 / 1000.0, 0.25, 100, 10000, 0.99999)
    assert ref.is_registered(rec.images[3]) and np.allclose(np.concatenate([rec.images[3].qvec, rec.images[3].tvec]), pose, atol=1e-15)
    assert m.last["events"] == [(i, (3, i)) for i in range(50) if mask[i]]
    assert m.num_reg_images_per_camera == {0: 2, 1: 1, 2: 1}


def test_rotation_matrix_to_quaternion_both_branches():
    from privacy_preserving_sfm_amd import synthetic
    from privacy_preserving_sfm_amd.estimators import RotationMatrixToQuaternion
    rng = np.random.default_rng(0)
    for _ in range(50):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        R = synthetic.quat_to_rot(q)
        got = ref.rotation_matrix_to_quaternion(R)
        assert np.array_equal(got, RotationMatrixToQuaternion(R))
        assert min(np.abs(got - q).max(), np.abs(got + q).max()) < 1e-14
