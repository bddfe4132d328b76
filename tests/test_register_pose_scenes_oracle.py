"""The pose scenes of tests/register_image_scenes.py through the ORACLE alone (oracle/absolute_pose.h, the CPU restatement of RANSAC<P6LEstimator>), so
that the GPU tests never rest on an input the reference's own estimator fails on: on every `found` scene it finds a pose whose inliers are exactly the
planted ones, close to the true pose, and on every failure scene the transcription of RegisterNextImage takes exactly the planted `return false`.
No device runs here."""
import numpy as np
import pytest

import register_image_reference as ref
import register_image_scenes as scenes


def _oracle_estimate(oracle, seen):
    def ransac(options, lines2D, points3D):
        lines = np.array([l.Line() for l in lines2D]).reshape(-1, 3)
        aligned = np.array([l.IsAligned() for l in lines2D], dtype=np.uint8)
        rep, mask = oracle.p6l_ransac(lines, np.array(points3D).reshape(-1, 3), aligned, options.max_error, seed=0, min_inlier_ratio=options.min_inlier_ratio,
                                      confidence=options.confidence, mult=options.dyn_num_trials_multiplier, min_num_trials=options.min_num_trials,
                                      max_num_trials=options.max_num_trials)
        seen.update(num_trials=int(rep.num_trials), num_inliers=int(rep.num_inliers), mask=mask.copy())
        return int(rep.num_inliers), (mask if rep.success else np.zeros(len(lines2D), dtype=np.uint8)), np.array(rep.model).reshape(3, 4)
    return lambda o, l, X: ref.estimate_absolute_pose_from_lines(ransac, o, l, X)


@pytest.mark.parametrize("name", sorted(scenes.POSE_SCENES))
def test_the_oracle_hits_what_is_planted(oracle, name):
    world_kw, options_kw, planted = scenes.POSE_SCENES[name]
    rec, graph, info = scenes.pose_world(**world_kw)
    m, seen = ref.Mapper(rec, graph), {}
    ok = m.register_next_image(ref.Options(**options_kw), info["image"], _oracle_estimate(oracle, seen), lambda *a: True, lambda camera, px: px / camera.params[0])
    print(name, m.last["failure"], seen.get("num_trials"), seen.get("num_inliers"))
    assert m.last["failure"] == planted and ok == (planted == 0)
    if planted == 0:
        assert np.array_equal(np.asarray(m.last["inlier_mask"]).astype(bool), info["inliers"])
        pose = m.last["estimated_pose"]
        err = min(np.abs(pose - info["pose"]).max(), np.abs(pose * np.array([-1] * 4 + [1] * 3) - info["pose"]).max())
        assert err < 1e-8, err      # exact lines: the minimal solver's own rounding
        assert ref.is_registered(rec.images[info["image"]]) and len(m.last["events"]) == int(info["inliers"].sum())
    if planted == ref.NO_INLIERS:
        assert seen["num_inliers"] == 0
    if planted == ref.FEW_INLIERS:
        assert seen["num_inliers"] == int(info["inliers"].sum()) == 20
    if planted == ref.ALIGNED:
        assert seen["num_inliers"] == 50
