"""The scene of tests/test_gpu_incremental_registration.py through the ORACLES alone, so that the GPU test never rests on an input the reference's own
estimators fail on: the controller's loop (FindNextImages, RegisterNextImage on the candidates in order until one registers, TriangulateImage) with
the transcription (tests/register_image_reference.py), the CPU RANSAC of oracle/absolute_pose.h and the sequential TriangulateImage of
tests/tracks_image_reference.py; the refinements are left out (the lines are exact: they have nothing to move).  It registers every image; with
`spoil_image = 4` image 4 fails once with PP_REG_FEW_INLIERS, waits in the second bucket, and registers last.  No device runs here."""
import numpy as np
import pytest

import incremental_registration_scene as irs
import register_image_reference as ref
import tracks_image_reference as tir


def _oracle_estimate(oracle):
    def ransac(options, lines2D, points3D):
        lines = np.array([l.Line() for l in lines2D]).reshape(-1, 3)
        rep, mask = oracle.p6l_ransac(lines, np.array(points3D).reshape(-1, 3), np.zeros(len(lines2D), dtype=np.uint8), options.max_error, seed=0,
                                      min_inlier_ratio=options.min_inlier_ratio, confidence=options.confidence, mult=options.dyn_num_trials_multiplier,
                                      min_num_trials=options.min_num_trials, max_num_trials=options.max_num_trials)
        return int(rep.num_inliers), (mask if rep.success else np.zeros(len(lines2D), dtype=np.uint8)), np.array(rep.model).reshape(3, 4)
    return lambda o, l, X: ref.estimate_absolute_pose_from_lines(ransac, o, l, X)


def _run(oracle, spoil_image):
    rec, graph, info = irs.make_world(seed=0, spoil_image=spoil_image)
    m = ref.Mapper(rec, graph)
    options = ref.Options(abs_pose_min_num_inliers=irs.MIN_NUM_INLIERS)
    order, failures, first_pose = [], [], None
    for _ in range(20):
        ranked = m.find_next_images(options)
        if not ranked:
            break
        for image_id in ranked:
            ok = m.register_next_image(options, image_id, _oracle_estimate(oracle), lambda *a: True, lambda camera, px: px / camera.params[0])
            if not ok:
                failures.append((image_id, m.last["failure"], m.last["num_inliers"], len(m.last["tri_corrs"])))
                continue
            order.append(image_id)
            if first_pose is None:
                first_pose = (image_id, np.concatenate([rec.images[image_id].qvec, rec.images[image_id].tvec]), len(m.last["tri_corrs"]))
            tir.ImageOracle(graph, rec).TriangulateImage(tir.Options(), image_id)
            break
        else:
            break
    return rec, info, m, order, failures, first_pose


def test_every_image_registers_in_order(oracle):
    rec, info, m, order, failures, first_pose = _run(oracle, None)
    assert order == [3, 4, 5, 6, 7] and failures == []
    assert m.num_reg_trials == {i: 1 for i in order}
    image_id, pose, n = first_pose
    assert image_id == 3 and n >= 40
    assert np.abs(pose - info["poses"][3]).max() < 1e-8      # exact lines: the minimal solver's own rounding
    for i in order:
        got = np.concatenate([rec.images[i].qvec, rec.images[i].tvec])
        assert min(np.abs(got - info["poses"][i]).max(), np.abs(got * np.array([-1] * 4 + [1] * 3) - info["poses"][i]).max()) < 1e-5
    assert len(rec.points3D) >= 140


def test_a_spoiled_image_fails_once_and_registers_from_the_second_bucket(oracle):
    rec, info, m, order, failures, first_pose = _run(oracle, 4)
    print(order, failures)
    assert order == [3, 5, 6, 7, 4]
    assert len(failures) == 1 and failures[0][0] == 4 and failures[0][1] in (ref.FEW_INLIERS, ref.NO_INLIERS) and failures[0][3] >= irs.MIN_NUM_INLIERS
    assert m.num_reg_trials == {3: 1, 5: 1, 6: 1, 7: 1, 4: 2}
