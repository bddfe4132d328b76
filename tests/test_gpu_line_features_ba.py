"""The lines of pp_line_features_from_keypoints (K19) are in the coordinates the bundle adjustment expects: the observations of a mixed-model scene at
its ground truth are projected to pixels with the oracle's WorldToImage, rounded to float32 keypoints, turned into lines on the device (ratio 0: random
directions) and evaluated through the existing BAProblem.  A float32 at 1280 px has a spacing of 1.2e-4 px, so rounding moves a keypoint by about
1e-4 px; every residual must stay below 1e-3 px, ten times that.  With the round trip of tests/test_line_features_host.py (the other direction) this
pins ImageToWorld on the device to the WorldToImage the residuals are evaluated with."""
import numpy as np
import pytest

import mixed_models
from privacy_preserving_sfm_amd.bundle_adjustment import _quat_to_rot
from privacy_preserving_sfm_amd.device import BAProblem, LineFeatureGenerator

pytestmark = pytest.mark.gpu


def test_device_lines_have_zero_residual_at_the_ground_truth(oracle):
    sc = mixed_models.mixed_ba_scene(6, 40, 3)
    sc["poses"], sc["points"] = sc["gt_poses"].copy(), sc["gt_points"].copy()
    obs_pose, obs_point = sc["obs_pose"], sc["obs_point"]
    cam_of_obs = sc["pose_camera"][obs_pose]
    assert len(set(int(m) for m in sc["camera_model"][sc["pose_camera"]])) == 6      # six images, six models
    pixels = np.zeros((len(obs_pose), 2))
    for o in range(len(obs_pose)):
        q = sc["poses"][obs_pose[o]]
        X = _quat_to_rot(q[:4]) @ sc["points"][obs_point[o]] + q[4:]
        k = int(cam_of_obs[o])
        pixels[o] = oracle.world_to_image(int(sc["camera_model"][k]), sc["intr"][k], X[0] / X[2], X[1] / X[2])
    assert pixels.min() > 0 and pixels[:, 0].max() < 1280 and pixels[:, 1].max() < 960
    # keypoints by image: line index = keypoint index
    order = np.argsort(obs_pose, kind="stable")
    counts = np.bincount(obs_pose, minlength=6)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out = LineFeatureGenerator(0).generate(image_ids=np.arange(6) + 1, kp_start=start, keypoints=pixels[order].astype(np.float32),
                                           image_camera=sc["pose_camera"], camera_model=sc["camera_model"], intr=sc["intr"],
                                           has_gravity=np.zeros(6, dtype=np.uint8), aligned_line_ratio=0.0, seed=3)
    rep = out["report"]
    assert rep.num_lines == len(obs_pose) and rep.num_aligned == 0 and rep.num_degenerate == 0 and rep.num_newton_exhausted == 0
    assert rep.num_images_without_gravity == 6
    lines = np.zeros((len(obs_pose), 3))
    lines[order] = out["lines"]
    assert np.abs(np.linalg.norm(lines[:, :2], axis=1) - 1).max() <= 1e-12
    sc["lines"] = np.ascontiguousarray(lines)
    pb = BAProblem(sc, device=0)
    _, r, _, _, _ = pb.evaluate()
    pb.close()
    print("largest residual %.3g px over %d observations" % (np.abs(r).max(), len(obs_pose)))
    assert np.abs(r).max() < 1e-3
