"""The edges of the step kernels (csrc/ba_step.hip) that the two forms of a trial step share: k_step_points (PPSFM_BA_FUSED_STEP=1, the default) against
k_backsub_points + k_model_cost_apply (+ the cost-only evaluation), and inside the latter the trial cost fused (PPSFM_BA_FUSED_TRIAL_COST=1) against its own
launch.  The scenes of tests/test_gpu_bundle_adjustment.py have 260 or 300 points and 4 to 11 observations per point; here: the lanes of the four-lane walk
with no, one and two rows and one and two reloads, the last point workgroup full to the point and one point into the next, the last observation workgroup full
to the observation and four observations into the next, variable intrinsics through both forms at 1e-7 (the host-callback group reaches the two-kernel form
with them at a loose tolerance only), and a second pose workgroup with one live thread.  Not covered: more than 8 x 256 images, where the norms kernel's
pose blocks saturate and a thread takes more than one image - a reduced system of that size is no test of seconds."""
import numpy as np
import pytest

from privacy_preserving_sfm_amd import synthetic
from test_gpu_bundle_adjustment import _intr_scene

pytestmark = pytest.mark.gpu


def _solve_both_step_forms(sc, monkeypatch, **opts):
    from privacy_preserving_sfm_amd.device import BAProblem, ba_options
    runs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("PPSFM_BA_FUSED_STEP", fused)
        pb = BAProblem(sc, linear_solver=1)
        s = pb.solve(ba_options(**opts))
        poses, points, intr = pb.get_parameters()
        runs.append((pb.trace().copy(), poses.copy(), points.copy(), intr.copy(), s))
        pb.close()
    return runs


def _assert_fused_follows_two_kernel_form(runs, sc, num_const):
    """the assertions and tolerances of test_fused_point_step_follows_the_two_kernel_form"""
    (tf, pf, xf, kf, sf), (t0, p0, x0, k0, s0) = runs
    n = min(len(tf), len(t0))
    assert n > 3
    tf, t0 = tf[:n], t0[:n]
    big = t0[:, 0] > 1e-12 * t0[0, 0]
    moving = np.concatenate([[True], np.abs(np.diff(t0[:, 0])) > 1e-9 * t0[1:, 0]])
    big &= np.cumprod(moving).astype(bool)
    print("rows %d / %d, compared %d, costs %s / %s, max differences %.3g %.3g" % (len(runs[0][0]), len(runs[1][0]), big.sum(), tf[:, 0], t0[:, 0],
                                                                                 np.abs(pf - p0).max() / np.abs(p0).max(), np.abs(xf - x0).max() / np.abs(x0).max()))
    assert big.sum() > 3
    assert np.array_equal(tf[big, 6], t0[big, 6]) and np.allclose(tf[big, 0], t0[big, 0], rtol=1e-10) and np.allclose(tf[big, 5], t0[big, 5], rtol=1e-7)
    assert np.abs(pf - p0).max() <= 1e-7 * np.abs(p0).max() and np.abs(xf - x0).max() <= 1e-7 * np.abs(x0).max()
    assert np.array_equal(xf[:num_const], sc["points"][:num_const])      # constant points did not move


# observations per point: 3 - a lane with none; 5 - lane 0 holds two rows, the others one; 9 - lane 0's third observation is loaded again; 13 - its
# third and fourth.  Points: 64 per workgroup - the last workgroup one short, full, and a second workgroup with one point.
@pytest.mark.parametrize("num_points", [63, 64, 65])
@pytest.mark.parametrize("track", [3, 5, 9, 13])
def test_four_lane_walk_at_lane_and_workgroup_edges(track, num_points, monkeypatch):
    sc = synthetic.make_ba_scene(14, num_points, track, seed=33 + track, model=2)
    rng = np.random.default_rng(33)
    sc["points"] = sc["gt_points"] + 0.3 * rng.normal(size=sc["gt_points"].shape)
    sc["point_const"][:5] = 1
    sc["loss_type"] = 1; sc["loss_scale"] = 0.8
    runs = _solve_both_step_forms(sc, monkeypatch, max_num_iterations=20)
    _assert_fused_follows_two_kernel_form(runs, sc, 5)


# 256 observations: one observation workgroup, full; 260: a second one with four live threads
@pytest.mark.parametrize("num_points", [64, 65])
@pytest.mark.parametrize("loss", [0, 2])
def test_fused_trial_cost_bit_for_bit_at_the_observation_workgroup_edge(loss, num_points, monkeypatch):
    """the assertion of test_fused_trial_cost_is_the_separate_launch_bit_for_bit"""
    from privacy_preserving_sfm_amd.device import BAProblem, ba_options
    monkeypatch.setenv("PPSFM_BA_FUSED_STEP", "0")
    runs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("PPSFM_BA_FUSED_TRIAL_COST", fused)
        sc = synthetic.make_ba_scene(12, num_points, 4, seed=21, model=2)
        assert len(sc["lines"]) == 4 * num_points
        rng = np.random.default_rng(21)
        sc["points"] = sc["gt_points"] + 0.4 * rng.normal(size=sc["gt_points"].shape)
        sc["loss_type"] = loss; sc["loss_scale"] = 0.7
        pb = BAProblem(sc)
        pb.solve(ba_options(max_num_iterations=25))
        poses, points, _ = pb.get_parameters()
        runs.append((pb.trace().copy(), poses.copy(), points.copy()))
        pb.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    assert len(runs[0][0]) > 3


def test_variable_intrinsics_through_both_step_forms(monkeypatch):
    """k_step_points<true> behind the trial intrinsics against k_backsub_points, k_model_cost_apply and the cost-only evaluation with the trial intrinsics.
    Initial radius 1: from the default 1e4 this scene is at 1e-12 of its first cost after three steps (with or without noise on its lines), both forms
    alike, which leaves three rows to compare where the assertions ask for more than three; from 1 it takes eight."""
    sc = _intr_scene(14, 260, 5, 2, 3, 0b0110, seed=0xC0FFEE + 91)
    rng = np.random.default_rng(91)
    sc["points"] = sc["gt_points"] + 0.3 * rng.normal(size=sc["gt_points"].shape)
    sc["point_const"][:5] = 1
    sc["loss_type"] = 1; sc["loss_scale"] = 0.8
    runs = _solve_both_step_forms(sc, monkeypatch, max_num_iterations=20, initial_trust_region_radius=1.0)
    _assert_fused_follows_two_kernel_form(runs, sc, 5)
    kf, k0 = runs[0][3], runs[1][3]
    assert np.abs(kf - k0).max() <= 1e-7 * np.abs(k0).max()
    assert not np.array_equal(k0, np.asarray(sc["intr"]))      # (they were refined)


def test_second_pose_workgroup_with_one_live_thread(monkeypatch):
    """257 images: the pose role of k_step_points, ApplyStepBody and the norms kernel's pose blocks take a second workgroup for the last image.
    Half a pixel of noise on the lines: five iterations are all this test has, and the noise-free scene with its points moved instead had its third step
    rejected (both forms alike), after which nothing is compared."""
    sc = synthetic.make_ba_scene(257, 20 * 257, 4, seed=0xC0FFEE + 92, model=2, window=12, line_noise_px=0.5)
    sc["point_const"][:5] = 1
    sc["loss_type"] = 1; sc["loss_scale"] = 0.8
    runs = _solve_both_step_forms(sc, monkeypatch, max_num_iterations=5)
    _assert_fused_follows_two_kernel_form(runs, sc, 5)
