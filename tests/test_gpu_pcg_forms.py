"""The edges of the conjugate-gradient vector step (k_pcg_step, csrc/ba_pcg.hip) that both forms of the loop share: the last pose workgroup full to the
thread / two threads into the next one, and the intrinsics workgroups behind MORE than one pose workgroup.  The other iterative scenes have one
vector-step workgroup (60 images) or twelve (1500 images).  Not covered: more than 64 vector-step workgroups (C > 8192), where PcgDecide's lanes take
more than one part each - too large for a test of seconds."""
import numpy as np
import pytest

from privacy_preserving_sfm_amd import synthetic
from test_gpu_bundle_adjustment import _intr_scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cams", [128, 129])      # 2 C = 256 parameter blocks: exactly one workgroup; 258: a second one with two live threads
def test_iterative_schur_vector_step_workgroup_edges_run_the_same_loop(cams, monkeypatch):
    """What test_iterative_schur_many_workgroup_vector_step_runs_the_same_loop asserts, with its tolerances, of the three-launch form (the default)
    against the four-launch form (PPSFM_PCG_FUSED=0, the anchor) at the workgroup edges of the vector step.
    20 points per image: with 10 the inner loops run to 400 iterations and more and the two forms, which sum in different orders, part by more than
    these tolerances in at least one of the two scenes for four seeds of six (CG counts up to 8 apart, parameters beyond 1e-7) - already before the
    vector steps were merged, so the scene, not the tolerance, was changed; at 20 five seeds of six pass, the first of them is used."""
    from privacy_preserving_sfm_amd.device import BAProblem, ba_options
    sc = synthetic.make_ba_scene(cams, 20 * cams, 3, seed=0xC0FFEE + 40, model=2, window=12)
    runs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("PPSFM_PCG_FUSED", fused)
        pb = BAProblem(sc, linear_solver=2)
        s = pb.solve(ba_options(max_num_iterations=5, eta=1e-3))
        poses, points, _ = pb.get_parameters()
        runs.append((s, pb.trace().copy(), poses, points))
        pb.close()
    (sw, tw, pw, xw), (s1, t1, p1, x1) = runs
    print("C=%d: LM iterations %d / %d, CG iterations %d / %d, costs %s / %s" % (cams, sw.num_iterations, s1.num_iterations, sw.linear_solver_iterations,
                                                                             s1.linear_solver_iterations, tw[:, 0], t1[:, 0]))
    assert sw.linear_solver == s1.linear_solver == 3 and sw.num_iterations == s1.num_iterations
    assert sw.linear_solver_iterations > 12 * sw.num_iterations // 2      # long enough inner loops to cross the residual reset
    assert abs(sw.linear_solver_iterations - s1.linear_solver_iterations) <= 3
    big = t1[:, 0] > 1e-12 * t1[0, 0]      # (below that the accept / reject pattern is rounding)
    assert big.sum() >= 3 and np.array_equal(tw[big, 6], t1[big, 6]) and np.allclose(tw[big, 0], t1[big, 0], rtol=1e-7)
    assert np.abs(pw - p1).max() <= 1e-7 * np.abs(p1).max() and np.abs(xw - x1).max() <= 1e-7 * np.abs(x1).max()


def test_iterative_schur_intrinsics_behind_two_pose_workgroups_takes_the_direct_solvers_steps():
    """What test_iterative_schur_with_variable_intrinsics_takes_the_direct_solvers_steps asserts, at its 1e-7, with 129 images: the three cameras'
    workgroup of the vector step sits behind TWO pose workgroups, the second with two live threads.  The partner is the direct factorisation."""
    from privacy_preserving_sfm_amd.device import BAProblem, ba_options
    sc = _intr_scene(129, 1300, 4, 2, 3, 0b0110, seed=0xC0FFEE + 78)
    out = []
    for ls in (1, 2):
        pb = BAProblem(sc, linear_solver=ls)
        s = pb.solve(ba_options(max_num_iterations=3, eta=1e-14, max_linear_solver_iterations=3000))
        out.append((s, pb.get_parameters(), pb.trace().copy()))
        pb.close()
    (sd, (pd, xd, kd), td), (si, (pi, xi, ki), ti) = out
    print("CG iterations %d, costs %s / %s, max differences %.3g %.3g %.3g" % (si.linear_solver_iterations, td[:, 0], ti[:, 0], np.abs(ki - kd).max() / np.abs(kd).max(),
                                                                               np.abs(pi - pd).max() / np.abs(pd).max(), np.abs(xi - xd).max() / np.abs(xd).max()))
    assert sd.linear_solver != 3 and si.linear_solver == 3 and si.linear_solver_iterations > 3 * 20
    assert np.array_equal(td[:, 6], ti[:, 6]) and np.allclose(td[:, 0], ti[:, 0], rtol=1e-7)
    assert np.abs(ki - kd).max() <= 1e-7 * np.abs(kd).max() and np.abs(pi - pd).max() <= 1e-7 * np.abs(pd).max() and np.abs(xi - xd).max() <= 1e-7 * np.abs(xd).max()
