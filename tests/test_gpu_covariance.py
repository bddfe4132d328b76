"""pp_ba_covariance on the device against the host references of tests/covariance_reference.py (never against the code under test).

Error of a block: e = ||Sigma - Sigma*||_F / sqrt(||Sigma*_ii||_F ||Sigma*_jj||_F).
Bar: e <= max(4 e_LAPACK, kappa_2(S_scaled) sqrt(n) u), u = 2^-53; e_LAPACK = the plain float64 Schur route against the refined one, 4 = another, equally
valid summation order.  Every scene has the default gauge of synthetic.make_ba_scene (pose 0 constant, tvec[1].x constant) unless the case says otherwise.

Seeds (all from the suite's existing scenes) and kappa_2(S_scaled), computed on the host (every test asserts kappa < 1e10 and bar < 1e-5 before it judges):
    cfg 1 (20 / 250 / 8)    seed 0xC0FFEE + 1   TRIVIAL 4.34e+02, constant blocks 1.18e+01, camera per image with f and k variable 3.17e+05
                            the same seed, THIN_PRISM_FISHEYE per image with fx fy and the 8 extra parameters variable (n = 313) 1.16e+06
    cfg 2 (100 / 5000 / 8)  seed 0xC0FFEE + 2   6.49e+04
    cfg 3 (500 / 25000 / 8) seed 0xC0FFEE + 3   8.64e+06;  the 500-image sequence (window 40), seed 0xC0FFEE + 3   5.97e+08
    cfg 1 noisy (0.5 px, 5 % outliers, float32 lines), Cauchy, at the solved parameters   4.19e+02
Observed on MI355X (ACCURACY lines: kappa, n, e_LAPACK, bar, worst pose / point error):
    cfg1 trivial dense      4.34e+02  113  2.86e-15  5.12e-13  8.83e-14  6.86e-14
    cfg1 constant blocks    1.18e+01  105  5.98e-16  1.35e-14  2.72e-15  2.38e-15
    cfg1 intrinsics tail    3.17e+05  153  6.08e-12  4.35e-10  1.73e-11  1.87e-11
    cfg1 intrinsics beside  3.17e+05  153  6.08e-12  4.35e-10  2.35e-11  2.55e-11
    cfg2 (default, PPSFM_CHOL_SPARSE=0, PPSFM_BA_ORDERING=natural, PPSFM_CHOL_MODE=columns: the same figures)
                            6.49e+04  593  2.58e-13  1.75e-10  1.01e-12  9.81e-13
    cfg1 noisy cauchy       4.19e+02  113  7.00e-15  4.95e-13  1.95e-14  3.30e-14
    seq500 default          5.97e+08 2993  1.94e-09  3.63e-06  2.36e-08  2.36e-08   (PPSFM_CHOL_SPARSE=0 the same, natural order 2.97e-08, columns 2.32e-08)
    cfg3 schur              8.64e+06 2993  8.98e-11  5.25e-08  7.07e-10  7.07e-10   (device 6.47 ms for every diagonal block and all 25 000 points)
The noisy Cauchy case runs with the default loss_function_scale of BundleAdjustmentOptions (1.0).  With a scale of 1e-3 (kappa 5.34e+03, bar 6.31e-12) the
device sat at pose 6.0e-12 / point 9.5e-12 against the oracle's Jacobians and at 1.2e-12 / 1.2e-12 against a reference built from its own: the oracle's
and the device's residuals differ by 2.3e-13 (3e-16 of the largest), and the Cauchy weight 1 / (1 + |r|^2 / scale^2) of an outlier carries that
difference, times 1 / scale^2, into the reference's H - an uncertainty of the reference's input, not of either inversion.
"""

import numpy as np
import pytest

import covariance_reference as cr
from privacy_preserving_sfm_amd import _capi, synthetic
from privacy_preserving_sfm_amd.device import BAProblem, ba_options

pytestmark = pytest.mark.gpu

CFG1 = dict(num_cams=20, num_points=250, track=8, seed=0xC0FFEE + 1, model=2)


def _all_pairs(C):
    return [(i, j) for i in range(C) for j in range(C)]


def _judge(tag, ref, schur, pose_cov, pairs, point_cov, points):
    """asserts every returned block inside the bar; ref: the judge (dense or refined Schur), schur: where e_LAPACK and kappa come from"""
    assert schur.kappa < 1e10, "%s: kappa(S_scaled) = %.2e: not a scene this suite may judge by" % (tag, schur.kappa)
    diag = sorted(set(i for ij in pairs for i in ij))
    e_lapack = max([cr.block_error(schur.pose(i, i, True), schur.pose(i, i), schur.pose(i, i), schur.pose(i, i)) for i in diag if schur.pose(i, i).any()] +
                   [cr.block_error(schur.point(p, True), schur.point(p), schur.point(p), schur.point(p)) for p in list(points)[:200] if schur.point(p).any()] + [0.0])
    limit = cr.bar(e_lapack, schur.kappa, schur.n)
    ep = max([cr.block_error(pose_cov[q], ref.pose(i, j), ref.pose(i, i), ref.pose(j, j)) for q, (i, j) in enumerate(pairs)] + [0.0])
    ex = max([cr.block_error(point_cov[q], ref.point(p), ref.point(p), ref.point(p)) for q, p in enumerate(points)] + [0.0])
    print("ACCURACY %-28s kappa %.2e n %4d e_lapack %.2e bar %.2e pose %.2e point %.2e" % (tag, schur.kappa, schur.n, e_lapack, limit, ep, ex))
    assert limit < 1e-5
    assert np.isfinite(pose_cov).all() and np.isfinite(point_cov).all()
    assert ep <= limit, "%s: pose blocks %.3e > %.3e" % (tag, ep, limit)
    assert ex <= limit, "%s: point blocks %.3e > %.3e" % (tag, ex, limit)


def test_cfg1_every_block_against_the_dense_inverse(oracle):
    sc = synthetic.make_ba_scene(**CFG1)
    pairs, points = _all_pairs(20), list(range(250))
    pb = BAProblem(sc, device=0)
    pc, xc, info = pb.covariance(pairs, points, return_info=True)
    pb.close()
    assert info.n == 120 and info.device_ms > 0
    _judge("cfg1 trivial dense", cr.dense_covariance(sc), cr.SchurCovariance(sc), pc, pairs, xc, points)
    for q, (i, j) in enumerate(pairs):      # the block of (j, i) is the transpose of the block of (i, j)
        assert np.allclose(pc[q], pc[pairs.index((j, i))].T, rtol=1e-9, atol=0)
    assert not pc[pairs.index((0, 0))].any() and not pc[pairs.index((0, 5))].any()      # constant pose
    b11 = pc[pairs.index((1, 1))]
    assert not b11[3].any() and not b11[:, 3].any() and b11[0, 0] > 0                     # constant tvec component


def test_cfg1_noisy_cauchy_after_a_solve(oracle):
    sc = synthetic.make_ba_scene(**CFG1, line_noise_px=0.5, outlier_obs=0.05, quantise_float32=True)
    sc["loss_type"], sc["loss_scale"] = 2, 1.0      # BundleAdjustmentOptions' default loss_function_scale
    pb = BAProblem(sc, device=0)
    pb.solve(ba_options(max_num_iterations=30))
    poses, points_, intr = pb.get_parameters()
    pairs, points = _all_pairs(20), list(range(250))
    pc, xc = pb.covariance(pairs, points)
    pb.close()
    at = dict(sc, poses=poses, points=points_, intr=intr)
    _judge("cfg1 noisy cauchy", cr.dense_covariance(at), cr.SchurCovariance(at), pc, pairs, xc, points)


def test_constant_blocks_are_zero_where_stated(oracle):
    sc = synthetic.make_ba_scene(**CFG1)
    sc["pose_const"][5] = 1
    sc["tvec_const_mask"][7] = 0b101
    sc["point_const"][::10] = 1
    pairs, points = _all_pairs(20), list(range(250))
    pb = BAProblem(sc, device=0)
    pc, xc = pb.covariance(pairs, points)
    pb.close()
    for q, (i, j) in enumerate(pairs):
        if i in (0, 5) or j in (0, 5):
            assert not pc[q].any()
        if i == 7:
            assert not pc[q][3].any() and not pc[q][5].any()
        if j == 7:
            assert not pc[q][:, 3].any() and not pc[q][:, 5].any()
        if i == 1:
            assert not pc[q][3].any()
    assert not xc[::10].any() and all(xc[p].any() for p in range(250) if p % 10)
    _judge("cfg1 constant blocks", cr.dense_covariance(sc), cr.SchurCovariance(sc), pc, pairs, xc, points)


@pytest.mark.parametrize("layout", ["tail", "beside"])
def test_camera_per_image_variable_intrinsics(oracle, monkeypatch, layout):
    monkeypatch.setenv("PPSFM_BA_INTR_LAYOUT", layout)
    sc = synthetic.make_ba_scene(**CFG1, num_intrinsics=20)
    sc["camera_const_mask"][:] = 0xFFFF & ~0b1001      # SIMPLE_RADIAL: f and k variable
    pairs, points = _all_pairs(20), list(range(250))
    pb = BAProblem(sc, device=0)
    pc, xc, info = pb.covariance(pairs, points, return_info=True)
    pb.close()
    assert info.n == 120 + 40
    _judge("cfg1 intrinsics " + layout, cr.dense_covariance(sc), cr.SchurCovariance(sc), pc, pairs, xc, points)


@pytest.mark.parametrize("layout", ["tail", "beside"])
def test_twelve_parameter_model_with_focal_and_extra_parameters_variable(oracle, monkeypatch, layout):
    """THIN_PRISM_FISHEYE (12 parameters), a camera per image, fx fy and the eight extra parameters variable: 10 variable columns per camera, more than the
    widest compact layout of the solver's specialised paths (8).  cx and cy stay constant: a line observation is stored relative to the principal point,
    so their Jacobian columns are identically zero (the oracle's too) and H would be singular with them."""
    monkeypatch.setenv("PPSFM_BA_INTR_LAYOUT", layout)
    sc = synthetic.make_ba_scene(**dict(CFG1, model=10), num_intrinsics=20)
    sc["camera_const_mask"][:] = 0xFFFF & ~0b111111110011
    pairs, points = _all_pairs(20), list(range(250))
    pb = BAProblem(sc, device=0)
    pc, xc, info = pb.covariance(pairs, points, return_info=True)
    pb.close()
    assert info.n == 120 + 200
    _judge("cfg1 thin-prism 10 var " + layout, cr.dense_covariance(sc), cr.SchurCovariance(sc), pc, pairs, xc, points)


def _sampled(C, P, rng, npairs, npoints):
    pairs = [(i, i) for i in range(C)] + [tuple(int(v) for v in rng.integers(0, C, 2)) for _ in range(npairs)]
    return pairs, sorted(int(v) for v in rng.choice(P, size=min(P, npoints), replace=False))


@pytest.mark.parametrize("scene_kw", [dict(num_cams=100, num_points=5000, track=8, seed=0xC0FFEE + 2, model=2),
                                      dict(num_cams=500, num_points=25000, track=8, seed=0xC0FFEE + 3, model=2, window=40)], ids=["cfg2", "sequence500"])
def test_switch_variants_agree_to_the_bar(oracle, monkeypatch, scene_kw):
    sc = synthetic.make_ba_scene(**scene_kw)
    C, P = scene_kw["num_cams"], scene_kw["num_points"]
    pairs, points = _sampled(C, P, np.random.default_rng(5), 200, 300)
    schur = cr.SchurCovariance(sc)
    seq = bool(scene_kw.get("window"))
    # what shows that a switch took effect: (info.path, images renumbered, block-sparse handle); PP_LINSOLVE_*: COLUMNS 0, TASKS 1, SPARSE 2.
    #  - cfg 2 is dense in any order (every image shares points with every other): only the launch structure has anything to change there.
    #  - the sequence is block-sparse and renumbered by AUTO; a block-sparse factorisation reports SPARSE on either launch structure, so the columns switch
    #    shows on cfg 2 only.
    #  - PPSFM_CHOL_SPARSE is the switch of pp_dense_cholesky_solve: a handle does not read it, and its run must equal the default's in
    #    every respect.  The handle's own switch for the dense treatment of a block-sparse system is PPSFM_BA_SPARSE, run beside it.
    expect = {"default": (2, True, True) if seq else (1, False, False), "chol_sparse=0": (2, True, True) if seq else (1, False, False),
              "ba_sparse=0": (1, False, False), "ordering=natural": (2, False, True) if seq else (1, False, False),
              "chol_mode=columns": (2, True, True) if seq else (0, False, False)}
    got = {}
    for name, env in (("default", {}), ("chol_sparse=0", {"PPSFM_CHOL_SPARSE": "0"}), ("ba_sparse=0", {"PPSFM_BA_SPARSE": "0"}),
                      ("ordering=natural", {"PPSFM_BA_ORDERING": "natural"}), ("chol_mode=columns", {"PPSFM_CHOL_MODE": "columns"})):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            pb = BAProblem(sc, device=0)
            st = pb.structure()
            pc, xc, info = pb.covariance(pairs, points, return_info=True)
            pb.close()
        print("VARIANT %s %s: path %d reordered %d block_sparse %d nnz_used %d of %d" % (scene_kw.get("window") and "seq500" or "cfg2", name, info.path, st["reordered"],
                                                                                     st["block_sparse"], st["nnz_used"], st["tiles"]))
        assert (info.path, st["reordered"], st["block_sparse"]) == expect[name], (name, info.path, st)
        got[name] = (pc, xc)
        _judge("%s %s path %d %.1f ms" % (scene_kw.get("window") and "seq500" or "cfg2", name, info.path, info.device_ms), schur, schur, pc, pairs, xc, points)
    assert np.array_equal(got["default"][0], got["chol_sparse=0"][0]) and np.array_equal(got["default"][1], got["chol_sparse=0"][1])


def test_cfg3_full_size_against_the_schur_reference(oracle):
    sc = synthetic.make_ba_scene(500, 25000, 8, seed=0xC0FFEE + 3, model=2)
    pairs, points = _sampled(500, 25000, np.random.default_rng(6), 1000, 2000)
    pb = BAProblem(sc, device=0)
    pc, xc, info = pb.covariance(pairs, points, return_info=True)
    _, _, info_all = pb.covariance(None, list(range(25000)), return_info=True)      # the figure DESIGN.md section 6 reports: every diagonal block, every point
    pb.close()
    print("COVARIANCE cfg3: sampled request %.2f ms, all 500 diagonal blocks + 25000 points %.2f ms (n = %d, path %d)" % (info.device_ms, info_all.device_ms, info.n, info.path))
    schur = cr.SchurCovariance(sc)
    _judge("cfg3 schur", schur, schur, pc, pairs, xc, points)
    for q in range(1, 500):      # every returned diagonal block of a variable pose is symmetric positive definite (pose 1 has one constant component)
        b = pc[q] if q != 1 else np.delete(np.delete(pc[q], 3, 0), 3, 1)
        assert np.allclose(b, b.T, rtol=1e-9, atol=0) and np.linalg.eigvalsh(0.5 * (b + b.T))[0] > 0
    for b in xc:
        assert np.allclose(b, b.T, rtol=1e-12, atol=0) and np.linalg.eigvalsh(b)[0] > 0


def test_two_calls_are_bitwise_equal():
    sc = synthetic.make_ba_scene(100, 5000, 8, seed=0xC0FFEE + 2, model=2)
    pairs, points = _sampled(100, 5000, np.random.default_rng(7), 100, 500)
    pb = BAProblem(sc, device=0)
    a = pb.covariance(pairs, points)
    b = pb.covariance(pairs, points)
    pb.close()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("scene_kw", [CFG1, dict(num_cams=100, num_points=5000, track=8, seed=0xC0FFEE + 2, model=2)], ids=["cfg1", "cfg2"])
def test_covariance_then_solve_equals_solve_alone(scene_kw):
    sc = synthetic.make_ba_scene(**scene_kw)
    out = []
    for with_cov in (True, False):
        pb = BAProblem(sc, device=0)
        if with_cov:
            pb.covariance(None, list(range(0, scene_kw["num_points"], 7)))
        s = pb.solve(ba_options(max_num_iterations=8))
        out.append((pb.get_parameters(), pb.trace(), (s.initial_cost, s.final_cost, s.num_successful_steps, s.num_unsuccessful_steps, s.termination, s.num_iterations,
                                                      s.linear_solver, s.cholesky_fallbacks)))
        pb.close()
    (pa, ta, sa), (pb_, tb, sb) = out
    assert all(np.array_equal(x, y) for x, y in zip(pa, pb_)) and np.array_equal(ta, tb) and sa == sb


def test_covariance_between_two_solves_changes_nothing():
    """a used handle: solve, covariance, solve against solve, solve - the call overwrites only what the next solve recomputes (Jacobians, U, V, gradients, the
    gather records), and the graph of the handle's own factorisation, captured by the first solve, still replays on the handle's own buffers"""
    sc = synthetic.make_ba_scene(100, 5000, 8, seed=0xC0FFEE + 2, model=2)
    out = []
    for with_cov in (True, False):
        pb = BAProblem(sc, device=0)
        s1 = pb.solve(ba_options(max_num_iterations=3))
        if with_cov:
            pb.covariance(None, list(range(0, 5000, 7)))
        s2 = pb.solve(ba_options(max_num_iterations=5))
        out.append((pb.get_parameters(), pb.trace(), [(s.initial_cost, s.final_cost, s.num_successful_steps, s.num_unsuccessful_steps, s.termination, s.num_iterations,
                                                        s.linear_solver, s.cholesky_fallbacks) for s in (s1, s2)]))
        pb.close()
    (pa, ta, sa), (pb_, tb, sb) = out
    assert all(np.array_equal(x, y) for x, y in zip(pa, pb_)) and np.array_equal(ta, tb) and sa == sb


def test_group_attached_handle_is_refused():
    """a host-callback group of one rank is a group all the same (the handle may hold a shard): refused with a message that says so, and served again
    once detached"""
    sc = synthetic.make_ba_scene(**CFG1)
    pb = BAProblem(sc, device=0, ordering=1)      # (PP_ORDERING_NATURAL: what a group's handles are created with)
    pb.set_allreduce(lambda ptr, count, op: 0, group_rank=0, group_size=1)
    with pytest.raises(_capi.PPError) as e:
        pb.covariance()
    assert e.value.code == _capi.PP_ERR_INVALID and "attached to a group" in str(e.value)
    pb.set_allreduce(None)
    pc, _ = pb.covariance()
    pb.close()
    assert pc.shape == (20, 6, 6) and np.isfinite(pc).all() and pc[2][0, 0] > 0


def test_error_reporting():
    sc = synthetic.make_ba_scene(**CFG1)
    pb = BAProblem(sc, device=0, linear_solver=_capi.LINEAR_SOLVER_ITERATIVE_SCHUR)
    with pytest.raises(_capi.PPError) as e:
        pb.covariance()
    assert e.value.code == _capi.PP_ERR_INVALID and "iterative" in str(e.value)
    pb.close()
    pb = BAProblem(sc, device=0)
    for kw in (dict(pose_pairs=[(0, 20)]), dict(pose_pairs=[(-1, 0)]), dict(points=[250])):
        with pytest.raises(_capi.PPError) as e:
            pb.covariance(**kw)
        assert e.value.code == _capi.PP_ERR_INVALID and "out of range" in str(e.value)
    pb.close()
    # the gauge left free: an ordinary numeric failure report, and the handle solves cleanly afterwards
    free = synthetic.make_ba_scene(**CFG1)
    free["pose_const"][:] = 0
    free["tvec_const_mask"][:] = 0
    pb = BAProblem(free, device=0)
    with pytest.raises(_capi.PPError) as e:
        pb.covariance()
    assert e.value.code == _capi.PP_ERR_NUMERIC
    s = pb.solve(ba_options(max_num_iterations=5))
    assert s.num_successful_steps >= 1 and s.final_cost < s.initial_cost
    pb.close()
    ref = BAProblem(free, device=0)
    s2 = ref.solve(ba_options(max_num_iterations=5))
    assert (s.final_cost, s.num_iterations) == (s2.final_cost, s2.num_iterations)
    ref.close()
