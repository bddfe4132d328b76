"""Cameras of DIFFERENT models in one problem, across the bundle-adjustment pipeline, the filters, the track triangulation and track completion / merging.

Every other scene of the suite gives all its cameras one model; the reference gives every camera its own parameter block with its own size and constant
subset (BundleAdjuster::SetUp, src/optim/bundle_adjustment.cc:260-542).  What runs here for the first time: the model id packed per observation and switched
on per lane (ba_eval.hip k_eval; in point order the lanes of one wavefront take different arms), compact intrinsics columns of per-camera width with an
unreferenced camera in the middle of the array, rectangular n_v(a) x n_v(b) intrinsics block pairs, a preconditioner block per camera of its own size, the
camera-per-image wide path with the same even width at other columns per model - and its refusal when the widths differ -, per-camera strides in
ba_filter.hip, triangulation.hip and tracks.hip.

The scenes come from tests/mixed_models.py (checked with the oracle alone by tests/test_mixed_models.py); every comparison is against the CPU oracle or the
host references of tests/, except where a switch is compared with the default.  Every numeric bar is the one of the homogeneous test named beside it.
Sizes: 22 images / 11 cameras / 1200 observations - one wavefront of 64 observations spans several models, intr_off is non-trivial."""
import numpy as np
import pytest

import fuzz_scenes
import mixed_models as mm
from cholesky_reference import var_cols as _var_cols
from privacy_preserving_sfm_amd import synthetic

pytestmark = pytest.mark.gpu

TRACK_MODELS = [0, 2, 4, 5, 7, 9, 10]


def _assert_close(got, want, rtol, name):      # test_gpu_line_eval._assert_close: the scale rule of test_eval_matches_oracle_all_models
    scale = max(1.0, float(np.abs(want).max()))
    err = np.abs(got - want)
    assert np.all(err <= rtol * scale + rtol * np.abs(want)), (name, float(err.max()), scale)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _check_eval(oracle, sc):
    from privacy_preserving_sfm_amd.device import BAProblem
    pb = BAProblem(sc)
    try:
        for ambient in (False, True):
            cost, r, jp, jx, jc = pb.evaluate(ambient=ambient, want_cam=True)
            r0, jp0, jx0, jc0 = oracle.ba_eval(sc, ambient=ambient, want_cam=True)
            # 1e-11, and 1e-10 for Jcam: test_gpu_line_eval.test_eval_matches_oracle_all_models
            _assert_close(r, r0, 1e-11, "r")
            _assert_close(jp, jp0, 1e-11, "Jpose")
            _assert_close(jx, jx0, 1e-11, "Jpoint")
            _assert_close(jc, jc0, 1e-10, "Jcam")
            # per model as well: a 12-parameter camera's entries must not set the scale a 3-parameter camera is judged by
            model = sc["camera_model"][sc["pose_camera"][sc["obs_pose"]]]
            jc, jc0 = jc.reshape(-1, 2, 12), jc0.reshape(-1, 2, 12)
            for m in sorted(set(int(v) for v in model)):
                _assert_close(jc[model == m], jc0[model == m], 1e-10, "Jcam of model %d" % m)
                assert not jc[model == m][:, :, synthetic.NUM_PARAMS[m]:].any(), m      # nothing behind a model's parameters
            c0, _ = oracle.ba_cost(sc)
            assert abs(cost - c0) <= 1e-11 * max(1.0, c0)
    finally:
        pb.close()


@pytest.mark.parametrize("sort", ["pose", "point"])
def test_eval_all_models_in_one_scene_matches_oracle(oracle, sort):
    """all 11 models in one launch; sort="point": neighbouring lanes belong to different images, so one wavefront runs several arms of the model switch"""
    sc = mm.mixed_ba_scene(22, 300, 4, seed=5, model=2, sort=sort)
    model = sc["camera_model"][sc["pose_camera"][sc["obs_pose"]]]
    per_wave = [len(set(model[o:o + 64])) for o in range(0, len(model), 64)]
    assert min(per_wave) >= (4 if sort == "point" else 1) and max(per_wave) >= 2, per_wave
    _check_eval(oracle, sc)


def test_eval_narrowest_beside_widest_model_in_a_ragged_wave(oracle):
    """two images, SIMPLE_PINHOLE (3 parameters) and THIN_PRISM_FISHEYE (12): 140 observations = two wavefronts and a tail of 12 lanes, both arms in each"""
    sc = mm.mixed_ba_scene(2, 70, 2, models=[0, 10], seed=5, model=2)
    assert len(sc["obs_pose"]) == 140 and set(sc["obs_pose"][128:]) == {0, 1}
    _check_eval(oracle, sc)


@pytest.mark.parametrize("rule,unused,loss", [("widths", (), 0), ("widths", (4,), 2), ("focal", (4,), 0), ("focal", (), 2), ("stride3", (4,), 2)])
def test_reduced_system_with_mixed_widths_matches_oracle(oracle, rule, unused, loss):
    """masks (a) and (c) (and the principal point partly free: zero columns): per-camera n_v from 0 to 8, rectangular block pairs between cameras, one
    camera without columns, one unreferenced camera (intr_off = -1) between two that have some.
    The Cauchy loss runs at the default scale 1.0, as in test_reduced_system_matches_oracle whose bar this is.  At scale 0.05 (residuals of ~3 px: weights of
    1e-4) the POSE-POSE blocks at radius 1e4 miss this bar by a factor 4.4-4.6 here and by 6.3-13.8 on the same scene with ONE model (SIMPLE_RADIAL, OPENCV,
    THIN_PRISM_FISHEYE; measured on an MI355X), the pose-intrinsics and intrinsics blocks stay below 0.15 of it, and at radius 100 everything below 0.08: the
    conditioning of V_p^-1 under tiny weights, whatever the models - the fuzz tests judge that regime at their 1e-8."""
    from privacy_preserving_sfm_amd.device import BAProblem
    sc = mm.perturb_variable_intrinsics(mm.mixed_ba_scene(22, 300, 4, seed=5, model=2, sort="point", rule=rule, unused=unused), 6)
    sc["loss_type"], sc["loss_scale"] = loss, 1.0
    sc["point_const"] = sc["point_const"].copy(); sc["point_const"][:9] = 1
    nv = mm.num_variable(sc)
    referenced = sorted(set(int(k) for k in sc["pose_camera"]))
    assert (len(referenced) == 10) == bool(unused)
    pb = BAProblem(sc)
    try:
        st = pb.structure()
        assert st["intrinsics_columns"] == int(nv[referenced].sum()) and st["private_intrinsics"] == 0 and st["wide_intrinsics"] == 0
        for radius in (1e4, 100.0):
            S, rhs = pb.reduced_system(radius)
            ref = oracle.ba_reduced_system(sc, radius)
            cols = _var_cols(sc)
            assert S.shape[0] == 6 * 22 + int(nv[referenced].sum())
            assert len(cols) == ref["nc"]
            # rtol 1e-9, atol 1e-11 of the largest entry: test_gpu_bundle_adjustment.test_reduced_system_with_variable_intrinsics_matches_oracle
            scale = np.abs(ref["S"]).max()
            assert np.allclose(S[np.ix_(cols, cols)], ref["S"], rtol=1e-9, atol=1e-11 * scale)
            assert np.allclose(rhs[cols], ref["rhs"], rtol=1e-9, atol=1e-11 * np.abs(ref["rhs"]).max())
            # constant columns: identity rows, zero rhs (test_reduced_system_matches_oracle)
            fixed = np.setdiff1d(np.arange(S.shape[0]), cols)
            assert np.array_equal(S[np.ix_(fixed, fixed)], np.eye(len(fixed))) and np.all(S[np.ix_(fixed, cols)] == 0) and np.all(rhs[fixed] == 0)
    finally:
        pb.close()


def _per_image_scene(num_images, num_points, rule, **kw):
    sc = mm.mixed_ba_scene(num_images, num_points, 5, models=[1, 2, 8, 4], num_intrinsics=num_images, rule=rule, model=2, **kw)
    return mm.perturb_variable_intrinsics(sc, 8)


def _system(monkeypatch, sc, radius, env=None, iterations=0):
    """(structure, reduced system, right-hand side, summary of an `iterations`-iteration solve or None) of a handle created under the switches of `env`"""
    from privacy_preserving_sfm_amd.device import BAProblem, ba_options
    with monkeypatch.context() as m:
        for k, v in (env or {}).items():
            m.setenv(k, v)
        pb = BAProblem(sc)
        try:
            st = pb.structure()
            S, rhs = pb.reduced_system(radius)
            s = pb.solve(ba_options(max_num_iterations=iterations)) if iterations else None
        finally:
            pb.close()
    return st, S, rhs, s


def _assert_system_is_the_oracles(oracle, sc, S, rhs, radius):
    ref = oracle.ba_reduced_system(sc, radius)
    cols = _var_cols(sc)
    assert len(cols) == ref["nc"], (len(cols), ref["nc"])
    # rtol 1e-8, atol 1e-10 of the largest entry: test_gpu_bundle_adjustment.test_camera_per_image_wide_blocks_equal_the_general_block_pairs
    scale = np.abs(ref["S"]).max()
    assert np.allclose(S[np.ix_(cols, cols)], ref["S"], rtol=1e-8, atol=1e-10 * scale)
    assert np.allclose(rhs[cols], ref["rhs"], rtol=1e-8, atol=1e-10 * np.abs(ref["rhs"]).max())


def test_camera_per_image_equal_widths_of_different_models_take_the_wide_path(oracle, monkeypatch):
    """24 images, each with a camera of its own, models PINHOLE / SIMPLE_RADIAL / SIMPLE_RADIAL_FISHEYE / OPENCV in turn, mask (b): n_v = 2 everywhere, at
    columns (0, 1) / (0, 3) / (0, 3) / (0, 7) of the camera Jacobian.  The intrinsics sit beside their image's pose columns and the 8-wide blocks come from the
    pose gather with wider rows; the system is the oracle's, and the one of the general block pairs (PPSFM_BA_INTR_WIDE=0) and of the tail layout
    (PPSFM_BA_INTR_LAYOUT=tail).  Constant poses in the middle and constant points as in the homogeneous test."""
    sc = _per_image_scene(24, 400, "pair", seed=9)
    sc["pose_const"] = sc["pose_const"].copy(); sc["pose_const"][[7, 13]] = 1
    sc["point_const"] = sc["point_const"].copy(); sc["point_const"][::37] = 1
    st, S, rhs, _ = _system(monkeypatch, sc, 1e3)
    assert st["private_intrinsics"] == 2 and st["wide_intrinsics"] == 2 and st["intrinsics_columns"] == 48, st
    assert S.shape[0] == 6 * 24 + 2 * 24
    _assert_system_is_the_oracles(oracle, sc, S, rhs, 1e3)
    st0, S0, rhs0, _ = _system(monkeypatch, sc, 1e3, {"PPSFM_BA_INTR_WIDE": "0"})
    assert st0["private_intrinsics"] == 2 and st0["wide_intrinsics"] == 0, st0
    stt, St, rhst, _ = _system(monkeypatch, sc, 1e3, {"PPSFM_BA_INTR_LAYOUT": "tail"})
    assert stt["private_intrinsics"] == 0 and stt["wide_intrinsics"] == 0, stt
    for Sx, rhsx in ((S0, rhs0), (St, rhst)):      # 1e-10 of the largest entry: test_camera_per_image_wide_blocks_equal_the_general_block_pairs
        assert np.abs(S - Sx).max() <= 1e-10 * np.abs(Sx).max() and np.abs(rhs - rhsx).max() <= 1e-10 * np.abs(rhsx).max()


@pytest.mark.parametrize("rule", ["widths", "even"])
def test_camera_per_image_unequal_widths_refuse_the_wide_path(oracle, monkeypatch, rule):
    """the same cameras with widths that differ - PrivateIntrinsicsColumns must answer 0, the intrinsics follow the pose columns, and the system is still the
    oracle's.  "widths" (mask (a)): the second image's width is odd and a later camera has none, which refuse by themselves; "even": 2 2 2 4 in turn, all even
    and none zero, so that the INEQUALITY (PINHOLE's 2 beside OPENCV's 4) is the only reason left to refuse."""
    sc = _per_image_scene(24, 400, rule, seed=9)
    nv = mm.num_variable(sc)
    assert (len(set(nv)) > 2 and 0 in nv) if rule == "widths" else (list(nv) == [2, 2, 2, 4] * 6)
    st, S, rhs, _ = _system(monkeypatch, sc, 1e3)
    assert st["private_intrinsics"] == 0 and st["wide_intrinsics"] == 0 and st["intrinsics_columns"] == int(mm.num_variable(sc).sum()), st
    _assert_system_is_the_oracles(oracle, sc, S, rhs, 1e3)


def test_camera_per_image_mixed_models_on_the_block_sparse_path(oracle, monkeypatch):
    """192 images of a sequence (window 8), a camera per image, the four models in turn, n_v = 2: the dissected several-chain factorisation sees 8-wide
    private blocks of mixed models.  No fallback, the dense natural-order system to 1e-9 relative (test_gpu_fuzz.
    test_random_sequence_and_collection_scenes_device_lists_equal_host_lists_and_the_dense_path), the oracle's solve to BASELINE's 1e-5."""
    from privacy_preserving_sfm_amd.device import BAProblem, ba_options
    sc = _per_image_scene(192, 2400, "pair", seed=10, window=8)
    st, S, rhs, s = _system(monkeypatch, sc, 1e3, iterations=3)
    assert st["block_sparse"] and st["chains"] >= 2 and st["private_intrinsics"] == 2 and st["wide_intrinsics"] == 2, st
    assert s.cholesky_fallbacks == 0 and s.linear_solver == 2
    std, Sd, rhsd, sd = _system(monkeypatch, sc, 1e3, {"PPSFM_BA_SPARSE": "0", "PPSFM_BA_ORDERING": "natural"}, iterations=3)
    assert not std["block_sparse"] and not std["reordered"], std
    assert _rel(S, Sd) <= 1e-9 and _rel(rhs, rhsd) <= 1e-9
    assert s.num_iterations == sd.num_iterations and s.num_successful_steps == sd.num_successful_steps
    _assert_system_is_the_oracles(oracle, sc, S, rhs, 1e3)
    pb = BAProblem(sc)
    try:
        s = pb.solve(ba_options(max_num_iterations=3))
        poses, points, intr = pb.get_parameters()
    finally:
        pb.close()
    rposes, rpoints, rintr, rs, _ = oracle.ba_solve(sc, oracle.BAOptionsC.defaults(max_num_iterations=3))
    assert s.num_iterations == rs.num_iterations and s.num_successful_steps == rs.num_successful_steps
    # 1e-5: test_sequence_scene_with_variable_intrinsics_takes_the_block_sparse_path
    assert _rel(points, rpoints) <= 1e-5 and _rel(poses, rposes) <= 1e-5 and _rel(intr, rintr) <= 1e-5


def _solve_scene(rule, loss, unused=()):
    sc = mm.perturb_variable_intrinsics(mm.mixed_ba_scene(22, 300, 4, seed=5, model=2, sort="point", rule=rule, unused=unused), 6)
    sc["loss_type"], sc["loss_scale"] = loss, 0.05
    return sc


def _assert_constants_kept_their_bits(sc, intr):
    start = np.asarray(sc["intr"])
    for k, m in enumerate(sc["camera_model"]):
        for j in range(12):
            if j >= synthetic.NUM_PARAMS[int(m)] or (int(sc["camera_const_mask"][k]) >> j) & 1:
                assert intr[k, j] == start[k, j], (k, j)      # a constant parameter, or padding behind the model's parameters


def _assert_parameters(sc, got, want):
    """1e-5: test_solve_with_variable_intrinsics_matches_oracle (poses absolute) - the intrinsics camera by camera, each row on its own scale"""
    (poses, points, intr), (rposes, rpoints, rintr) = got, want
    assert np.abs(points - rpoints).max() <= 1e-5 * np.abs(rpoints).max()
    assert np.abs(poses - rposes).max() <= 1e-5
    for k in range(len(intr)):
        assert np.abs(intr[k] - rintr[k]).max() <= 1e-5 * np.abs(rintr[k]).max(), (k, int(sc["camera_model"][k]), intr[k] - rintr[k])
    _assert_constants_kept_their_bits(sc, intr)
    assert np.array_equal(poses[0], sc["poses"][0]) and poses[1, 4] == sc["poses"][1, 4]      # the gauge did not move


def _oracle_is_stable(oracle, sc, options, want):
    """The ORACLE's own counts, parameters and cost trace under three 1e-12 perturbations of the start points (the criterion of test_gpu_fuzz._oracle_spread and
    of the refinement-loop tests): the scene may be judged at 1e-5 (parameters) and 1e-6 (costs) only where the oracle itself moves far less.  Computed from
    the oracle alone -> (largest relative movement of a parameter array, of a cost of the trace)."""
    rposes, rpoints, rintr, rs, rtrace = want
    spread, trace_spread = 0.0, 0.0
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        pert = dict(sc, points=np.asarray(sc["points"]) * (1.0 + 1e-12 * rng.uniform(-1, 1, size=np.shape(sc["points"]))))
        pposes, ppoints, pintr, ps, ptrace = oracle.ba_solve(pert, options())
        assert (ps.num_iterations, ps.num_successful_steps) == (rs.num_iterations, rs.num_successful_steps)
        spread = max(spread, _rel(ppoints, rpoints), _rel(pposes, rposes), _rel(pintr, rintr))
        trace_spread = max(trace_spread, float((np.abs(ptrace[:, 0] - rtrace[:, 0]) / np.maximum(rtrace[:, 0], 1e-300)).max()))
    return spread, trace_spread


@pytest.mark.parametrize("rule,loss,unused", [("widths", 0, ()), ("widths", 2, ()), ("focal", 0, (4,)), ("focal", 2, ())])
def test_direct_solve_with_mixed_widths_matches_oracle(oracle, rule, loss, unused):
    from privacy_preserving_sfm_amd.device import BAProblem, ba_options
    sc = _solve_scene(rule, loss, unused)
    options = lambda: oracle.BAOptionsC.defaults(max_num_iterations=8)
    rposes, rpoints, rintr, rs, rtrace = oracle.ba_solve(sc, options())
    spread, _ = _oracle_is_stable(oracle, sc, options, (rposes, rpoints, rintr, rs, rtrace))      # (the costs end at their rounding floor: the trace is compared with an absolute term below)
    assert spread <= 1e-7, spread
    pb = BAProblem(sc)
    s = pb.solve(ba_options(max_num_iterations=8))
    got = pb.get_parameters()
    trace = pb.trace()
    pb.close()
    print("direct %s loss %d: iterations %d / %d, successful %d / %d, cost %.3e -> %.3e / %.3e, oracle spread %.2e" % (
        rule, loss, s.num_iterations, rs.num_iterations, s.num_successful_steps, rs.num_successful_steps, s.initial_cost, s.final_cost, rs.final_cost, spread))
    assert s.linear_solver != 3 and s.cholesky_fallbacks == 0
    assert s.num_iterations == rs.num_iterations and s.num_successful_steps == rs.num_successful_steps
    # the first six rows, rtol 1e-6 / atol 1e-12, the same accept / reject flags: test_solve_with_variable_intrinsics_matches_oracle
    k = min(len(trace), len(rtrace), 6)
    assert np.allclose(trace[:k, 0], rtrace[:k, 0], rtol=1e-6, atol=1e-12)
    assert np.array_equal(trace[:k, 6], rtrace[:k, 6])
    assert s.final_cost < 1e-3 * s.initial_cost
    _assert_parameters(sc, got, (rposes, rpoints, rintr))


@pytest.mark.parametrize("rule,loss", [("widths", 0), ("widths", 2), ("focal", 0), ("focal", 2)])
def test_iterative_schur_with_mixed_widths_follows_the_oracle(oracle, rule, loss):
    """ITERATIVE_SCHUR + SCHUR_JACOBI with variable intrinsics: the operator's intrinsics part from per-observation Jacobians of per-camera width, one
    preconditioner block per camera of its own size (ba_pcg.hip k_pcg_cam_t / k_pcg_cam_q, k_pcg_intr_inverse).  With variable intrinsics PcgSolve always
    takes the four-launch form with the many-workgroup vector step: PPSFM_PCG_FUSED cannot change anything here and is not varied (the fused iteration runs
    on a mixed scene in test_iterative_schur_constant_intrinsics_on_both_vector_steps).
    Three LM iterations (16 to 20 conjugate-gradient iterations, a rejected step in the mask-(a) TRIVIAL case): the oracle's own inexact steps on weakly
    determined intrinsics soon move with its input's twelfth digit - under a 1e-12 perturbation of the start points its parameters after 8 iterations move by
    up to 4e-4, its cost of iteration 5 by 2.3e-5 and of iteration 4 by 3.4e-7, more than or too close to the 1e-6 the costs are compared at; up to iteration 3
    by 2.5e-9 (asserted below 1e-8, the parameters below 1e-7, before anything is judged).  Pixel noise on the lines (0.5 and 1 px, a cost floor far above
    rounding) does not help: over 8 iterations the oracle's parameters then move by 2e-8 to 3e0 and its costs by 2e-7 to 1e2 under the same perturbation."""
    from privacy_preserving_sfm_amd.device import BAProblem, ba_options
    sc = _solve_scene(rule, loss)
    options = lambda: oracle.BAOptionsC.defaults(max_num_iterations=3, iterative_schur=1)
    ref = oracle.ba_solve(sc, options())
    rposes, rpoints, rintr, rs, rtrace = ref
    spread, trace_spread = _oracle_is_stable(oracle, sc, options, ref)
    assert spread <= 1e-7 and trace_spread <= 1e-8, (spread, trace_spread)
    pb = BAProblem(sc, linear_solver=2)
    try:
        assert pb.structure()["iterative"] and pb.structure()["intrinsics_columns"] == int(mm.num_variable(sc).sum())
        s = pb.solve(ba_options(max_num_iterations=3))
        got = pb.get_parameters()
        trace = pb.trace()
    finally:
        pb.close()
    print("iterative %s loss %d: successful %d / %d, CG %d / %d, cost %.3e -> %.3e / %.3e, oracle spread %.2e / %.2e" % (
        rule, loss, s.num_successful_steps, rs.num_successful_steps, s.linear_solver_iterations, rs.linear_solver_iterations, s.initial_cost, s.final_cost, rs.final_cost, spread, trace_spread))
    # counts, +-3 conjugate-gradient iterations, the cost per iteration to 1e-6: test_iterative_schur_with_variable_intrinsics_follows_the_oracle
    assert s.linear_solver == 3 and s.linear_solver_iterations > 0
    assert s.num_iterations == rs.num_iterations == 3 and s.num_successful_steps == rs.num_successful_steps
    assert abs(s.linear_solver_iterations - rs.linear_solver_iterations) <= 3
    assert np.allclose(trace[:, 0], rtrace[:, 0], rtol=1e-6, atol=1e-18)
    _assert_parameters(sc, got, (rposes, rpoints, rintr))


_CONSTANT_INTRINSICS_REFERENCE = {}


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("loss", [0, 2])
def test_iterative_schur_constant_intrinsics_on_both_vector_steps(oracle, monkeypatch, loss, fused):
    """All eleven models with every intrinsic parameter constant (NI = 0): the only iterative configuration in which PPSFM_PCG_FUSED chooses - the fused
    three-launch iteration (PcgFusedRun, the default) or the two-launch many-workgroup vector step - and both run here on records K1 wrote for eleven models
    in point order.  Seven LM iterations, counts, conjugate-gradient counts within 2, costs to 1e-6, parameters to 1e-5: the figures and bars of
    test_gpu_bundle_adjustment.test_iterative_schur_pcg_follows_the_oracle.  The lines carry 0.5 px of noise: the cost stays five orders above its rounding
    floor, and the oracle's own parameters / costs move by 4e-14 / 5e-12 (TRIVIAL) and 2e-9 / 7e-10 (CAUCHY) under a 1e-12 perturbation (asserted below
    1e-7 / 1e-8 first)."""
    from privacy_preserving_sfm_amd.device import BAProblem, ba_options
    monkeypatch.setenv("PPSFM_PCG_FUSED", fused)
    sc = mm.mixed_ba_scene(22, 300, 4, seed=5, model=2, sort="point", line_noise_px=0.5)
    sc["loss_type"], sc["loss_scale"] = loss, 0.05
    assert (sc["camera_const_mask"] == 0xFFFF).all()
    options = lambda: oracle.BAOptionsC.defaults(max_num_iterations=7, iterative_schur=1)
    if loss not in _CONSTANT_INTRINSICS_REFERENCE:      # (computed once, shared by both forms of the vector step, never modified)
        ref = oracle.ba_solve(sc, options())
        _CONSTANT_INTRINSICS_REFERENCE[loss] = ref + _oracle_is_stable(oracle, sc, options, ref)
    rposes, rpoints, rintr, rs, rtrace, spread, trace_spread = _CONSTANT_INTRINSICS_REFERENCE[loss]
    assert spread <= 1e-7 and trace_spread <= 1e-8, (spread, trace_spread)
    pb = BAProblem(sc, linear_solver=2)
    try:
        st = pb.structure()
        assert st["iterative"] and st["intrinsics_columns"] == 0
        s = pb.solve(ba_options(max_num_iterations=7))
        poses, points, intr = pb.get_parameters()
        trace = pb.trace()
    finally:
        pb.close()
    print("iterative NI = 0 loss %d fused %s: successful %d / %d, CG %d / %d, cost %.3e -> %.3e / %.3e, oracle spread %.2e / %.2e" % (
        loss, fused, s.num_successful_steps, rs.num_successful_steps, s.linear_solver_iterations, rs.linear_solver_iterations, s.initial_cost, s.final_cost, rs.final_cost, spread, trace_spread))
    assert s.linear_solver == 3 and s.linear_solver_iterations > 0
    assert s.num_iterations == rs.num_iterations == 7 and s.num_successful_steps == rs.num_successful_steps
    assert abs(s.linear_solver_iterations - rs.linear_solver_iterations) <= 2
    assert np.allclose(trace[:, 0], rtrace[:, 0], rtol=1e-6, atol=1e-18)
    assert np.abs(points - rpoints).max() <= 1e-5 * np.abs(rpoints).max() and np.abs(poses - rposes).max() <= 1e-5 * np.abs(rposes).max()
    assert np.array_equal(intr, sc["intr"]) and np.array_equal(poses[0], sc["poses"][0]) and poses[1, 4] == sc["poses"][1, 4]


def test_covariance_with_mixed_widths_against_the_host_references(oracle):
    """pp_ba_covariance on a mask-(a) scene: every pose pair and every point against the dense inverse, at the bar of test_gpu_covariance (_judge: max(4 e_LAPACK,
    kappa sqrt(n) u), kappa < 1e10, bar < 1e-5 asserted before judging).  The call returns no intrinsics blocks of their own; the intrinsics stay in S, and a
    point's block is formed through its observing cameras' intrinsics columns, each at its own width (ba_covariance.hip).  Eight observations per point: with
    four, the higher-order distortion terms of the wide models put kappa(S_scaled) at 1.2e10, outside what that bar may judge (host figures: 4.2e9 here)."""
    from test_gpu_covariance import _all_pairs, _judge
    import covariance_reference as cr
    from privacy_preserving_sfm_amd.device import BAProblem
    sc = mm.mixed_ba_scene(22, 300, 8, seed=5, model=2, sort="point", rule="widths")
    pairs, points = _all_pairs(22), list(range(300))
    pb = BAProblem(sc, device=0)
    pc, xc, info = pb.covariance(pairs, points, return_info=True)
    pb.close()
    assert info.n == 6 * 22 + int(mm.num_variable(sc).sum())
    _judge("mixed models, mask (a)", cr.dense_covariance(sc), cr.SchurCovariance(sc), pc, pairs, xc, points)


def _filter_scene(seed):
    """test_gpu_bundle_adjustment._filter_scene with 7 cameras of 7 models and image sizes that differ per camera: the narrow ones cut projections the wide
    ones keep"""
    sc = mm.mixed_ba_scene(14, 600, 6, models=TRACK_MODELS, seed=seed, model=2, noise_point=0.0, noise_q=0.0, noise_t=0.0)
    rng = np.random.default_rng(seed)
    M = len(sc["obs_pose"])
    lines = sc["lines"].copy()
    bad = rng.choice(M, M // 12, replace=False)
    lines[bad, 2] += rng.normal(0, 0.02, len(bad))                 # corrupted line offsets -> large pixel error
    sc["lines"] = lines
    pts = sc["points"].copy()
    pts[:12] *= 40.0                                               # far points: small triangulation angles
    pts[12:20] = -pts[12:20] - np.array([0, 0, 12.0])              # behind the cameras
    sc["points"] = pts
    aligned = rng.random(M) < 0.5
    aligned[np.isin(sc["obs_point"], np.arange(20, 30))] = True    # tracks with aligned lines only
    cam_size = np.array([[2200, 1800], [1000, 850], [1800, 1500], [950, 800], [2000, 1700], [900, 900], [1600, 1300]], dtype=np.int32)
    return sc, aligned, cam_size


@pytest.mark.parametrize("seed,max_err,min_ang,subset", [(1, 4.0, 1.5, False), (2, 1.0, 0.5, True)])
def test_filters_with_mixed_models_match_oracle(oracle, seed, max_err, min_ang, subset):
    """shape and exact-equality assertions of test_gpu_bundle_adjustment.test_filter_points3d_matches_oracle; ba_filter.hip reads camera_model[k],
    intr + kCamStride k and cam_size + 2 k per observation"""
    from privacy_preserving_sfm_amd.device import BAProblem
    sc, aligned, cam_size = _filter_scene(seed)
    sub = (np.arange(600) % 3 != 0) if subset else None
    rnf, rod, rpd, rpe = oracle.filter_points3d(sc, max_err, min_ang, cam_size, aligned, sub)
    # the rows matter: with every camera given the first camera's size the oracle itself decides otherwise
    _, rod0, rpd0, _ = oracle.filter_points3d(sc, max_err, min_ang, np.tile(cam_size[:1], (7, 1)), aligned, sub)
    assert not np.array_equal(rod, rod0) and not np.array_equal(rpd, rpd0)
    pb = BAProblem(sc)
    rep, od, pd, pe = pb.filter_points(max_err, min_ang, cam_size, obs_aligned=aligned, point_subset=sub)
    assert rep.num_filtered == rnf and np.array_equal(od, rod) and np.array_equal(pd, rpd)
    assert np.allclose(pe, rpe, rtol=1e-9, atol=1e-12)
    assert rep.num_points_deleted == int(rpd.sum()) and rep.num_observations_deleted == int(rod.sum())
    # every rule fires somewhere in this scene
    assert rpd.sum() > 20 and (~rpd).sum() > 100 and (rod & ~rpd[sc["obs_point"]]).sum() > 10
    n, neg = pb.filter_negative_depth()
    rn, rneg = oracle.filter_negative_depth(sc)
    assert n == rn and np.array_equal(neg, rneg) and n >= 8 * 6
    pb.close()


@pytest.mark.parametrize("residual_type,max_error,min_angle", [(0, 2e-3, 0.0), (1, 2.0, 0.02)])
def test_triangulate_tracks_with_mixed_models_matches_oracle(oracle, residual_type, max_error, min_angle):
    """14 views on 7 cameras of 7 models (view v -> camera v % 7), 400 tracks: agreement shares and point tolerances of
    test_gpu_triangulation.test_triangulate_tracks_matches_oracle; its counts (800 decided, 300 clean of 1500 tracks) scaled by 400 / 1500 - the oracle alone
    decides 339 / 335 and finds 289 / 292 clean ones here.  A statistical comparison; every model alone and all eleven in one call are held exactly to a
    50-digit reference in tests/test_gpu_triangulation_exact.py (the `models` set)"""
    from privacy_preserving_sfm_amd.device import triangulate_tracks, triangulation_options
    sc = mm.mix_track_scene(synthetic.make_track_scene(14, 400, seed=3 + residual_type), TRACK_MODELS)
    opt = triangulation_options(min_tri_angle=min_angle, residual_type=residual_type, max_error=max_error, confidence=0.9999, min_inlier_ratio=0.02)
    ok, xyz, mask, nt, ms = triangulate_tracks(sc["track_start"], sc["lines"], sc["obs_view"], sc["P"], sc["centers"], sc["view_camera"], sc["camera_model"],
                                               sc["intr"], sc["cam_size"], opt)
    rok, rxyz, rmask, rnt = oracle.triangulate_tracks(sc, min_angle, residual_type, max_error=max_error, confidence=0.9999, min_inlier_ratio=0.02)
    agree = (ok == rok)
    assert agree.mean() >= 0.995, agree.mean()
    both = ok & rok
    same_trials = (nt == rnt)[both].mean()
    assert same_trials >= 0.99, same_trials
    ts = sc["track_start"]
    ninl = np.array([mask[ts[t]:ts[t + 1]].sum() for t in range(len(ts) - 1)])
    rinl = np.array([rmask[ts[t]:ts[t + 1]].sum() for t in range(len(ts) - 1)])
    assert (rok & (rinl >= 4)).sum() >= 330                       # the oracle's own count (339 / 335), well above the floor below
    decided = np.nonzero(both & (ninl >= 4) & (rinl >= 4))[0]
    assert len(decided) > 800 * 400 // 1500
    same_mask = np.array([np.array_equal(mask[ts[t]:ts[t + 1]], rmask[ts[t]:ts[t + 1]]) for t in decided])
    assert same_mask.mean() >= 0.999, same_mask.mean()
    assert (ninl[both] == rinl[both]).mean() >= 0.995
    good = decided[same_mask]
    err = np.abs(xyz[good] - rxyz[good]).max(axis=1)
    assert np.mean(err < 1e-8) >= 0.99 and np.median(err) < 1e-11
    clean = np.array([(~sc["is_outlier"][ts[t]:ts[t + 1]]).sum() for t in range(len(ts) - 1)])
    sel = ok & (clean >= 5)
    assert sel.sum() > 300 * 400 // 1500
    assert np.median(np.linalg.norm(xyz[sel] - sc["points"][sel], axis=1)) < 5e-3
    if min_angle == 0.0:
        assert ok[clean >= 5].mean() > 0.95
    for t in np.nonzero(~ok)[0][:50]:
        assert not mask[ts[t]:ts[t + 1]].any()
    # every model decides tracks: each camera is the view of inlier observations
    cam_of_obs = sc["view_camera"][sc["obs_view"]]
    assert all(mask[cam_of_obs == k].sum() > 50 for k in range(7))


def test_tracks_complete_and_merge_with_mixed_models_equal_the_oracle(oracle):
    """test_gpu_tracks' smallest scene (20 images, 150 points, 10 observations, seed 1, quiet start) on 5 cameras of 5 models with image sizes that differ:
    the same pairs in the same order, the same merges, the same final state as tests/tracks_reference.py (exact; oracle margin 4.5e-2, asserted above 1e-6)"""
    from test_gpu_tracks import QUIET, _compare
    from privacy_preserving_sfm_amd.incremental_triangulator import reconstruction_from_completion_scene
    sc = synthetic.make_completion_scene(20, 150, 10, seed=1, num_intrinsics=5, **QUIET)
    sc = mm.mix_camera_models(sc, [2, 4, 7, 9, 10])
    sc["cam_size"] = np.array([[1280 + 16 * k, 960 + 12 * k] for k in range(5)], dtype=np.int32)
    reports, o = _compare(reconstruction_from_completion_scene(sc), "cm")
    assert len(o.completed) > 100 and len(o.merged) > 10
    assert all(r.candidates_evaluated > 0 for r in reports)


def test_random_small_scenes_with_mixed_models(oracle):
    """fuzz_scenes.reduced_system_case(7, k, mixed=True) for eight k - fixed (1), shared (0, 2, 4, 6) and per-image (17, 23, 31) intrinsics; dense, window,
    loop and cluster co-visibility -: the random small scenes of test_gpu_fuzz with their cameras re-labelled to random models and a random constant mask
    per camera, through the same check (test_gpu_fuzz._check_case: system 1e-8, cost trace, parameters 1e-5 or explained by the oracle's
    own spread)"""
    from test_gpu_fuzz import _check_case
    from privacy_preserving_sfm_amd.device import camera_num_params
    ran, models = 0, set()
    for case in (0, 1, 2, 4, 6, 17, 23, 31):
        sc, m = fuzz_scenes.reduced_system_case(7, case, camera_num_params, mixed=True)
        assert sc is not None
        ran += 1
        models |= set(m["model"])
        _check_case(oracle, sc, m, (case, m))
    assert ran == 8 and len(models) == 11
