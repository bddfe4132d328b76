"""Device against oracle on NOISY bundle adjustment problems, run to termination (reference src/optim/bundle_adjustment.cc:260-320; presets
src/controllers/incremental_mapper.cc:95-97, 196-243).

Every scene has the same observation model: 0.5 px line noise, 5 % outlier observations, float32-stored lines (refinement_oracle.NOISY).
Set-ups: cfg 1 (20 images) and cfg 2 (100 images) under the TRIVIAL loss to convergence (Ceres' default tolerances: function 1e-6,
gradient 1e-10, parameter 1e-8, at most 100 iterations); cfg 1 and cfg 2 under the local preset (a SOFT_L1 solve, then a TRIVIAL solve
from its result; gradient tolerance 10, at most 25 iterations each); cfg 3 (500 images, 200k observations) under the global preset
(gradient tolerance 1, at most 50 iterations).

Asserted per set-up: termination type, iteration count and accept / reject pattern equal to the oracle's; cost trace within 1e-6
relative; parameters within 1e-5 relative - a parameter that misses may pass if it is within 20 x what the ORACLE itself moves under a
1e-12 perturbation of its input (tests/test_gpu_fuzz.py's rule), at most 1 % of the parameters may; the final cost is at least 1e3 x the
exact scene's.  The cfg-2 set-ups also assert a rejected step in the oracle's own trace.

Seeds: chosen on the CPU so that the ORACLE is reproducible on them - run with its input points perturbed by 1e-12 relative (three
perturbations), the share of its parameters that move by more than 1e-5 stays under the 1 % cap.  Most seeds are not: with 5 % gross outliers
(338 px rms) under a TRIVIAL loss the oracle rejects a quarter to a half of its steps, and on 37 of 41 seeds tried at cfg 1 (0x12c..0x154) its end
point moves in 4-93 % of the parameters.  Measured for the seeds below (largest movement; shares):
  cfg 1 TRIVIAL 0x134: 80 iterations, 12 rejected, CONVERGENCE; 1.3e-5; 0.1 % / 0.1 % / 0.1 %
  cfg 2 TRIVIAL 0x190: 39 iterations, 6 rejected, CONVERGENCE; 3.2e-11; 0 / 0 / 0
  cfg 1 local   0x68:  25 + 25 iterations, 0 + 13 rejected; 2.4e-8; 0 / 0 / 0
  cfg 2 local   0x1f4: 25 + 25 iterations, 0 + 5 rejected; 7.3e-6; 0 / 0 / 0
  cfg 3 global  0xC0FFF1: 50 iterations, 17 rejected, NO_CONVERGENCE; one perturbation (an oracle run takes one to four minutes): the same accept / reject
                          pattern, 4.9e-8; 0.  On the device it matched the oracle to 2.2e-9 and 2.5e-9 relative in two runs, in 41 ms (47 ms with
                          the handle's creation).

A defect these scenes found (fixed in pp_ba_solve): when the factorisation of the reduced system met a non-positive pivot, the NaN it left in the
zero padding of S - which the assembly never rewrites - made every later, more strongly damped system fail too; a solve of the noisy cfg-2 scene ended
with "10 consecutive invalid steps" at a radius of 2.5e-8 where the oracle recovered after two.  The system is now cleared after such a step.

"1e-5 relative" is the project's array-norm bound (tests/test_gpu_baseline_sizes.py `_rel`): |a - b| of every parameter over the largest magnitude of its
array - the poses (quaternions and translations together, largest entry about 4) and the points (about 1) - so a small parameter is held to about
1e-5 absolute, not to 1e-5 of itself.
"""
import time

import numpy as np
import pytest

import refinement_oracle
from privacy_preserving_sfm_amd import synthetic

pytestmark = pytest.mark.gpu

CFG = {1: (20, 500, 4), 2: (100, 5000, 8), 3: (500, 25000, 8)}
TRIVIAL, SOFT_L1 = 0, 1
CONVERGENCE = dict(max_num_iterations=100, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8)
LOCAL = dict(max_num_iterations=25, function_tolerance=0.0, gradient_tolerance=10.0, parameter_tolerance=0.0, max_linear_solver_iterations=100)
GLOBAL = dict(max_num_iterations=50, function_tolerance=0.0, gradient_tolerance=1.0, parameter_tolerance=0.0, max_linear_solver_iterations=100)
STAGES = {"trivial": [(TRIVIAL, CONVERGENCE)], "local": [(SOFT_L1, LOCAL), (TRIVIAL, LOCAL)], "global": [(TRIVIAL, GLOBAL)]}


def _rel_each(a, b):
    return np.abs(a - b) / np.abs(b).max()


def _oracle_run(oracle, sc, stages):
    cur, out = dict(sc), []
    for loss, kw in stages:
        cur = dict(cur, loss_type=loss, loss_scale=1.0)
        poses, points, _, s, trace = oracle.ba_solve(cur, oracle.BAOptionsC.defaults(**kw), trace_cap=512)
        out.append((s, trace))
        cur = dict(cur, poses=poses, points=points)
    return cur["poses"], cur["points"], out


def _device_run(sc, stages):
    from privacy_preserving_sfm_amd.device import BAProblem, ba_options
    cur, out = dict(sc), []
    for loss, kw in stages:
        cur = dict(cur, loss_type=loss, loss_scale=1.0)
        pb = BAProblem(cur)
        try:
            s = pb.solve(ba_options(**kw))
            poses, points, _ = pb.get_parameters()
            out.append((s, pb.trace().copy()))
        finally:
            pb.close()
        cur = dict(cur, poses=poses, points=points)
    return cur["poses"], cur["points"], out


def _oracle_spread(oracle, sc, stages, ref_poses, ref_points):
    spread = 0.0
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        pert = dict(sc, points=np.asarray(sc["points"]) * (1.0 + 1e-12 * rng.uniform(-1, 1, size=np.shape(sc["points"]))))
        pposes, ppoints, _ = _oracle_run(oracle, pert, stages)
        spread = max(spread, _rel_each(pposes, ref_poses).max(), _rel_each(ppoints, ref_points).max())
    return spread


@pytest.mark.parametrize("cfg,preset,seed", [(1, "trivial", 0x134), (2, "trivial", 0x190), (1, "local", 0x68), (2, "local", 0x1F4), (3, "global", 0xC0FFEE + 3)])
def test_noisy_scene_to_termination_matches_oracle(oracle, cfg, preset, seed):
    C, P, track = CFG[cfg]
    stages = STAGES[preset]
    sc = synthetic.make_ba_scene(C, P, track, seed=seed, model=2, **refinement_oracle.NOISY)
    t0 = time.time()
    poses, points, dev = _device_run(sc, stages)
    wall = time.time() - t0
    rposes, rpoints, ref = _oracle_run(oracle, sc, stages)
    for k, ((s, trace), (rs, rtrace)) in enumerate(zip(dev, ref)):
        print("cfg %d %s stage %d: device %d iterations (%d rejected), termination %d, cost %.9g -> %.9g, solve %.3f s | oracle %d iterations (%d rejected), termination %d, "
              "cost -> %.9g" % (cfg, preset, k, s.num_iterations, s.num_unsuccessful_steps, s.termination, s.initial_cost, s.final_cost, s.total_time_s, rs.num_iterations,
                                rs.num_unsuccessful_steps, rs.termination, rs.final_cost))
    print("cfg %d %s: device wall time %.3f s (handle creation included)" % (cfg, preset, wall))
    if cfg == 2:
        assert any((rtrace[1:, 6] == 0).any() for _, rtrace in ref), "the oracle's own trace must contain a rejected step"
    for (s, trace), (rs, rtrace) in zip(dev, ref):
        assert s.termination == rs.termination
        assert s.num_iterations == rs.num_iterations
        assert len(trace) == len(rtrace) and np.array_equal(trace[:, 6], rtrace[:, 6])                 # accept / reject pattern
        assert np.allclose(trace[:, 0], rtrace[:, 0], rtol=1e-6, atol=0.0)                              # cost trace
    err = np.concatenate([_rel_each(poses, rposes).ravel(), _rel_each(points, rpoints).ravel()])
    missed = err > 1e-5
    print("cfg %d %s: largest parameter difference %.3g relative, %d of %d parameters over 1e-5" % (cfg, preset, err.max(), int(missed.sum()), err.size))
    if missed.any():
        spread = _oracle_spread(oracle, sc, stages, rposes, rpoints)
        print("cfg %d %s: the oracle itself moves %.3g under a 1e-12 perturbation" % (cfg, preset, spread))
        assert (err[missed] <= 20.0 * spread).all(), (err.max(), spread)
        assert missed.mean() <= 0.01, missed.mean()
    # the generator did not silently produce exact data
    exact = synthetic.make_ba_scene(C, P, track, seed=seed, model=2)
    _, _, dev_exact = _device_run(exact, stages)
    assert dev[-1][0].final_cost >= 1e3 * dev_exact[-1][0].final_cost


def test_solve_recovers_after_a_factorisation_that_met_a_non_positive_pivot(oracle):
    """The noisy cfg-2 scene of seed 0xC0FFF0 under the global preset: at iteration 20 the reduced system is not positive definite (radius 8.8e5; the oracle
    meets invalid steps there too).  The step is invalid, the radius shrinks, and the next systems - ever more strongly damped - must factorise again: before
    the fix every one of them failed on the NaN the first had left in the padding of S, down to a radius of 2.5e-8, and the solve ended in FAILURE at
    iteration 28.  (On this seed the oracle itself is not reproducible to 1e-5: the trajectories are compared over the first ten iterations only.)"""
    from privacy_preserving_sfm_amd.device import BAProblem, ba_options
    sc = synthetic.make_ba_scene(100, 5000, 8, seed=0xC0FFEE + 2, model=2, **refinement_oracle.NOISY)
    pb = BAProblem(sc)
    s = pb.solve(ba_options(**GLOBAL))           # (a FAILURE raises)
    trace = pb.trace().copy()
    pb.close()
    _, _, _, rs, rtrace = oracle.ba_solve(sc, oracle.BAOptionsC.defaults(**GLOBAL))
    invalid = np.flatnonzero((trace[1:, 6] == 0) & (trace[1:, 3] == 0)) + 1           # rejected without a step: the linear solve failed
    assert len(invalid) >= 1
    first = int(invalid[0])
    # (the oracle's own trajectory on this seed depends on the machine it runs on from about iteration 14: only the first ten iterations are compared)
    assert first > 10 and np.array_equal(trace[:11, 6], rtrace[:11, 6]) and np.allclose(trace[:11, 0], rtrace[:11, 0], rtol=1e-6)
    assert (trace[first:, 6] == 1).any()                                               # a later step was accepted ...
    assert s.final_cost < trace[first, 0]                                              # ... and the cost went on falling
    assert s.termination == rs.termination == 1 and s.num_iterations == rs.num_iterations == 50


def test_noisy_scene_on_the_iterative_solver_runs_to_termination(oracle):
    """The same noisy cfg-2 scene with linear_solver = ITERATIVE_SCHUR under the global preset: an iterative handle has no N x N system, and its
    conjugate-gradient loop reports a failed solve with the same flag bit as a failed pivot - the clear after an invalid step must leave it alone.
    The solve ends by the loop's own rules (no HIP error, no FAILURE), on conjugate gradients, with a falling cost; the direct solve of the same
    scene ends within 1 % of its final cost (inexact steps: another trajectory on a scene where the oracle itself is not reproducible)."""
    from privacy_preserving_sfm_amd.device import BAProblem, ba_options
    sc = synthetic.make_ba_scene(100, 5000, 8, seed=0xC0FFEE + 2, model=2, **refinement_oracle.NOISY)
    out = {}
    for solver in (2, 1):
        pb = BAProblem(sc, linear_solver=solver)
        s = pb.solve(ba_options(**GLOBAL))
        out[solver] = (s, pb.trace().copy())
        pb.close()
    s, trace = out[2]
    print("iterative: %d iterations (%d rejected), termination %d, %d CG iterations, cost %.9g -> %.9g; direct -> %.9g" % (
        s.num_iterations, s.num_unsuccessful_steps, s.termination, s.linear_solver_iterations, s.initial_cost, s.final_cost, out[1][0].final_cost))
    assert s.linear_solver == 3 and s.linear_solver_iterations > 0
    assert s.termination in (0, 1) and s.num_iterations <= 50
    assert (np.diff(trace[:, 0]) <= 0).all() and s.final_cost < 0.7 * s.initial_cost
    assert abs(s.final_cost - out[1][0].final_cost) <= 1e-2 * out[1][0].final_cost
