"""The work buffers of the three estimator handles (csrc/init_solvers.hip) grow with the calls made on them: what a handle answers does not depend on
what it was asked before.  For each handle: A, fresh, makes the large call; B makes a small call first (one model or sample, minimal sample size) and
then the same large call (300 models or samples - more than one workgroup, above the planar floor of 64 - and a larger sample size): equal outputs,
element for element, NaN equal to NaN.  Then LO-MSAC on B and on a fresh handle C: the same counters, inlier indices and model bits."""
import numpy as np
import pytest

from privacy_preserving_sfm_amd import synthetic

pytestmark = pytest.mark.gpu

NUM = 300
COUNTERS = ("num_iterations", "best_num_inliers", "best_model_score", "inlier_ratio", "number_lo_iterations", "num_inlier_indices", "hypotheses_evaluated")


def _samples(rng, n, num, m):
    return np.stack([rng.choice(n, m, replace=False) for _ in range(num)]).astype(np.int32)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        assert np.array_equal(g, w, equal_nan=True) if g.dtype.kind == "f" else np.array_equal(g, w)


def _same_lomsac(got, want):
    """(report, model arrays ..., inlier indices) of two runs: counters, indices, and the models bit for bit"""
    for name in COUNTERS:
        assert getattr(got[0], name) == getattr(want[0], name), name
    assert np.array_equal(got[-1], want[-1])
    for g, w in zip(got[1:-1], want[1:-1]):
        assert np.array_equal(np.ascontiguousarray(g).view(np.int64), np.ascontiguousarray(w).view(np.int64))


def _close_twice(*handles):
    for h in handles:
        h.close()
        h.close()


def test_planar_handle_grows_without_changing_answers():
    from privacy_preserving_sfm_amd.device import PlanarOffsetProblem, lomsac_options
    n = 20
    sc = synthetic.make_planar_offset_scene(n, n_outliers=0, seed=7, noise=0.0)
    rng = np.random.default_rng(0)
    small, large = _samples(rng, n, 1, 3), _samples(rng, n, NUM, 20)
    models = sc["t_gt"][None] + 0.05 * rng.normal(size=(NUM, 3))
    models[17] = np.nan
    thr = 0.005

    def large_call(pp):
        return (pp.solve_batch(large),) + pp.score(models, thr)

    a, b, c = (PlanarOffsetProblem(sc["poses"], sc["lines"], sc["Rg"]) for _ in range(3))
    want = large_call(a)
    assert np.isfinite(want[0]).all() and np.isnan(want[1][17]) and want[2].max() > 0
    b.solve_batch(small)
    b.score(models[:1], thr)
    _same(large_call(b), want)
    opt = lomsac_options(squared_inlier_threshold=0.005 * 0.005)
    _same_lomsac(b.lomsac(opt), c.lomsac(opt))
    _close_twice(a, b, c)


def test_pose2d_handle_grows_without_changing_answers():
    from privacy_preserving_sfm_amd.device import Pose2dProblem, lomsac_options
    n = 10
    sc = synthetic.make_scene_2d(4, n, seed=3)
    rng = np.random.default_rng(1)
    small, large = _samples(rng, n, 1, 3), _samples(rng, n, NUM, 6)
    models = sc["cams"][1][None] + 0.05 * rng.normal(size=(NUM, 2, 3))
    models[17] = np.nan
    thr = 1e-3

    def large_call(pp):
        return (pp.solve_batch(large),) + pp.score(models, thr)

    a, b, c = (Pose2dProblem(sc["x"][1], sc["X"]) for _ in range(3))
    want = large_call(a)
    assert np.isfinite(want[0]).all() and np.isnan(want[1][17]) and want[2].max() > 0
    b.solve_batch(small)
    b.score(models[:1], thr)
    _same(large_call(b), want)
    opt = lomsac_options(squared_inlier_threshold=1.0)
    _same_lomsac(b.lomsac(opt), c.lomsac(opt))
    _close_twice(a, b, c)


def test_fourview2d_handle_grows_without_changing_answers():
    from privacy_preserving_sfm_amd.device import FourView2dProblem, lomsac_options
    n = 100
    sc = synthetic.make_scene_2d(4, n, n_outliers=20, seed=6)
    rng = np.random.default_rng(2)
    small, large = _samples(rng, n, 1, 5), _samples(rng, n, NUM, 10)
    models = sc["cams"][None] + 0.05 * rng.normal(size=(NUM, 4, 2, 3))
    models[17] = np.nan
    thr = 1e-3

    def large_call(fv):
        return fv.minimal_batch(large) + fv.nonminimal_batch(large, thr) + fv.score(models, thr)

    a, b, c = (FourView2dProblem(sc["x"]) for _ in range(3))
    want = large_call(a)
    assert want[1].max() > 0 and np.isnan(want[5][17]) and want[6].max() > 0
    b.minimal_batch(small)
    b.nonminimal_batch(small, thr)
    b.score(models[:1], thr)
    _same(large_call(b), want)
    opt = lomsac_options(squared_inlier_threshold=1e-7, min_num_iterations=256, max_num_iterations=256)
    _same_lomsac(b.lomsac(opt), c.lomsac(opt))
    _close_twice(a, b, c)
