"""K4/K5 + RANSAC driver parity vs the oracle.

L0  scoring / inlier masks: BIT-identical (integer counts, residual bits) for identical model bits.
L1  P6L/re3q3 solver: poses within 1e-9 relative of the oracle's (different root finder: Aberth vs
    companion-matrix QR), and the reference's own re3q3 properties (lib/re3q3/test_re3q3.cpp).
L2  end-to-end RANSAC: same num_trials, same winning trial, identical inlier set.
"""
import numpy as np
import pytest

from privacy_preserving_sfm_amd import synthetic

pytestmark = pytest.mark.gpu


def _mons(s):
    x, y, z = s
    return np.array([x * x, x * y, x * z, y * y, y * z, z * z, x, y, z, 1.0])


def test_residuals_bit_exact(oracle):
    from privacy_preserving_sfm_amd.device import PoseProblem
    sc = synthetic.make_ransac_scene(5000, seed=3)
    pp = PoseProblem(sc["lines"], sc["points"], sc["aligned"])
    rng = np.random.default_rng(0)
    models = np.stack([sc["gt_pose"] + rng.normal(0, s, (3, 4)) for s in (0, 1e-3, 1e-2, 0.1, 1.0)])
    models[4, 2] *= -1
    got = pp.residuals(models)
    for m in range(len(models)):
        want = oracle.line_residuals(sc["lines"], sc["points"], models[m])
        assert np.array_equal(got[m].view(np.uint64), want.view(np.uint64))
    # counts exact for three thresholds; tree sum close to (not bitwise equal to) the sequential sum;
    # the sequential kernel is bitwise equal
    for thr in (1e-6, sc["max_error"] ** 2, 1e-2):
        inl, sums = pp.score(models, thr)
        inl_s, sums_s = pp.score(models, thr, sequential=True)
        for m in range(len(models)):
            want = oracle.line_residuals(sc["lines"], sc["points"], models[m])
            n, s = oracle.support(want, thr)
            assert inl[m] == n == inl_s[m]
            assert sums_s[m] == s
            assert abs(sums[m] - s) <= 1e-12 * max(s, 1e-300)
    pp.close()


def _tree_support(res, thr):
    """the scoring kernel's fixed summation order: lane l adds the inlier residuals l, l+64, ... in index
    order, then a 64-lane xor butterfly (32, 16, ..., 1)"""
    n = len(res)
    pad = (-n) % 64
    r = np.concatenate([res, np.full(pad, np.inf)]).reshape(-1, 64)
    acc = np.zeros(64)
    for row in r:
        acc = acc + np.where(row <= thr, row, 0.0)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[np.arange(64) ^ off]
    return int((res <= thr).sum()), acc[0]


def test_score_tree_sum_bitwise(oracle):
    """pp_pose_score runs the RANSAC scoring kernel (reciprocal without the division's range scaling, predicate
    in scalar registers, sum under EXEC): counts AND the fixed-order sum are bitwise those of the IEEE-division
    residuals (which are bitwise the oracle's, test above)."""
    from privacy_preserving_sfm_amd.device import PoseProblem
    sc = synthetic.make_ransac_scene(5000 + 37, seed=11)
    pp = PoseProblem(sc["lines"], sc["points"], sc["aligned"])
    rng = np.random.default_rng(1)
    models = np.stack([sc["gt_pose"] + rng.normal(0, s, (3, 4)) for s in (0, 1e-4, 1e-3, 1e-2, 0.1, 1.0, 3.0)] * 3)
    models[5, 2] *= -1
    models[6, 2, 3] = 1e-17              # depths around DBL_EPSILON
    models[6, 2, :3] = 0.0
    res = pp.residuals(models)
    for m in range(len(models)):
        want = oracle.line_residuals(sc["lines"], sc["points"], models[m])
        assert np.array_equal(res[m].view(np.uint64), want.view(np.uint64))
    for thr in (1e-7, sc["max_error"] ** 2, 1e-2, 1e3):
        inl, sums = pp.score(models, thr)
        for m in range(len(models)):
            n, s = _tree_support(res[m], thr)
            assert inl[m] == n
            assert np.float64(sums[m]).view(np.uint64) == np.float64(s).view(np.uint64), (m, thr)
    pp.close()


def test_score_extreme_ranges(oracle):
    """inputs outside the range where the short reciprocal is proven exact take the full IEEE division: huge
    depth rows, huge / infinite / NaN points; and max_residual >= DBL_MAX counts points behind the camera."""
    from privacy_preserving_sfm_amd.device import PoseProblem
    sc = synthetic.make_ransac_scene(1500, seed=12)
    pts = sc["points"].copy()
    lines = sc["lines"].copy()
    pts[700] *= 1e200            # beyond the point bound from tile 1 on
    pts[900] = [np.inf, 1.0, 2.0]
    pts[901] = [np.nan, 1.0, 2.0]
    pts[1100] *= 1e-300
    pp = PoseProblem(lines, pts)
    models = np.stack([sc["gt_pose"]] * 6)
    models[1, 2] *= 1e290         # depth row beyond the row bound: pz up to ~1e291
    models[2, 2] *= 1e306         # pz overflows for some points
    models[3, 2, 3] = np.nan
    models[4, 2] *= -1
    models[5] *= 1e-200
    res = pp.residuals(models)
    thr_big = np.finfo(np.float64).max
    for thr in (sc["max_error"] ** 2, 1.0, thr_big, np.inf):
        inl, sums = pp.score(models, thr)
        for m in range(len(models)):
            want = oracle.line_residuals(lines, pts, models[m])
            assert np.array_equal(res[m].view(np.uint64), want.view(np.uint64), equal_nan=False) or \
                np.array_equal(np.isnan(res[m]), np.isnan(want))
            n, s = _tree_support(res[m], thr)
            assert inl[m] == n == oracle.support(want, thr)[0], (m, thr)
            if np.isfinite(s):
                assert np.float64(sums[m]).view(np.uint64) == np.float64(s).view(np.uint64), (m, thr)
    pp.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_score_ragged_sizes(oracle, n):
    from privacy_preserving_sfm_amd.device import PoseProblem
    sc = synthetic.make_ransac_scene(max(n, 1), seed=4)
    lines, pts = sc["lines"][:n], sc["points"][:n]
    pp = PoseProblem(lines, pts)
    inl, sums = pp.score(sc["gt_pose"][None], 1e-4)
    if n == 0:
        assert inl[0] == 0 and sums[0] == 0
    else:
        res = oracle.line_residuals(lines, pts, sc["gt_pose"])
        assert inl[0] == oracle.support(res, 1e-4)[0]
    pp.close()


def test_re3q3_reference_properties():
    from privacy_preserving_sfm_amd.device import re3q3_batch
    rng = np.random.default_rng(0)
    c = rng.uniform(-1, 1, (400, 3, 10))
    c[100:150, :, 3] = 0.5 * (c[100:150, :, 5] + c[100:150, :, 4])      # degenerate for x
    c[150:200, :, 0] = 0.5 * (c[150:200, :, 5] + c[150:200, :, 2])      # y
    c[200:250, :, 0] = 0.5 * (c[200:250, :, 1] + c[200:250, :, 3])      # z
    c[250:300, :, 0] = 0.5 * (c[250:300, :, 5] + c[250:300, :, 2]); c[250:300, :, 3] = 0.5 * (c[250:300, :, 5] + c[250:300, :, 4])
    sols, ns = re3q3_batch(c)
    # the reference asserts max|residual| < 1e-8 on ONE random draw per run (test_re3q3.cpp:34-44); over
    # 400 systems a few roots of magnitude ~1e2-1e3 exceed that absolute bound in any fp64 solver (the
    # oracle does too), so the bound is applied relative to the monomial magnitudes, plus a cap on how
    # many roots may miss the reference's absolute bound
    bad_abs = bad_rel = total = 0
    for i in range(400):
        for k in range(ns[i]):
            m = _mons(sols[i, :, k])
            res = np.abs(c[i] @ m).max()
            total += 1
            bad_abs += res >= 1e-8
            bad_rel += res >= 1e-8 and res >= 1e-10 * (np.abs(c[i]) @ np.abs(m)).max()
    assert bad_rel == 0 and bad_abs <= 0.01 * total
    assert np.all(ns % 2 == 0) and ns.sum() > 400
    sq = np.zeros((1, 3, 10)); sq[0, 0, 0] = 1; sq[0, 0, 9] = -1; sq[0, 1, 3] = 1; sq[0, 1, 9] = -1; sq[0, 2, 5] = 1; sq[0, 2, 9] = -1
    sols, ns = re3q3_batch(sq)
    assert ns[0] == 8
    assert sorted(map(tuple, np.round(sols[0, :, :8].T).astype(int))) == sorted((a, b, d) for a in (-1, 1) for b in (-1, 1) for d in (-1, 1))
    assert np.abs(np.abs(sols[0]) - 1).max() < 1e-8


def test_re3q3_matches_oracle(oracle):
    from privacy_preserving_sfm_amd.device import re3q3_batch
    rng = np.random.default_rng(1)
    c = rng.uniform(-1, 1, (200, 3, 10))
    sols, ns = re3q3_batch(c)
    for i in range(200):
        want = oracle.re3q3(c[i])
        assert want.shape[1] == ns[i]
        assert np.allclose(sols[i, :, :ns[i]], want, rtol=1e-7, atol=1e-9)


def test_p6l_batch_matches_oracle(oracle):
    from privacy_preserving_sfm_amd.device import PoseProblem, sampler_draw
    sc = synthetic.make_ransac_scene(300, outlier_ratio=0.3, noise_px=0.0, seed=8, aligned_ratio=0.3)
    pp = PoseProblem(sc["lines"], sc["points"], sc["aligned"])
    samples = sampler_draw(0, 300, 6, 500)
    assert np.array_equal(samples, oracle.sampler(0, 300, 6, 500))     # host sampler == oracle's restated stream
    models, nm = pp.p6l_batch(samples)
    hit = tight = total = 0
    for h in range(500):
        want = oracle.p6l(sc["lines"][samples[h]], sc["points"][samples[h]], sc["aligned"][samples[h]])
        assert len(want) == nm[h], h
        for k in range(nm[h]):
            # L1: 1e-9-class agreement on well-conditioned roots; roots close to a double root are only
            # determined to ~sqrt(eps) by ANY fp64 root finder (the reference's Eigen QR included), there
            # the two solvers may differ up to 1e-5 but the pose must still satisfy the six incidences
            assert np.allclose(models[h, k], want[k], rtol=1e-5, atol=1e-5), (h, k)
            total += 1
            tight += bool(np.allclose(models[h, k], want[k], rtol=1e-8, atol=1e-9))
            Xc = sc["points"][samples[h]] @ models[h, k, :, :3].T + models[h, k, :, 3]
            assert np.abs(np.sum(sc["lines"][samples[h]] * Xc, axis=1)).max() < 1e-8 * max(1.0, np.abs(Xc).max())
        if not sc["is_outlier"][samples[h]].any() and nm[h] > 0:
            hit += int(min(np.abs(models[h, k] - sc["gt_pose"]).max() for k in range(nm[h])) < 1e-7)
    assert hit > 10 and tight >= 0.97 * total
    pp.close()


@pytest.mark.parametrize("seed,n,out", [(0, 400, 0.4), (1, 150, 0.2), (7, 2000, 0.5)])
def test_ransac_matches_sequential_oracle(oracle, seed, n, out):
    from privacy_preserving_sfm_amd.device import PoseProblem, ransac_options
    sc = synthetic.make_ransac_scene(n, outlier_ratio=out, noise_px=0.3, seed=50 + seed, aligned_ratio=0.2)
    pp = PoseProblem(sc["lines"], sc["points"], sc["aligned"])
    # the mapper's options (sfm/incremental_mapper.cc:673-681)
    kw = dict(min_inlier_ratio=0.25, confidence=0.99999, min_num_trials=100, max_num_trials=10000)
    rep, mask = pp.ransac(ransac_options(max_error=sc["max_error"], seed=seed, dyn_num_trials_multiplier=3.0, **kw))
    ref, ref_mask = oracle.p6l_ransac(sc["lines"], sc["points"], sc["aligned"], sc["max_error"], seed=seed, mult=3.0, **kw)
    assert rep.success == ref.success == 1
    assert rep.num_trials == ref.num_trials
    assert rep.best_trial == ref.best_trial and rep.best_model_index == ref.best_model_idx
    assert rep.num_inliers == ref.num_inliers
    assert np.array_equal(mask, ref_mask)
    assert np.allclose(np.array(rep.model), np.array(ref.model), rtol=1e-7, atol=1e-8)
    assert abs(rep.residual_sum - ref.residual_sum) <= 1e-6 * ref.residual_sum
    assert rep.hypotheses_evaluated >= rep.num_trials - 1
    pp.close()


def test_ransac_does_not_depend_on_the_chunk_width(oracle):
    """chunk_trials only sets how far the device runs ahead of the replay (csrc/ransac_host.hpp): one trial per launch, a width that divides nothing,
    64 and the default give the same report, model and mask bit for bit - and the oracle's, as test_ransac_matches_sequential_oracle asserts it"""
    from privacy_preserving_sfm_amd.device import PoseProblem, ransac_options
    seed, n, out = 1, 150, 0.2
    sc = synthetic.make_ransac_scene(n, outlier_ratio=out, noise_px=0.3, seed=50 + seed, aligned_ratio=0.2)
    pp = PoseProblem(sc["lines"], sc["points"], sc["aligned"])
    kw = dict(min_inlier_ratio=0.25, confidence=0.99999, min_num_trials=100, max_num_trials=10000)      # the mapper's options
    ref, ref_mask = oracle.p6l_ransac(sc["lines"], sc["points"], sc["aligned"], sc["max_error"], seed=seed, mult=3.0, **kw)
    runs = []
    for chunk in (1, 7, 64, 0):
        rep, mask = pp.ransac(ransac_options(max_error=sc["max_error"], seed=seed, dyn_num_trials_multiplier=3.0, chunk_trials=chunk, **kw))
        assert rep.success == ref.success == 1
        assert rep.num_trials == ref.num_trials
        assert rep.best_trial == ref.best_trial and rep.best_model_index == ref.best_model_idx
        assert rep.num_inliers == ref.num_inliers
        assert np.array_equal(mask, ref_mask)
        assert np.allclose(np.array(rep.model), np.array(ref.model), rtol=1e-7, atol=1e-8)
        assert abs(rep.residual_sum - ref.residual_sum) <= 1e-6 * ref.residual_sum
        assert rep.hypotheses_evaluated >= rep.num_trials - 1
        runs.append((rep.num_trials, rep.best_trial, rep.best_model_index, rep.num_inliers, rep.residual_sum, tuple(rep.model), mask.tobytes()))
    assert all(r == runs[0] for r in runs[1:])
    pp.close()


def test_ransac_edge_cases():
    from privacy_preserving_sfm_amd.device import PoseProblem, ransac_options
    from privacy_preserving_sfm_amd._capi import PPError
    sc = synthetic.make_ransac_scene(5, seed=2)
    pp = PoseProblem(sc["lines"], sc["points"])
    rep, mask = pp.ransac(ransac_options(max_error=0.01))
    assert rep.success == 0 and rep.num_trials == 0 and mask.sum() == 0      # fewer than kMinNumSamples
    with pytest.raises(PPError):
        pp.ransac(ransac_options(max_error=0.0))                             # RANSACOptions::Check
    pp.close()
    # all lines gravity-aligned: P6L returns no model (absolute_pose.cc:87-97) => no success
    sc = synthetic.make_ransac_scene(50, seed=3, aligned_ratio=1.1)
    pp = PoseProblem(sc["lines"], sc["points"], sc["aligned"])
    rep, mask = pp.ransac(ransac_options(max_error=sc["max_error"], max_num_trials=200))
    assert rep.success == 0 and rep.num_trials == 200 and rep.num_inliers == 0
    # chunks that do not divide the cap stop exactly at it
    rep, mask = pp.ransac(ransac_options(max_error=sc["max_error"], max_num_trials=200, chunk_trials=7))
    assert rep.success == 0 and rep.num_trials == 200 and rep.num_inliers == 0
    pp.close()


def test_throughput_form_full_size_properties():
    """cfg 4 shape, reduced H: the best-of-H selection equals a host arg-max over the returned scores,
    and the winner's mask agrees with the truth labels."""
    from privacy_preserving_sfm_amd.device import PoseProblem
    sc = synthetic.make_ransac_scene(50000, outlier_ratio=0.5, noise_px=0.5, seed=0xBADC0DE)
    pp = PoseProblem(sc["lines"], sc["points"], sc["aligned"])
    thr = sc["max_error"] ** 2
    rep = pp.hypotheses(8192, thr, seed=0)
    assert rep.success == 1 and rep.models_scored > 8192
    model = np.array(rep.model).reshape(3, 4)
    inl, sums = pp.score(model[None], thr)
    assert inl[0] == rep.num_inliers and sums[0] == rep.residual_sum
    res = pp.residuals(model[None])[0]
    mask = res <= thr
    assert mask.sum() == rep.num_inliers
    assert (mask[~sc["is_outlier"]]).mean() > 0.95
    rep2 = pp.hypotheses(8192, thr, seed=0)      # deterministic
    assert rep2.num_inliers == rep.num_inliers and rep2.best_trial == rep.best_trial and list(rep2.model) == list(rep.model)
    pp.close()


# ---- a-10 against the reference itself (src/optim/support_measurement.cc:36-60 compiled in place; fixture
# tests/golden/support_measurement_scene.json, generator tests/golden/gen_support_measurement_golden.py) ---------------
def test_support_matches_reference_support_measurer_fixture(oracle):
    import support_fixture as sf
    from privacy_preserving_sfm_amd.device import PoseProblem
    sc = sf.read_scene()
    ev, cmp, win = sc["expected"]
    pp = PoseProblem(sc["lines"], sc["points"], None)
    models = sc["models"]
    # the residual vectors the reference's Evaluate was run on are the device's, bit for bit
    assert np.array_equal(pp.residuals(models).view(np.uint64), sc["residuals"].view(np.uint64))
    for t, thr in enumerate(sc["thresholds"]):            # 0, max_error^2, a quarter of it, DBL_MAX, inf
        inl, sums = pp.score(models, thr, sequential=True)        # pp_pose_support_sequential
        tinl, tsums = pp.score(models, thr)                       # K4: exact counts, fixed-tree sums
        for m in range(len(models)):
            assert inl[m] == ev[t][m][0] == tinl[m], (t, m)
            assert sf.same_bits(sums[m], ev[t][m][1]), (t, m, sums[m], ev[t][m][1])
        # Compare / the sequential accept rule (optim/ransac.h:232-236) on the device's supports = the reference's table
        got = [(int(inl[m]), float(sums[m])) for m in range(len(models))]
        best, winner = (0, np.finfo(np.float64).max), -1
        for m, g in enumerate(got):
            for j, g2 in enumerate(got):
                assert oracle.support_better(*g, *g2) == cmp[t][m, j]
            if oracle.support_better(*g, *best):
                best, winner = g, m
        assert winner == win[t]
    # the winner rule of pp_pose_hypotheses over the fixture's six-tuples: first strictly better in (trial, model) order under
    # the Compare the CPU test pins to the reference (test_support_restatement_equals_reference_support_measurer_bit_for_bit)
    for thr in sc["thresholds"][1:3]:
        rep = pp.hypotheses(len(sc["samples"]), thr, samples=sc["samples"])
        nm, hinl, hsum = pp.last_scores(len(sc["samples"]))
        best, where = (0, np.finfo(np.float64).max), (-1, -1)
        for h in range(len(nm)):
            for s in range(nm[h]):
                g = (int(hinl[h, s]), float(hsum[h, s]))
                if oracle.support_better(*g, *best):
                    best, where = g, (h, s)
        assert (rep.best_trial, rep.best_model_index) == where and rep.num_inliers == best[0]
    pp.close()
