"""pp_ba_covariance_blocks on the device against the refined Schur route of tests/covariance_blocks_reference.py (never against the code under test).

Error of a block: e = ||Sigma_ab - Sigma*_ab||_F / sqrt(||Sigma*_aa||_F ||Sigma*_bb||_F).
Bar: e <= max(4 e_LAPACK, kappa_2(S_scaled) sqrt(n) u), u = 2^-53 (covariance_reference.bar); e_LAPACK = the plain float64 Schur route against the refined one
over the requested blocks.  Every test asserts kappa < 1e10 and bar < 1e-5 before it judges.  The gauge is synthetic.make_ba_scene's (pose 0 constant,
tvec[1].x constant) unless the case says otherwise.

Scenes (kappa_2(S_scaled), n, bar on the host):
    cfg 1 = 20 / 250 / 8, seed 0xC0FFEE + 1, SIMPLE_RADIAL                4.3e2   113  5.1e-13
    cfg 1, the one shared camera's f and k variable                         8.9e3   115  1.1e-11
    cfg 1, three cameras (0 1 2 0 1 2 ..), f and k variable                 2.3e5   119  2.8e-10
    cfg 1, a camera per image, f and k variable                             3.2e5   153  4.4e-10
    cfg 1 as THIN_PRISM_FISHEYE, a camera per image, 10 variable            1.2e6   313  2.3e-9
    72 / 200 / 70, seed 0xC0FFEE + 2 (tracks of 70: three staging chunks)   2.6e4   425  6.0e-11
    sequence 100 / 1500 / 6, window 10, seed 0xC0FFEE + 9 (renumbered)      1.1e7   593  2.9e-8
Observed on MI355X (ACCURACY lines: kappa, n, e_LAPACK, bar, blocks, worst error):
    cfg1 all kinds                   4.34e+02  113  2.86e-15  5.12e-13  1206  4.39e-15
    cfg1 constant blocks             1.18e+01  105  5.38e-17  1.35e-14   256  5.28e-16
    cfg1 shared camera               8.90e+03  115  1.25e-13  1.06e-11   233  7.22e-12
    cfg1 three cameras               2.28e+05  119  2.17e-13  2.76e-10   335  2.16e-11
    cfg1 camera per image tail       3.17e+05  153  6.09e-12  4.35e-10   413  6.22e-12      beside  5.74e-13
    cfg1 thin prism 10 var tail      1.15e+06  313  4.48e-12  2.27e-09   413  1.31e-11      beside  1.67e-11
    72/200/70 long tracks            2.62e+04  425  9.62e-14  5.99e-11   222  2.73e-14
    sequence 100 reordered           1.07e+07  593  1.06e-11  2.89e-08   495  4.02e-11
    cfg1 new entry / old entry       4.34e+02  113  2.86e-15  5.12e-13   650  4.39e-15 / 4.39e-15, 0.00e+00 apart
    BundleAdjuster.CovarianceBlocks  8.90e+03  115  1.25e-13  1.06e-11     7  5.92e-12
The judge is the Schur route with S formed in long double (covariance_blocks_reference.schur_inverse_ld).  With SchurCovariance.inv as it stands in its place
(S formed in float64) the same device results read: shared camera 1.28e-10 - above the bar, and so are the unchanged pose blocks of pp_ba_covariance on
that scene, 1.17e-10 -, three cameras 1.09e-11, camera per image 1.18e-11 / 1.85e-11, thin prism 1.90e-11 / 1.72e-11, long tracks 2.07e-13, sequence
1.83e-10, cfg1 4.06e-14: inv itself is 1.2e-10 from an inverse taken in long double throughout on the shared-camera scene, the device 6.9e-12.
Timing (recorded, not gated): cfg 3 = 500 / 25 000 / 8, seed 0xC0FFEE + 3: 500 diagonal pose blocks + 500 pose x point + 500 point x point blocks,
info.device_ms, median of five calls after a warm-up: 3.29 ms (3.06 ms of it the front half: a request of one block), beside pp_ba_covariance's 6.47 ms
(6.43 ms in the same run) for every diagonal pose block and all 25 000 points.
"""
import ctypes as C

import numpy as np
import pytest

import covariance_blocks_reference as cbr
import covariance_reference as cr
from privacy_preserving_sfm_amd import _capi, synthetic
from privacy_preserving_sfm_amd.device import BAProblem, ba_options, plan_ordering

pytestmark = pytest.mark.gpu

CFG1 = dict(num_cams=20, num_points=250, track=8, seed=0xC0FFEE + 1, model=2)
FK = 0xFFFF & ~0b1001                    # SIMPLE_RADIAL: f and k variable
THIN10 = 0xFFFF & ~0b111111110011        # THIN_PRISM_FISHEYE: fx fy and the eight extra parameters variable
_cache = {}


def _scene(name):
    """(scene, its SchurCovariance): built once, shared, never modified"""
    if name not in _cache:
        if name == "cfg1":
            sc = synthetic.make_ba_scene(**CFG1)
        elif name == "constant":      # the modifications of test_gpu_covariance.test_constant_blocks_are_zero_where_stated
            sc = synthetic.make_ba_scene(**CFG1)
            sc["pose_const"][5] = 1
            sc["tvec_const_mask"][7] = 0b101
            sc["point_const"][::10] = 1
        elif name in ("shared", "three", "per image"):
            sc = synthetic.make_ba_scene(**CFG1, num_intrinsics={"shared": 1, "three": 3, "per image": 20}[name])
            sc["camera_const_mask"][:] = FK
        elif name == "thin prism":
            sc = synthetic.make_ba_scene(**dict(CFG1, model=10), num_intrinsics=20)
            sc["camera_const_mask"][:] = THIN10
        elif name == "long tracks":
            sc = synthetic.make_ba_scene(num_cams=72, num_points=200, track=70, seed=0xC0FFEE + 2, model=2)
        elif name == "sequence":
            sc = synthetic.make_ba_scene(num_cams=100, num_points=1500, track=6, seed=0xC0FFEE + 9, model=2, window=10)
        _cache[name] = (sc, cr.SchurCovariance(sc))
    return _cache[name]


def _run(sc, blocks, **kw):
    pb = BAProblem(sc, device=0, **kw)
    try:
        return pb.covariance_blocks(blocks)
    finally:
        pb.close()


def _pose_point(images, points):
    return [(("pose", i), ("point", p)) for i in images for p in points]


def _point_pairs(P, rng, count):
    """`count` random pairs of points, the first tenth of them a point with itself"""
    pq = rng.integers(0, P, (count, 2))
    pq[:count // 10, 1] = pq[:count // 10, 0]
    return [(("point", int(p)), ("point", int(q))) for p, q in pq]


def _camera_kinds_request(sc, rng, cams, cam_pairs):
    """every kind a scene with variable intrinsics has, sampled: intrinsics x intrinsics for cam_pairs, each camera of cams against every image (both ways for
    some) and against every 17th point (both ways), pose x pose / pose x point / point x point samples"""
    Cn, Pn = sc["poses"].shape[0], sc["points"].shape[0]
    pts = list(range(3, Pn, 17))
    blocks = [(("intrinsics", k), ("intrinsics", l)) for k, l in cam_pairs]
    for k in cams:
        blocks += [(("pose", i), ("intrinsics", k)) for i in range(Cn)] + [(("intrinsics", k), ("pose", i)) for i in range(0, Cn, 3)]
        blocks += [(("intrinsics", k), ("point", p)) for p in pts] + [(("point", p), ("intrinsics", k)) for p in pts[::3]]
    blocks += [(("pose", i), ("pose", int(j))) for i in range(Cn) for j in rng.integers(0, Cn, 2)]
    blocks += _pose_point(range(0, Cn, 3), pts) + _point_pairs(Pn, rng, 40)
    return blocks


def _assert_transposes(blocks, got):
    where = {b: q for q, b in enumerate(blocks)}
    checked = 0
    for (a, b), q in where.items():
        if (b, a) in where:
            assert np.allclose(got[q], got[where[(b, a)]].T, rtol=1e-9, atol=0), (a, b)
            checked += 1
    return checked


def test_cfg1_every_kind_without_intrinsics(oracle):
    sc, schur = _scene("cfg1")
    rng = np.random.default_rng(21)
    pts = list(range(0, 250, 17))
    # two points no image sees both: their block is non-zero all the same (S^-1 is dense)
    seen = np.zeros((250, 20), dtype=bool)
    seen[sc["obs_point"], sc["obs_pose"]] = True
    apart = [(p, q) for p in range(250) for q in range(p + 1, 250) if not (seen[p] & seen[q]).any()]
    assert apart, "no pair of points without a common image in this scene"
    blocks = [(("pose", i), ("pose", j)) for i in range(20) for j in range(20)]
    blocks += _pose_point(range(20), pts) + [(b, a) for a, b in _pose_point(range(20), pts)]
    blocks += _point_pairs(250, rng, 200) + [(("point", p), ("point", q)) for p, q in apart[:3]] + [(("point", q), ("point", p)) for p, q in apart[:3]]
    got = _run(sc, blocks)
    cbr.judge("cfg1 all kinds", schur, blocks, got)
    assert _assert_transposes(blocks, got) >= 400 + 600
    for (a, b), g in zip(blocks, got):
        for side, rows in ((a, g), (b, g.T)):
            if side == ("pose", 0):                        # the constant pose
                assert not rows.any()
            if side == ("pose", 1):                        # the constant component tvec[1].x
                assert not rows[3].any()
    assert got[blocks.index((("pose", 1), ("point", 17)))][[0, 1, 2, 4, 5]].all()
    far = got[blocks.index((("point", apart[0][0]), ("point", apart[0][1])))]
    assert far.any()


def test_constant_blocks_are_exactly_zero_in_the_cross_blocks(oracle):
    sc, schur = _scene("constant")
    pts = [0, 10, 3, 17, 20, 121, 240, 249]
    blocks = _pose_point(range(20), pts) + [(b, a) for a, b in _pose_point((0, 5, 7, 12), pts)]
    blocks += [(("point", p), ("point", q)) for p in pts for q in pts]
    got = _run(sc, blocks)
    for (a, b), g in zip(blocks, got):
        for side, rows in ((a, g), (b, g.T)):
            if side in (("pose", 0), ("pose", 5)) or (side[0] == "point" and side[1] % 10 == 0):
                assert not rows.any(), (a, b)
            if side == ("pose", 7):
                assert not rows[3].any() and not rows[5].any()
            if side == ("pose", 1):
                assert not rows[3].any()
    assert got[blocks.index((("pose", 12), ("point", 3)))].all() and got[blocks.index((("point", 17), ("point", 121)))].all()
    cbr.judge("cfg1 constant blocks", schur, blocks, got)


def test_shared_variable_camera(oracle):
    sc, schur = _scene("shared")
    blocks = _camera_kinds_request(sc, np.random.default_rng(22), [0], [(0, 0)])
    got = _run(sc, blocks)
    cbr.judge("cfg1 shared camera", schur, blocks, got)
    kk = got[0]
    for j in (1, 2, 4, 5, 6, 7, 8, 9, 10, 11):
        assert not kk[j].any() and not kk[:, j].any()
    live = kk[np.ix_([0, 3], [0, 3])]
    assert np.allclose(live, live.T, rtol=1e-9, atol=0) and np.linalg.eigvalsh(0.5 * (live + live.T))[0] > 0
    for (a, b), g in zip(blocks, got):      # the constant slots are zero in the cross blocks too
        if a[0] == "intrinsics":
            assert not g[[1, 2] + list(range(4, 12))].any()
        if b[0] == "intrinsics":
            assert not g[:, [1, 2] + list(range(4, 12))].any()
    assert _assert_transposes(blocks, got) > 10


def test_three_cameras_shared_among_the_images(oracle):
    sc, schur = _scene("three")
    assert list(sc["pose_camera"][:6]) == [0, 1, 2, 0, 1, 2]
    blocks = _camera_kinds_request(sc, np.random.default_rng(23), [0, 1, 2], [(k, l) for k in range(3) for l in range(3)])
    got = _run(sc, blocks)
    cbr.judge("cfg1 three cameras", schur, blocks, got)
    assert _assert_transposes(blocks, got) > 30


@pytest.mark.parametrize("layout", ["tail", "beside"])
def test_camera_per_image(oracle, monkeypatch, layout):
    monkeypatch.setenv("PPSFM_BA_INTR_LAYOUT", layout)
    sc, schur = _scene("per image")
    rng = np.random.default_rng(24)
    pairs = [(k, k) for k in range(20)] + [tuple(int(v) for v in rng.integers(0, 20, 2)) for _ in range(20)]
    blocks = _camera_kinds_request(sc, rng, [0, 1, 7, 19], pairs)
    got = _run(sc, blocks)
    cbr.judge("cfg1 camera per image " + layout, schur, blocks, got)


@pytest.mark.parametrize("layout", ["tail", "beside"])
def test_thin_prism_fisheye_with_ten_variable_parameters(oracle, monkeypatch, layout):
    """the widest side: 10 of 12 slots live, both halves of a 12-wide side carry columns (cx, cy constant: slots 2 and 3 are zero)"""
    monkeypatch.setenv("PPSFM_BA_INTR_LAYOUT", layout)
    sc, schur = _scene("thin prism")
    rng = np.random.default_rng(25)
    pairs = [(k, k) for k in range(20)] + [tuple(int(v) for v in rng.integers(0, 20, 2)) for _ in range(20)]
    blocks = _camera_kinds_request(sc, rng, [0, 1, 7, 19], pairs)
    got = _run(sc, blocks)
    cbr.judge("cfg1 thin prism 10 var " + layout, schur, blocks, got)
    for q in range(20):
        kk = got[q]
        assert not kk[2:4].any() and not kk[:, 2:4].any()
        live = np.delete(np.delete(kk, [2, 3], 0), [2, 3], 1)
        assert np.allclose(live, live.T, rtol=1e-9, atol=0) and np.linalg.eigvalsh(0.5 * (live + live.T))[0] > 0


def test_long_tracks_take_several_staging_chunks(oracle):
    sc, schur = _scene("long tracks")
    assert np.bincount(sc["obs_point"]).max() > 64
    rng = np.random.default_rng(26)
    blocks = _point_pairs(200, rng, 60) + _pose_point(range(0, 72, 5), range(1, 200, 23)) + [(b, a) for a, b in _pose_point((1, 30, 71), range(1, 200, 23))]
    got = _run(sc, blocks)
    cbr.judge("72/200/70 long tracks", schur, blocks, got)
    assert _assert_transposes(blocks, got) > 5


def test_reordered_images_are_asked_for_in_the_callers_order(oracle):
    sc, schur = _scene("sequence")
    old_of_new, plan = plan_ordering(sc)
    assert plan["reordered"] and not np.array_equal(old_of_new, np.arange(100))
    rng = np.random.default_rng(27)
    pts = [int(p) for p in rng.choice(1500, 25, replace=False)]
    blocks = _pose_point(range(0, 100, 7), pts) + [(("point", p), ("pose", int(i))) for p in pts[:5] for i in rng.integers(0, 100, 4)]
    blocks += [(("pose", int(i)), ("pose", int(j))) for i, j in rng.integers(0, 100, (60, 2))] + _point_pairs(1500, rng, 40)
    pb = BAProblem(sc, device=0)
    assert pb.structure()["reordered"]
    got = pb.covariance_blocks(blocks)
    pb.close()
    cbr.judge("sequence 100 reordered", schur, blocks, got)


def test_agreement_with_pp_ba_covariance(oracle):
    sc, schur = _scene("cfg1")
    pairs = [(i, j) for i in range(20) for j in range(20)]
    points = list(range(250))
    blocks = [(("pose", i), ("pose", j)) for i, j in pairs] + [(("point", p), ("point", p)) for p in points]
    pb = BAProblem(sc, device=0)
    pc, xc = pb.covariance(pairs, points)
    got = pb.covariance_blocks(blocks)
    pb.close()
    old = list(pc) + list(xc)
    limit, _ = cbr.judge("cfg1 new entry", schur, blocks, got)
    cbr.judge("cfg1 old entry", schur, blocks, old)
    ref = cbr.SchurBlocks(schur)
    apart = max(cr.block_error(g, o, ref.diag(a), ref.diag(b)) for (a, b), g, o in zip(blocks, got, old))
    print("cfg1: new entry against pp_ba_covariance %.2e (2 x bar = %.2e)" % (apart, 2 * limit))
    assert apart <= 2 * limit


def _mixed_request(sc, rng, count):
    Cn, Pn, Kn = sc["poses"].shape[0], sc["points"].shape[0], sc["intr"].shape[0]
    sides = [("pose", Cn), ("intrinsics", Kn), ("point", Pn)]
    out = []
    for _ in range(count):
        (ka, na), (kb, nb) = sides[rng.integers(0, 3)], sides[rng.integers(0, 3)]
        out.append(((ka, int(rng.integers(0, na))), (kb, int(rng.integers(0, nb)))))
    return out


def test_two_calls_are_bitwise_equal():
    sc = synthetic.make_ba_scene(100, 5000, 8, seed=0xC0FFEE + 2, model=2, num_intrinsics=4)
    sc["camera_const_mask"][:] = FK
    blocks = _mixed_request(sc, np.random.default_rng(28), 600)
    pb = BAProblem(sc, device=0)
    a = pb.covariance_blocks(blocks)
    b = pb.covariance_blocks(blocks)
    pb.close()
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and any(x.any() for x in a)


def _solve_record(pb, s):
    return (s.initial_cost, s.final_cost, s.num_successful_steps, s.num_unsuccessful_steps, s.termination, s.num_iterations, s.linear_solver, s.cholesky_fallbacks)


def test_covariance_blocks_then_solve_equals_solve_alone():
    sc = synthetic.make_ba_scene(**CFG1, num_intrinsics=20)
    sc["camera_const_mask"][:] = FK
    blocks = _mixed_request(sc, np.random.default_rng(29), 200)
    out = []
    for with_cov in (True, False):
        pb = BAProblem(sc, device=0)
        if with_cov:
            pb.covariance_blocks(blocks)
        s = pb.solve(ba_options(max_num_iterations=8))
        out.append((pb.get_parameters(), pb.trace(), _solve_record(pb, s)))
        pb.close()
    (pa, ta, sa), (pb_, tb, sb) = out
    assert all(np.array_equal(x, y) for x, y in zip(pa, pb_)) and np.array_equal(ta, tb) and sa == sb


def test_covariance_blocks_between_two_solves_changes_nothing():
    """a used handle: solve, covariance_blocks, solve against solve, solve (the pattern of test_gpu_covariance.test_covariance_between_two_solves_changes_nothing)"""
    sc = synthetic.make_ba_scene(100, 5000, 8, seed=0xC0FFEE + 2, model=2)
    blocks = _mixed_request(sc, np.random.default_rng(30), 400)
    out = []
    for with_cov in (True, False):
        pb = BAProblem(sc, device=0)
        s1 = pb.solve(ba_options(max_num_iterations=3))
        if with_cov:
            pb.covariance_blocks(blocks)
        s2 = pb.solve(ba_options(max_num_iterations=5))
        out.append((pb.get_parameters(), pb.trace(), [_solve_record(pb, s) for s in (s1, s2)]))
        pb.close()
    (pa, ta, sa), (pb_, tb, sb) = out
    assert all(np.array_equal(x, y) for x, y in zip(pa, pb_)) and np.array_equal(ta, tb) and sa == sb


def _raw_call(pb, quads, capacity=None):
    """the C entry with raw (kind_a, index_a, kind_b, index_b) quadruples -> (return code, pp_last_error text)"""
    L = _capi.lib()
    req = (_capi.CovBlock * max(1, len(quads)))(*[_capi.CovBlock(*q) for q in quads])
    out = np.zeros(144 * max(1, len(quads)))
    o = ba_options()
    rc = L.pp_ba_covariance_blocks(pb._h, C.byref(o), len(quads), req, _capi.dp(out), out.size if capacity is None else capacity, None)
    return rc, L.pp_last_error().decode(errors="replace")


def test_error_reporting():
    sc, _ = _scene("cfg1")
    pb = BAProblem(sc, device=0)
    rc, text = _raw_call(pb, [(0, 1, 3, 0)])
    assert rc == _capi.PP_ERR_INVALID and "unknown kind" in text
    rc, text = _raw_call(pb, [(-1, 1, 0, 0)])
    assert rc == _capi.PP_ERR_INVALID and "unknown kind" in text
    for quad in ((0, 20, 0, 0), (0, 0, 0, -1), (1, 1, 0, 0), (2, 0, 1, -1), (2, 250, 2, 0), (0, 3, 2, -1)):
        rc, text = _raw_call(pb, [(0, 1, 2, 5), quad])
        assert rc == _capi.PP_ERR_INVALID and "block 1" in text and "out of range" in text, (quad, text)
    rc, text = _raw_call(pb, [(0, 1, 2, 5), (1, 0, 1, 0)], capacity=18 + 143)
    assert rc == _capi.PP_ERR_INVALID and "capacity" in text
    rc, text = _raw_call(pb, [])
    assert rc == _capi.PP_OK
    assert pb.covariance_blocks([]) == []
    pb.close()
    pb = BAProblem(sc, device=0, linear_solver=_capi.LINEAR_SOLVER_ITERATIVE_SCHUR)
    with pytest.raises(_capi.PPError) as e:
        pb.covariance_blocks([(("pose", 1), ("point", 0))])
    assert e.value.code == _capi.PP_ERR_INVALID and "iterative" in str(e.value)
    pb.close()


def test_group_attached_handle_is_refused():
    """as test_gpu_covariance.test_group_attached_handle_is_refused: refused while attached, served once detached"""
    sc, _ = _scene("cfg1")
    pb = BAProblem(sc, device=0, ordering=1)
    pb.set_allreduce(lambda ptr, count, op: 0, group_rank=0, group_size=1)
    with pytest.raises(_capi.PPError) as e:
        pb.covariance_blocks([(("pose", 1), ("point", 0))])
    assert e.value.code == _capi.PP_ERR_INVALID and "attached to a group" in str(e.value)
    pb.set_allreduce(None)
    (block,) = pb.covariance_blocks([(("pose", 2), ("point", 0))])
    pb.close()
    assert block.shape == (6, 3) and np.isfinite(block).all() and block.any()


def test_a_free_gauge_is_a_numeric_error_and_the_handle_solves_afterwards():
    free = synthetic.make_ba_scene(**CFG1)
    free["pose_const"][:] = 0
    free["tvec_const_mask"][:] = 0
    pb = BAProblem(free, device=0)
    with pytest.raises(_capi.PPError) as e:
        pb.covariance_blocks([(("pose", 1), ("point", 0))])
    assert e.value.code == _capi.PP_ERR_NUMERIC and "pp_ba_covariance_blocks" in str(e.value)
    s = pb.solve(ba_options(max_num_iterations=5))
    assert s.num_successful_steps >= 1 and s.final_cost < s.initial_cost
    pb.close()
    ref = BAProblem(free, device=0)
    s2 = ref.solve(ba_options(max_num_iterations=5))
    ref.close()
    assert (s.final_cost, s.num_iterations) == (s2.final_cost, s2.num_iterations)


def test_bundle_adjuster_covariance_blocks(oracle):
    from privacy_preserving_sfm_amd.bundle_adjustment import BundleAdjuster, BundleAdjustmentConfig, BundleAdjustmentOptions, Reconstruction
    sc, _ = _scene("cfg1")
    rec = Reconstruction.from_scene(sc)
    cfg = BundleAdjustmentConfig()
    for i in range(20):
        cfg.AddImage(i)
    cfg.SetConstantPose(0)
    cfg.SetConstantTvec(1, [0])
    opt = BundleAdjustmentOptions()
    opt.print_summary = False
    opt.refine_focal_length = opt.refine_extra_params = True
    ba = BundleAdjuster(opt, cfg)
    scene, pose_index, point_index, cam_index = ba.flatten(rec)
    assert [point_index[p] for p in range(250)] != list(range(250))      # the keys are ids, not positions
    keys = [(("image", 3), ("image", 3)), (("image", 7), ("point", 17)), (("camera", 0), ("camera", 0)), (("point", 199), ("camera", 0)), (("camera", 0), ("image", 12)),
            (("point", 4), ("point", 230)), (("image", 0), ("point", 5))]
    got = ba.CovarianceBlocks(rec, keys)
    assert list(got) == keys
    assert [got[k].shape for k in keys] == [(6, 6), (6, 3), (4, 4), (3, 4), (4, 6), (3, 3), (6, 3)]      # SIMPLE_RADIAL: NumParams() = 4
    side = {"image": lambda i: ("pose", pose_index[i]), "camera": lambda c: ("intrinsics", cam_index[c]), "point": lambda p: ("point", point_index[p])}
    blocks = [(side[a[0]](a[1]), side[b[0]](b[1])) for a, b in keys]
    schur = cr.SchurCovariance(scene)
    full = [np.zeros((cbr.WIDTH[a[0]], cbr.WIDTH[b[0]])) for a, b in blocks]
    for f, k in zip(full, keys):
        f[:got[k].shape[0], :got[k].shape[1]] = got[k]
    limit, _ = cbr.judge("BundleAdjuster.CovarianceBlocks", schur, blocks, full)
    assert not got[keys[-1]].any() and got[keys[2]][0, 0] > 0 and got[keys[2]][3, 3] > 0 and not got[keys[2]][1:3].any()
    poses, _ = ba.Covariance(rec, [3])
    ref = cbr.SchurBlocks(schur)
    d = ref.diag(("pose", pose_index[3]))
    assert cr.block_error(got[keys[0]], poses[3], d, d) <= 2 * limit
