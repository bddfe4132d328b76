"""pp_tracks_complete / pp_tracks_merge on the device against the sequential oracle (tests/tracks_reference.py): EXACT equality - the same pairs in
the same order, the same merges and new indices, the same counts and final state.

The device and the oracle round differently (fused multiply-adds) far below 1e-6 relative, so every scene's seed was picked on the CPU for an oracle
margin (smallest relative distance of a tested squared error from its squared threshold) above 1e-6, and each test asserts that margin; no candidate
is left out of any comparison.  Oracle margins over complete + merge (quiet start): (20,150,10, seed 1) 6.7e-3, (20,150,10, seed 2) 0.62,
(24,200,12, seed 5) 0.11, (100,1500,10, seed 4) 3.8e-2, (500,6000,8, seed 11, window 40) 1.4e-3; the subset run 0.17; the hand-built scenes ~1.
Loop integration ((20,300,10, seed 4), the noisy suite's observation model): 5 rounds, margin 1.1e-3 over completion, merge and filter thresholds
(asserted above 1e-4), completed 12 / 47 / 17 / 11 / 8 per round after 494 + 196 before the loop, round 1 filters 2673; decisions unchanged under three
1e-12 perturbations of the input points.  Measured on an MI355X: all of this file passes."""
import copy

import numpy as np
import pytest

import tracks_reference as tr
import tracks_refinement_oracle as tro
from privacy_preserving_sfm_amd import synthetic
from privacy_preserving_sfm_amd.bundle_adjustment import (Camera, FeatureLine, Image, IncrementalMapperOptions, IterativeGlobalRefinement, Point3D,
                                                          Reconstruction)
from privacy_preserving_sfm_amd.device import TracksProblem, tracks_options
from privacy_preserving_sfm_amd.incremental_triangulator import CorrespondenceGraph, IncrementalTriangulator, reconstruction_from_completion_scene

pytestmark = pytest.mark.gpu

QUIET = dict(noise_point=1e-4, noise_t=1e-5, noise_q=1e-5)
SMALL = [(20, 150, 10, 1), (20, 150, 10, 2), (24, 200, 12, 5)]


def _check_state(pb, rec, point_ids, line_ref):
    """the handle's state against the oracle's reconstruction (device index i = point id i in these scenes, new points included)"""
    st = pb.state()
    want_lp = np.array([rec.images[i].lines[k].Point3DId() for (i, k) in line_ref], dtype=np.int32)
    assert np.array_equal(st["line_point"], want_lp)
    P = len(st["deleted"])
    assert sorted(rec.points3D) == [p for p in range(P) if not st["deleted"][p]]
    for p, pt in rec.points3D.items():
        assert np.array_equal(st["points"][p], pt.xyz), (p, st["points"][p], pt.xyz)
        assert [line_ref[l] for l in st["track_line"][st["track_start"][p]:st["track_start"][p + 1]]] == pt.track


def _compare(world, ops, subset_ids=None, options=None):
    """runs `ops` (a string of 'c' / 'm') on one handle and on the oracle over a copy; -> (reports, oracle)"""
    rec, graph = world
    orec = copy.deepcopy(rec)
    oracle = tr.TracksOracle(graph, orec)
    oo = options or tr.Options()
    flat, point_ids, line_ref = IncrementalTriangulator(graph, rec).flatten()
    assert point_ids == list(range(len(point_ids)))
    do = tracks_options(merge_max_reproj_error=oo.merge_max_reproj_error, complete_max_reproj_error=oo.complete_max_reproj_error,
                        complete_max_transitivity=oo.complete_max_transitivity)
    pb = TracksProblem(flat)
    reports = []
    try:
        for op in ops:
            P = pb.num_points()[0]
            sub = None if subset_ids is None else np.array([p in subset_ids for p in range(P)], dtype=np.uint8)
            ids = None if subset_ids is None else [p for p in subset_ids if p < P]
            if op == "c":
                c0 = len(oracle.completed)
                n = oracle.CompleteTracks(oo, ids)
                rep, pairs = pb.complete(do, sub)
                assert [(int(p), line_ref[l]) for p, l in pairs] == oracle.completed[c0:]
                assert rep.num_changed == n == rep.num_entries
            else:
                m0 = len(oracle.merged)
                n = oracle.MergeTracks(oo, ids)
                rep, merges = pb.merge(do, sub)
                assert [tuple(int(v) for v in row) for row in merges] == oracle.merged[m0:]
                assert rep.num_changed == n and rep.num_entries == len(oracle.merged) - m0
            reports.append(rep)
            _check_state(pb, orec, point_ids, line_ref)
    finally:
        pb.close()
    print("oracle margin %.3e over %d tested pairs" % (oracle.margin, len(oracle.tested)))
    assert oracle.margin > 1e-6
    return reports, oracle


def _scene_world(cfg, **kw):
    sc = synthetic.make_completion_scene(*cfg[:3], seed=cfg[3], **dict(QUIET, **kw))
    return reconstruction_from_completion_scene(sc)


@pytest.mark.parametrize("cfg", SMALL + [(100, 1500, 10, 4)])
@pytest.mark.parametrize("ops", ["c", "m", "cm"])
def test_equals_the_oracle(cfg, ops, oracle):
    reports, o = _compare(_scene_world(cfg), ops)
    assert len(o.completed) > 0 or len(o.merged) > 0
    assert all(r.candidates_evaluated > 0 for r in reports)


@pytest.mark.parametrize("ops", ["c", "m", "cm"])
def test_equals_the_oracle_500_images(ops, oracle):
    """configs[2]-derived: 500 images, a sequence window as the block-banded benchmark scene"""
    reports, o = _compare(_scene_world((500, 6000, 8, 11), window=40, split=0.1), ops)
    assert ("c" not in ops or len(o.completed) > 1000) and ("m" not in ops or len(o.merged) > 100)


def test_subset_form(oracle):
    world = _scene_world(SMALL[0])
    subset = set(range(0, 200, 3))
    reports, o = _compare(world, "cm", subset_ids=subset)
    assert 0 < len(o.completed) and all(p in subset for p, _ in o.completed)


# ---- hand-built scenes: conflicts between points, the merge recursion, a closure larger than the on-chip list --------------------------------

class _World:
    """cameras of a make_ba_scene ring at their true poses; add_point / add_line build exact observations (a random line through the projection)"""

    def __init__(self, num_cams=12, seed=0):
        base = synthetic.make_ba_scene(num_cams, 10, 4, seed=seed)
        self.rng = np.random.default_rng(seed + 1000)
        self.rec, self.graph = Reconstruction(), CorrespondenceGraph()
        self.rec.cameras[0] = Camera(0, 2, base["intr"][0, :4], width=1280, height=960)
        self.poses = base["gt_poses"]
        for c in range(num_cams):
            self.rec.images[c] = Image(c, 0, self.poses[c, :4], self.poses[c, 4:])

    def add_line(self, c, X, point_id=-1):
        R = synthetic.quat_to_rot(self.poses[c, :4])
        Xc = R @ np.asarray(X) + self.poses[c, 4:]
        l = np.cross(np.array([Xc[0] / Xc[2], Xc[1] / Xc[2], 1.0]), self.rng.uniform(-1, 1, 3))
        l /= np.linalg.norm(l[:2])
        self.rec.images[c].lines.append(FeatureLine(l, False, point_id))
        el = (c, len(self.rec.images[c].lines) - 1)
        if point_id >= 0:
            self.rec.points3D[point_id].track.append(el)
        return el

    def add_point(self, pid, X, cams, at=None):
        self.rec.points3D[pid] = Point3D(X if at is None else at)
        return [self.add_line(c, X, pid) for c in cams]

    def link(self, a, b):
        self.graph.AddCorrespondence(a[0], a[1], b[0], b[1]); self.graph.AddCorrespondence(b[0], b[1], a[0], a[1])


def test_forced_completion_conflict(oracle):
    """points 0 and 1 (the same place) both reach f1; f2 hangs on f1 only; f3 is point 1's own: the lower index takes f1 and f2, the loser's walk is redone on the
    host and keeps f3 only"""
    w = _World()
    X = np.array([0.1, -0.2, 0.3])
    a = w.add_point(0, X, [0, 1, 2, 3]); b = w.add_point(1, X, [4, 5, 6, 7], at=X + 1e-7)
    f1, f2, f3 = w.add_line(8, X), w.add_line(9, X), w.add_line(10, X)
    w.link(a[0], f1); w.link(b[0], f1); w.link(f1, f2); w.link(b[1], f3)
    reports, o = _compare((w.rec, w.graph), "c")
    assert o.completed == [(0, f1), (0, f2), (1, f3)]
    assert reports[0].conflict_replays == 1


def test_forced_merge_chain_and_stale_candidate(oracle):
    """0 + 1 -> 4, then (the recursion) 4 + 2 -> 5; point 3 lies elsewhere and its line corresponds to a line of point 0, which is gone by its turn.
    (4, 2), (4, 3) and (5, 3) are pairs the speculation never saw: each gets a launch of its own."""
    w = _World()
    X, Y = np.array([0.1, -0.2, 0.3]), np.array([-0.4, 0.3, 0.1])
    a = w.add_point(0, X, [0, 1, 2, 3]); b = w.add_point(1, X, [4, 5, 6, 7], at=X + 1e-7); c = w.add_point(2, X, [8, 9, 10, 11], at=X - 1e-7)
    e = w.add_point(3, Y, [0, 1, 2, 3])
    w.link(a[0], b[0]); w.link(b[1], c[0]); w.link(e[0], a[1])
    reports, o = _compare((w.rec, w.graph), "m")
    assert o.merged == [(0, 1, 4), (4, 2, 5)]
    assert reports[0].num_changed == 12 and reports[0].fresh_pair_launches == 3


def test_closure_larger_than_the_on_chip_list(oracle):
    w = _World()
    X = np.array([0.2, 0.1, -0.3])
    a = w.add_point(0, X, [0, 1, 2, 3])
    b = w.add_point(1, np.array([-0.5, 0.2, 0.4]), [0, 1, 2, 3])
    free = [w.add_line(4 + (i % 8), X) for i in range(700)]
    for f in free[:600]:
        w.link(a[0], f)
    for f, g in zip(free[600:], free[:100]):
        w.link(f, g)      # a second level behind the first 100
    w.link(b[0], free[0])
    reports, o = _compare((w.rec, w.graph), "c")
    assert len(o.completed) == 700 and all(p == 0 for p, _ in o.completed)
    assert reports[0].overflow_points == 1 and reports[0].second_launches >= 1


def test_closures_that_fit_on_chip_but_not_in_the_output_pool(oracle):
    """ten points at one place all reach the same 401 free lines (a hub line and 400 behind it): each closure fits the on-chip list, together they exceed the
    output pool (2 E + 1024 = 2664 entries), so the points that find it full are finished by the second launch; point 0 takes everything, the rest lose"""
    w = _World()
    X = np.array([0.2, 0.1, -0.3])
    tracks = [w.add_point(p, X, [0, 1, 2, 3], at=X + 1e-8 * p) for p in range(10)]
    hub = w.add_line(4, X)
    for i in range(400):
        w.link(hub, w.add_line(5 + (i % 7), X))
    for t in tracks:
        w.link(t[0], hub)
    reports, o = _compare((w.rec, w.graph), "c")
    assert len(o.completed) == 401 and all(p == 0 for p, _ in o.completed)
    assert reports[0].overflow_points > 0 and reports[0].second_launches >= 1 and reports[0].conflict_replays == 9


def test_more_partner_points_than_the_on_chip_candidate_list(oracle):
    """point 0's first line corresponds to a line of each of 300 other points (the on-chip list holds 256): its pairs are evaluated one by one.  299 partners lie
    elsewhere and fail; the last one is the same place, merges, and the merged point asks the 299 again"""
    w = _World()
    rng = np.random.default_rng(7)
    X = np.array([0.1, -0.2, 0.3])
    a = w.add_point(0, X, [0, 1, 2, 3])
    for p in range(1, 301):
        Y = X + 1e-7 if p == 300 else rng.uniform(-0.6, 0.6, 3)
        b = w.add_point(p, Y, [4 + (p % 8), 4 + ((p + 1) % 8), 4 + ((p + 2) % 8), 4 + ((p + 3) % 8)], at=Y)
        w.link(a[0], b[0])
    reports, o = _compare((w.rec, w.graph), "m")
    assert o.merged == [(0, 300, 301)]
    assert reports[0].overflow_points == 1 and reports[0].fresh_pair_launches == 300 + 299


# ---- the refinement loop -------------------------------------------------------------------------------------------------------------------

LOOP_CFG = (20, 300, 10, 4)


def _loop_world(eps=0.0, perturbation=0):
    """`eps`: the input points perturbed by eps relative, a normal draw per coordinate from the generator seeded with `perturbation`"""
    sc = synthetic.make_completion_scene(*LOOP_CFG[:3], seed=LOOP_CFG[3], line_noise_px=0.5, outlier_obs=0.05, quantise_float32=True)
    if eps:
        sc["points"] = sc["points"] * (1.0 + eps * np.random.default_rng(perturbation).standard_normal(sc["points"].shape))
    return reconstruction_from_completion_scene(sc)


def _mapper_options():
    o = IncrementalMapperOptions()
    o.print_summary = False
    return o


def test_loop_with_triangulator_equals_the_oracle_loop(oracle):
    """Per round the completed, merged and filtered sets equal the oracle loop's, the loop ends in the same round, and the reconstruction ends with more
    observations than the same scene refined without a triangulator.  No round excludes any observation from the comparison."""
    orec, ograph = _loop_world()
    want = tro.iterative_global_refinement(orec, ograph, _mapper_options())
    print("oracle loop: %d rounds, margin %.3e, completed %s merged %s filtered %s" % (want["num_rounds"], want["margin"], want["num_completed"], want["num_merged"], want["num_filtered"]))
    assert want["margin"] > 1e-4
    for k in (1, 2, 3):      # stable under three 1e-12 perturbations of the input points, the criterion of tests/test_gpu_global_refinement.py
        prec, pgraph = _loop_world(1e-12, k)
        assert tro.decisions(tro.iterative_global_refinement(prec, pgraph, _mapper_options())) == tro.decisions(want)
    rec, graph = _loop_world()
    rep = IterativeGlobalRefinement(rec, _mapper_options(), triangulator=IncrementalTriangulator(graph, rec))
    assert rep.num_rounds == want["num_rounds"]
    assert (rep.initial[0], rep.initial[1], rep.initial[2], rep.initial[3]) == want["initial"]
    assert rep.completed == want["completed"] and rep.merged == want["merged"]
    assert rep.num_completed == want["num_completed"] and rep.num_merged == want["num_merged"] and rep.num_filtered == want["num_filtered"]
    assert rep.obs_deleted == want["obs_deleted"] and rep.point_deleted == want["point_deleted"]
    assert rep.changed == want["changed"]
    assert rec._observations() == orec._observations()
    plain, _ = _loop_world()
    IterativeGlobalRefinement(plain, _mapper_options())
    assert rec.ComputeNumObservations() > plain.ComputeNumObservations()


def test_loop_without_triangulator_is_unchanged(oracle):
    """triangulator=None: the report equals the one of the loop as it was (AdjustGlobalBundle + FilterAllPoints3D per round, restated here)"""
    from privacy_preserving_sfm_amd.bundle_adjustment import AdjustGlobalBundle, GlobalBundleAdjustmentOptions
    sc = synthetic.make_ba_scene(12, 300, 6, seed=5, line_noise_px=0.5, outlier_obs=0.05, quantise_float32=True)
    rec, ref = Reconstruction.from_scene(sc), Reconstruction.from_scene(sc)
    rep = IterativeGlobalRefinement(rec, _mapper_options())
    options = _mapper_options()
    rounds, filtered, changed = 0, [], []
    for _ in range(options.ba_global_max_refinements):
        n = ref.ComputeNumObservations()
        AdjustGlobalBundle(ref, GlobalBundleAdjustmentOptions(len(ref.RegImageIds()), options))
        nf = ref.FilterAllPoints3D(options.filter_max_reproj_error, options.filter_min_tri_angle)
        rounds += 1; filtered.append(int(nf)); changed.append(float(nf) / n)
        if changed[-1] < options.ba_global_max_refinement_change:
            break
    assert (rep.num_rounds, rep.num_filtered, rep.changed) == (rounds, filtered, changed)
    assert rep.initial is None and rep.num_completed == [] and rep.merged == []
    assert rec._observations() == ref._observations()
    for p in rec.points3D:
        assert np.array_equal(rec.points3D[p].xyz, ref.points3D[p].xyz)
