"""pp_tracks_triangulate_image / pp_tracks_complete_image on the device against the sequential oracle (tests/tracks_image_reference.py): EXACT equality
of the event list, num_changed, the final line_point, the tracks and the deleted flags; new-point positions within 1e-8 absolute (unit-scale scenes,
the bound of tests/test_gpu_triangulation.py for device against oracle).

The device and the oracle round differently far below 1e-6 relative, so every scene was picked on the CPU with the oracle alone for a margin above 1e-6
(the bound of tests/test_gpu_tracks.py) and no RANSAC whose winner is arbitrary (support 3 of more than 3); each test asserts both, and that the scene
creates, continues and - where intended - conflicts.  No candidate is left out of any comparison.  Scenes: tests/tracks_image_scenes.py."""
import copy

import numpy as np
import pytest

import tracks_image_reference as tir
import tracks_image_scenes as scenes
from privacy_preserving_sfm_amd.device import TracksProblem, tracks_image_options, tracks_options
from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator

pytestmark = pytest.mark.gpu


def _check_state(pb, rec, line_ref, initial):
    st = pb.state()
    want_lp = np.array([rec.images[i].lines[k].Point3DId() for (i, k) in line_ref], dtype=np.int32)
    assert np.array_equal(st["line_point"], want_lp)
    P = len(st["deleted"])
    assert sorted(rec.points3D) == [p for p in range(P) if not st["deleted"][p]]
    for p, pt in rec.points3D.items():
        if p < initial:
            assert np.array_equal(st["points"][p], pt.xyz)
        assert np.abs(st["points"][p] - pt.xyz).max() <= 1e-8, (p, st["points"][p], pt.xyz)
        assert [line_ref[l] for l in st["track_line"][st["track_start"][p]:st["track_start"][p + 1]]] == pt.track


def _compare(world, image_id, ops, **option_kw):
    """`ops`: t / T TriangulateImage at max_transitivity 1 / 2, c CompleteImage, C pp_tracks_complete, M pp_tracks_merge - on one handle and on the
    oracle over a copy; -> (reports, oracle)"""
    rec, graph = world
    orec = copy.deepcopy(rec)
    oracle = tir.ImageOracle(graph, orec)
    flat, point_ids, line_ref = IncrementalTriangulator(graph, rec).flatten()
    assert point_ids == list(range(len(point_ids)))
    image = sorted(rec.images).index(image_id)
    pb = TracksProblem(flat)
    reports = []
    try:
        for op in ops:
            oo = tir.Options(max_transitivity=2 if op == "T" else 1, **option_kw)
            if op in "tTc":
                do = tracks_image_options(**{k: (int(v) if isinstance(v, bool) else v) for k, v in vars(oo).items() if hasattr(tracks_image_options(), k)})
                e0 = len(oracle.events)
                n = oracle.CompleteImage(oo, image_id) if op == "c" else oracle.TriangulateImage(oo, image_id)
                rep, events = pb.complete_image(image, do) if op == "c" else pb.triangulate_image(image, do, flat["line_aligned"])
                print("op %s: changed %d, created %d, continued %d, redone %d (%d fresh launches), device %.3f ms replay %.3f ms total %.3f ms" %
                      (op, rep.num_changed, rep.points_created, rep.lines_continued, rep.lines_redone, rep.fresh_launches, rep.device_ms, rep.replay_ms, rep.total_ms))
                assert [(int(p), line_ref[l]) for p, l in events] == oracle.events[e0:]
                assert rep.num_changed == n and rep.num_entries == len(oracle.events) - e0
            else:
                do = tracks_options(merge_max_reproj_error=oo.merge_max_reproj_error, complete_max_reproj_error=oo.complete_max_reproj_error,
                                    complete_max_transitivity=oo.complete_max_transitivity)
                n = oracle.CompleteTracks(oo) if op == "C" else oracle.MergeTracks(oo)
                rep, _ = pb.complete(do) if op == "C" else pb.merge(do)
                assert rep.num_changed == n
            reports.append(rep)
            _check_state(pb, orec, line_ref, len(point_ids))
    finally:
        pb.close()
    print("oracle margin %.3e, %d RANSACs, %d arbitrary" % (oracle.margin, oracle.num_ransacs, oracle.arbitrary))
    assert oracle.margin > 1e-6 and oracle.arbitrary == 0
    return reports, oracle


@pytest.mark.parametrize("spec", scenes.SYNTHETIC, ids=lambda s: "%dx%dx%d" % s["cfg"])
def test_synthetic_scene(spec, oracle):
    """TriangulateImage at transitivity 1, pp_tracks_complete and pp_tracks_merge in between, TriangulateImage at 2, CompleteImage - on one handle"""
    reports, o = _compare(scenes.synthetic_world(spec["cfg"], spec["seed"], spec["image"]), spec["image"], "tCMTc")
    t1, _, _, t2, c = reports
    assert t1.points_created > 0 and t1.lines_continued > 0 and t2.points_created > 0 and t2.lines_continued > 0
    assert t1.lines_redone + t2.lines_redone > 0 and c.num_changed > 0
    assert t1.ransac_trials > 0


@pytest.mark.parametrize("scene", scenes.HAND_BUILT, ids=lambda f: f.__name__)
def test_hand_built_scene(scene, oracle):
    w, want = scene()
    ops = "".join(("T" if want.get("transitivity") == 2 else "t") if op == "t" else op for op in want["ops"])
    before = IncrementalTriangulator(w.graph, w.rec).flatten()[0]["line_point"].copy()
    reports, o = _compare((w.rec, w.graph), want["image"], ops, **scenes.TIGHT)
    assert o.events == want["events"]
    assert sum(r.num_changed for r in reports) == want["num_changed"]
    assert sum(r.lines_redone for r in reports) == want["redone"]
    if want["redone"]:
        assert sum(r.fresh_launches for r in reports) >= want["redone"]


def test_complete_image_conflicts(oracle):
    """CompleteImage: r0 has point 0 whose completion takes r1 (free at the snapshot, with a speculative point of its own): at r1 the reference completes
    point 0 AGAIN - a track that grew since the snapshot, so K10a runs afresh; r2's 20-line set carries r-short's min_num_trials"""
    w = scenes.World()
    a = w.add_point(0, scenes.X, [1, 2, 3, 4])
    r0 = w.add_line(0, scenes.X, 0)
    r1 = w.add_line(0, scenes.X)
    w.link(r0, r1)
    f = [w.add_line(c, scenes.X) for c in (5, 6, 7)]
    for g in f:
        w.link(r1, g)
    r2 = w.add_line(0, scenes.Y)
    for c in (5, 6, 7):
        w.link(r2, w.add_line(c, scenes.Y))
    r3 = w.add_line(0, scenes.Z)
    for i in range(20):
        w.link(r3, w.add_line(1 + (i % 11), scenes.Z))
    reports, o = _compare((w.rec, w.graph), 0, "c", **scenes.TIGHT)
    assert o.events[:4] == [(0, r1)] + [(0, g) for g in f]
    assert reports[0].lines_redone >= 1 and reports[0].points_created == 2 and reports[0].num_changed == 4 + 4 + 21


def test_mirror_updates_the_reconstruction(oracle):
    """IncrementalTriangulator.TriangulateImage / CompleteImage apply the events to the Reconstruction: the same state as the oracle's"""
    spec = scenes.SYNTHETIC[0]
    rec, graph = scenes.synthetic_world(spec["cfg"], spec["seed"], spec["image"])
    orec = copy.deepcopy(rec)
    o = tir.ImageOracle(graph, orec)
    tri = IncrementalTriangulator(graph, rec)
    opt = IncrementalTriangulator.Options()
    assert tri.TriangulateImage(opt, spec["image"]) == o.TriangulateImage(tir.Options(), spec["image"])
    assert tri.CompleteImage(opt, spec["image"]) == o.CompleteImage(tir.Options(), spec["image"])
    got, want = tir.tr.state(rec), tir.tr.state(orec)
    assert got[1] == want[1] and sorted(got[0]) == sorted(want[0])
    for p in want[0]:
        assert got[0][p][1] == want[0][p][1] and np.abs(np.array(got[0][p][0]) - np.array(want[0][p][0])).max() <= 1e-8
    assert tri.GetModifiedPoints3D() >= set(o.created)
