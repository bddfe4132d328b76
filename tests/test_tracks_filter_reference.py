"""The plain-Python reference of the deletions on a live tracks handle (tests/tracks_filter_reference.py) against hand-written expectations, one rule per
scene (tests/tracks_filter_scenes.py), and on the corrupted synthetic worlds: every rule fires, and every tested pixel error and angle keeps a relative
margin above 1e-6 - the project's bound (tests/test_gpu_tracks.py) - from its threshold, so that the device cannot legitimately decide otherwise.  CPU only."""
import numpy as np
import pytest

import tracks_filter_reference as ref
import tracks_filter_scenes as scenes

MARGIN = 1e-6


def _consistent(rec):
    """tracks and lines agree"""
    for pid, point in rec.points3D.items():
        assert len(set(point.track)) == len(point.track)
        for (iid, idx) in point.track:
            assert rec.images[iid].lines[idx].Point3DId() == pid
    n = sum(len(p.track) for p in rec.points3D.values())
    assert n == rec.ComputeNumObservations()


@pytest.mark.parametrize("scene", scenes.HAND_BUILT, ids=lambda f: f.__name__)
def test_hand_built_scene_gives_the_hand_written_outcome(scene):
    rec, _, ops, expect = scene()
    for op, want in zip(ops, expect):
        points_before = set(rec.points3D)
        got = ref.run_op(rec, op)
        print(scene.__name__, op[0], {k: v for k, v in got.items() if k.startswith("margin")})
        assert got["events"] == want["events"]
        assert got["num_filtered"] == want["num_filtered"]
        assert got["point_deleted"] == sum(1 for e in want["events"] if e[1] is None)
        assert sorted(points_before - set(rec.points3D)) == sorted(e[0] for e in want["events"] if e[1] is None)
        if op[0] == "points":
            assert sorted(got["errors"]) == want["errors"]
            assert got["by_angle"] == want.get("by_angle", 0)
            assert all(0.0 <= e < 1e-6 or e <= op[1].get("max_reproj_error", 4.0) for e in got["errors"].values())
            assert got["margin_error"] > MARGIN and got["margin_angle"] > MARGIN
        if op[0] == "depth":
            assert got["margin_depth"] > MARGIN
        if op[0] == "images":
            assert got["filtered"] == want["filtered"]
            assert all(not rec.images[i].registered for i in want["filtered"])
        _consistent(rec)


def test_the_sufficient_pair_of_the_far_point_needs_the_deleted_element():
    rec, _, ops, _ = scenes.angle_needs_deleted_element()
    X, min_rad = rec.points3D[0].xyz, np.deg2rad(ops[0][1]["min_tri_angle"])
    c = {i: ref.projection_center(rec.images[i]) for (i, _) in rec.points3D[0].track}
    enough = [(a, b) for a in c for b in c if a < b and ref.triangulation_angle(c[a], c[b], X) >= min_rad]
    assert enough == [(6, 14)]
    assert not np.isfinite(ref.squared_line_error(rec, 6, 0, X))      # outside image 6: that element goes first


def test_the_only_sufficient_pair_of_many_pairs_is_the_last_one():
    """pair (i1, i2 < i1) has index i1 (i1 - 1) / 2 + i2 in the order the kernel's lanes walk: 252 of 253, in the fourth chunk of 64"""
    rec, _, ops, _ = scenes.many_pairs()
    X, min_rad = rec.points3D[0].xyz, np.deg2rad(ops[0][1]["min_tri_angle"])
    c = [ref.projection_center(rec.images[i]) for (i, _) in rec.points3D[0].track]
    enough = [i1 * (i1 - 1) // 2 + i2 for i1 in range(len(c)) for i2 in range(i1) if ref.triangulation_angle(c[i1], c[i2], X) >= min_rad]
    assert len(c) == 23 and enough == [252]
    assert max(ref.triangulation_angle(a, b, X) for a in c for b in c) < np.deg2rad(1.5)


def test_a_track_of_three_survives_the_package_rule_but_not_the_reference_rule():
    """Reconstruction.DeleteObservation (kept as it is) removes one element; the reference's rule, transcribed in delete_observation, takes the point"""
    rec, _, _, _ = scenes.depth_track3_one_flag()
    rec.DeleteObservation(0, 0)
    assert len(rec.points3D[0].track) == 2
    rec, _, _, _ = scenes.depth_track3_one_flag()
    events = []
    assert ref.delete_observation(rec, 0, 0, events) == 3 and events == [(0, None)] and 0 not in rec.points3D


@pytest.mark.parametrize("spec", scenes.SYNTHETIC, ids=lambda s: "%dx%dx%d" % s["cfg"])
def test_corrupted_world_fires_every_rule_with_margin(spec):
    rec, _, ops, _ = scenes.corrupted_world(spec)
    num_points = len(rec.points3D)
    margin_error = margin_angle = np.inf
    totals = dict(point_deleted=0, by_angle=0, elements_on_survivors=0, depth=0, errors=0)
    for op in ops:
        got = ref.run_op(rec, op)
        _consistent(rec)
        if op[0] == "points":
            margin_error, margin_angle = min(margin_error, got["margin_error"]), min(margin_angle, got["margin_angle"])
            totals["point_deleted"] += got["point_deleted"]
            totals["elements_on_survivors"] += sum(1 for e in got["events"] if e[1] is not None)
            totals["errors"] += len(got["errors"])
            totals["by_angle"] += got["by_angle"]
        elif op[0] == "depth":
            totals["depth"] += got["num_filtered"]
            assert got["margin_depth"] > MARGIN
    print(spec["cfg"], "margin_error %.3e margin_angle %.3e" % (margin_error, margin_angle), totals, "of", num_points, "points;", len(rec.points3D), "left")
    assert margin_error > MARGIN and margin_angle > MARGIN
    assert abs(margin_error - spec["margin_error"]) <= 1e-2 * spec["margin_error"] and abs(margin_angle - spec["margin_angle"]) <= 1e-2 * spec["margin_angle"]
    assert totals["depth"] > 0 and totals["point_deleted"] > 5 and totals["elements_on_survivors"] > 3
    assert len(rec.points3D) > num_points // 3      # some points survive
