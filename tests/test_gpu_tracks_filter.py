"""pp_tracks_filter_points / pp_tracks_filter_negative_depth / pp_tracks_filter_images (K14) on a live tracks handle against the plain-Python reference
(tests/tracks_filter_reference.py), for every scene of tests/tracks_filter_scenes.py and every operation of it, one after the other on ONE handle.
Exact: the event list, num_filtered, the other counts, pp_tracks_get_state (line_point, deleted, tracks).  point_error: rtol 1e-9, atol 1e-12 (the bound of
test_filter_points3d_matches_oracle for this quantity; the summation order on the device is free).  Every decision keeps a relative margin above 1e-6 from its
threshold (tests/test_tracks_filter_reference.py asserts it on the CPU), so the device has no legitimate reason to decide otherwise.
Afterwards the handle is still a handle: pp_tracks_complete and pp_tracks_find_next_images on it equal those of a fresh handle flattened from the filtered
reconstruction; and a PP_ERR_INVALID call leaves pp_tracks_get_state as it was."""
import numpy as np
import pytest

import tracks_filter_reference as ref
import tracks_filter_scenes as scenes
from privacy_preserving_sfm_amd import _capi
from privacy_preserving_sfm_amd.device import TracksProblem
from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator

pytestmark = pytest.mark.gpu


def _tracks(state):
    ts, tl = state["track_start"], state["track_line"]
    return [[int(l) for l in tl[ts[p]:ts[p + 1]]] for p in range(len(ts) - 1)]


def _assert_state(pb, ix):
    line_point, deleted, tracks = ix.state()
    st = pb.state()
    assert np.array_equal(st["line_point"], line_point) and np.array_equal(st["deleted"], deleted) and _tracks(st) == tracks


def _run_op(pb, ix, op):
    """the handle's call for one op (on the state before it) -> (report, events, point_error | None, filtered | None)"""
    kind, kw = op
    if kind == "points":
        rep, events, pe = pb.filter_points(kw.get("max_reproj_error", 4.0), kw.get("min_tri_angle", 1.5), ix.flat["line_aligned"],
                                           point_subset=ix.point_flags(kw.get("point3D_ids")), image_subset=ix.image_flags(kw.get("image_ids")))
        return rep, events, pe, None
    if kind == "depth":
        rep, events = pb.filter_negative_depth(ix.image_order())
        return rep, events, None, None
    rep, events, filtered = pb.filter_images(ix.image_order())
    return rep, events, None, filtered


@pytest.mark.parametrize("name,build", scenes.all_scenes(), ids=[n for n, _ in scenes.all_scenes()])
def test_handle_equals_the_reference_and_stays_usable(name, build):
    rec, graph, ops, _ = build()
    ix = ref.Indexed(rec, graph)
    pb = TracksProblem(ix.flat)
    try:
        for op in ops:
            rep, events, pe, filtered = _run_op(pb, ix, op)      # (reads the reconstruction before the reference changes it)
            got = ref.run_op(rec, op)
            print(name, op[0], "num_filtered", rep.num_filtered, got["num_filtered"], "events", len(events), "device_ms %.3f" % rep.device_ms)
            assert [(int(p), int(l)) for p, l in events] == ix.events(got["events"])
            assert rep.num_entries == len(got["events"])
            assert (rep.num_filtered, rep.num_points_deleted, rep.num_observations_deleted) == (got["num_filtered"], got["point_deleted"], got["obs_deleted"])
            if op[0] == "points":
                assert rep.points_tested == got["tested"]
                want = np.full(len(ix.point_ids), -1.0)
                for pid, e in got["errors"].items():
                    want[ix.point_index[pid]] = e
                assert np.array_equal(pe == -1.0, want == -1.0)
                assert np.allclose(pe, want, rtol=1e-9, atol=1e-12)
            if op[0] == "images":
                assert [int(c) for c in filtered] == [ix.image_index[i] for i in got["filtered"]] and rep.images_filtered == len(filtered)
            _assert_state(pb, ix)
        # the handle after the filters against a fresh one over the filtered reconstruction (its points renumbered: compared by id)
        fresh_flat, fresh_ids, _ = IncrementalTriangulator(graph, rec).flatten()
        fresh = TracksProblem(fresh_flat)
        try:
            a, b = pb.find_next_images(), fresh.find_next_images()
            assert (a[0].num_ranked, a[0].num_first_bucket, a[0].num_unregistered) == (b[0].num_ranked, b[0].num_first_bucket, b[0].num_unregistered)
            assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
            (ra, pa), (rb, pb_) = pb.complete(), fresh.complete()
            assert ra.num_changed == rb.num_changed
            assert [(ix.point_ids[int(p)], int(l)) for p, l in pa] == [(fresh_ids[int(p)], int(l)) for p, l in pb_]
        finally:
            fresh.close()
    finally:
        pb.close()


def test_invalid_calls_leave_the_state_unchanged():
    rec, graph, ops, _ = scenes.registration_order()
    rec.images[5].registered = False
    ix = ref.Indexed(rec, graph)
    pb = TracksProblem(ix.flat)
    try:
        before = pb.state()
        order = ix.image_order()
        P, C = len(ix.point_ids), len(ix.image_ids)

        def invalid(call):
            with pytest.raises(_capi.PPError) as e:
                call()
            assert e.value.code == _capi.PP_ERR_INVALID
            after = pb.state()
            assert all(np.array_equal(before[k], after[k]) for k in before)

        invalid(lambda: pb.filter_points(4.0, 1.5, point_subset=np.ones(P, dtype=np.uint8), image_subset=np.ones(C, dtype=np.uint8)))
        invalid(lambda: pb.filter_points(-4.0, 1.5))
        invalid(lambda: pb.filter_points(4.0, -1.5))
        invalid(lambda: pb.filter_negative_depth(order[:-1]))                     # one registered image is missing
        invalid(lambda: pb.filter_negative_depth(order[:-1] + [order[0]]))        # one is listed twice
        invalid(lambda: pb.filter_negative_depth(order + [ix.image_index[5]]))    # an unregistered one is listed
        invalid(lambda: pb.filter_negative_depth(order[:-1] + [C]))               # out of range
        invalid(lambda: pb.filter_images(order[1:]))
        invalid(lambda: pb.filter_images([]))
        # and the valid call still does its work
        rep, events = pb.filter_negative_depth(order)
        got = ref.run_op(rec, ("depth", {}))
        assert [(int(p), int(l)) for p, l in events] == ix.events(got["events"]) and rep.num_filtered == got["num_filtered"] == 4
    finally:
        pb.close()
