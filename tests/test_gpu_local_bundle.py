"""pp_tracks_find_local_bundle (K12) and pp_tracks_update on the device against the plain-Python FindLocalBundle (tests/local_bundle_reference.py).

EXACT equality of every decision: the bundle in the reference's order, the sorted overlap list with its counts, NumPoints3D, the threshold level, the
fill-up count, the number of lazily computed angles and the -1 pattern of the angles that were never asked for.  The computed angles agree within
1e-10 rad absolute: the argument of acos carries a few ulp (about 4e-16 relative) and acos amplifies by 1 / sin(theta); every compared angle is at
least 0.1 degree (asserted), so the error is at most 4e-16 / sin(0.1 deg) = 2.3e-13 - the bound has about 400 x headroom.  Every scene's `margin`
(smallest relative distance of a compared angle from its threshold) is asserted above 1e-6, the bound of tests/test_gpu_tracks.py; no case is left
out of any comparison."""
import copy
import math

import numpy as np
import pytest

import local_bundle_reference as ref
import local_bundle_scenes as scenes
import tracks_image_scenes as tis
from privacy_preserving_sfm_amd import _capi
from privacy_preserving_sfm_amd.device import TracksProblem, local_bundle_options, tracks_options
from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator

pytestmark = pytest.mark.gpu

ANGLE_TOL = 1e-10
MIN_COMPARED_ANGLE = math.radians(0.1)


def _flatten(rec, graph):
    flat, point_ids, line_ref = IncrementalTriangulator(graph, rec).flatten()
    assert sorted(rec.images) == list(range(len(rec.images))) and point_ids == sorted(rec.points3D)      # image id = image index in these scenes
    return flat


def _check(pb, rec, image, num_images, min_tri_angle=6.0):
    """one device call against the reference -> (report, bundle, overlap, reference result)"""
    want = ref.find_local_bundle(rec, ref.Options(num_images, min_tri_angle), image)
    rep, bundle, overlap = pb.find_local_bundle(image, local_bundle_options(local_ba_num_images=num_images, local_ba_min_tri_angle=min_tri_angle))
    print("image %d: N %d overlapping %d computed %d used %d level %d filled %d margin %.3e" %
          (image, rep.num_points3D, rep.num_overlapping, rep.angles_computed, rep.angles_used, rep.threshold_level, rep.filled, want["margin"]))
    assert want["margin"] > 1e-6
    assert list(bundle) == want["bundle"] and rep.num_selected == len(want["bundle"])
    assert list(zip(overlap["image"].tolist(), overlap["count"].tolist())) == want["overlap"] and rep.num_overlapping == len(want["overlap"])
    assert (rep.num_points3D, rep.threshold_level, rep.filled, rep.angles_used) == (want["num_points3D"], want["level"], want["filled"], want["lazy"])
    assert rep.angles_computed >= rep.angles_used
    got, exp = overlap["tri_angle"], np.array(want["tri_angle"], dtype=np.float64).reshape(-1)
    assert np.array_equal(got == -1.0, exp == -1.0)
    asked = exp != -1.0
    if asked.any():
        assert exp[asked].min() >= MIN_COMPARED_ANGLE
        err = np.abs(got[asked] - exp[asked]).max()
        print("  largest angle difference %.3e rad" % err)
        assert err <= ANGLE_TOL
    return rep, bundle, overlap, want


@pytest.mark.parametrize("scene", scenes.SCENES, ids=lambda f: f.__name__)
def test_scene_equals_the_reference(scene):
    w, expect = scene()
    pb = TracksProblem(_flatten(w.rec, w.graph))
    try:
        rep, bundle, overlap, want = _check(pb, w.rec, expect["image"], expect["options"]["local_ba_num_images"], expect["options"]["local_ba_min_tri_angle"])
    finally:
        pb.close()
    assert list(bundle) == expect["bundle"]      # the hand-written expectation too
    assert (rep.threshold_level, rep.filled, rep.angles_used, rep.num_points3D) == (expect["level"], expect["filled"], expect["lazy"], expect["num_points3D"])
    if expect["level"] < 0:
        assert rep.angles_computed == 0      # the early return and N = 0: K12b does not run


@pytest.mark.parametrize("world", tis.SYNTHETIC, ids=lambda s: "%dx%dx%d" % s["cfg"])
@pytest.mark.parametrize("num_images", [6, 3])
def test_synthetic_worlds_every_image(world, num_images):
    """the ring geometry lets every angle pass (checked on the CPU with the reference alone): the bundle is the top of the sorted overlap list, so this
    covers the counting kernel and the sort on tracks of every length the scene has"""
    rec, graph = tis.synthetic_world(world["cfg"], world["seed"], world["image"])
    pb = TracksProblem(_flatten(rec, graph))
    try:
        some = 0
        for image in sorted(rec.images):
            rep, bundle, overlap, want = _check(pb, rec, image, num_images)
            assert list(bundle) == [iid for iid, _ in want["overlap"]][: len(bundle)] and rep.filled == 0
            some += rep.num_overlapping > 0
        assert some >= len(rec.images) - 1
    finally:
        pb.close()


def _same_result(a, b):
    (ra, ba, oa), (rb, bb, ob) = a, b
    fields = ("num_points3D", "num_overlapping", "num_selected", "angles_computed", "angles_used", "threshold_level", "filled")
    return (all(getattr(ra, f) == getattr(rb, f) for f in fields) and np.array_equal(ba, bb) and
            all(np.array_equal(oa[k], ob[k]) for k in ("image", "count", "tri_angle")))      # the angles BIT-equal: same kernel, same inputs


def _same_state(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("line_point", "points", "deleted", "track_start", "track_line"))


def test_twice_in_a_row_and_the_state_is_untouched():
    w, expect = scenes.relax()
    pb = TracksProblem(_flatten(w.rec, w.graph))
    try:
        before = pb.state()
        o = local_bundle_options(**expect["options"])
        first, second = pb.find_local_bundle(0, o), pb.find_local_bundle(0, o)
        assert _same_result(first, second) and list(first[1]) == expect["bundle"]
        assert _same_state(before, pb.state())
    finally:
        pb.close()


def _moved(flat, seed=5):
    """two poses, ten points and the intrinsics of camera 0, slightly moved -> (image_idx, poses, point_idx, xyz, intr)"""
    rng = np.random.default_rng(seed)
    C, P = flat["poses"].shape[0], flat["points"].shape[0]
    ii = np.array([1, C - 2], dtype=np.int32)
    poses = flat["poses"][ii].copy()
    poses[:, :4] += rng.normal(0, 1e-3, (2, 4)); poses[:, 4:] += rng.normal(0, 1e-2, (2, 3))      # (not normalised: the handle normalises, as at create)
    pi = rng.choice(P, 10, replace=False).astype(np.int32)
    xyz = flat["points"][pi] + rng.normal(0, 1e-3, (10, 3))
    intr = flat["intr"].copy()
    intr[0, 0] *= 1.0005
    return ii, poses, pi, xyz, intr


def _run_all(pb, image):
    out = [pb.find_local_bundle(image, local_bundle_options(local_ba_num_images=4))]
    rep, pairs = pb.complete(tracks_options())
    out.append((int(rep.num_changed), int(rep.num_entries), pairs.tolist()))
    rep, merges = pb.merge(tracks_options())
    out.append((int(rep.num_changed), int(rep.num_entries), merges.tolist()))
    out.append(pb.find_local_bundle(image, local_bundle_options(local_ba_num_images=4)))
    return out, pb.state()


def test_update_equals_a_fresh_handle():
    world = tis.SYNTHETIC[0]
    rec, graph = tis.synthetic_world(world["cfg"], world["seed"], world["image"])
    flat = _flatten(rec, graph)
    ii, poses, pi, xyz, intr = _moved(flat)
    image = (world["image"] + 1) % len(rec.images)      # (the world's own image has no points: its lines were freed)
    pb = TracksProblem(flat)
    try:
        old = pb.find_local_bundle(image, local_bundle_options(local_ba_num_images=4))
        before = pb.state()
        pb.update()      # nothing in it: nothing changes
        assert _same_state(before, pb.state()) and _same_result(old, pb.find_local_bundle(image, local_bundle_options(local_ba_num_images=4)))
        pb.update(ii, poses, pi, xyz, intr, flat["camera_skip"])
        got, got_state = _run_all(pb, image)
    finally:
        pb.close()
    fresh = dict(flat, poses=flat["poses"].copy(), points=flat["points"].copy(), intr=intr)
    fresh["poses"][ii] = poses
    fresh["points"][pi] = xyz
    pf = TracksProblem(fresh)
    try:
        want, want_state = _run_all(pf, image)
    finally:
        pf.close()
    assert _same_result(got[0], want[0]) and got[1] == want[1] and got[2] == want[2] and _same_result(got[3], want[3])
    assert _same_state(got_state, want_state)
    assert got[1][0] > 0      # the completion had work to do on the moved state
    assert not np.array_equal(old[2]["tri_angle"], got[0][2]["tri_angle"])      # and the moved poses and points were seen


def test_invalid_arguments_leave_the_handle_as_it_was():
    w, expect = scenes.strict()
    w.rec.images[5].registered = False
    flat = _flatten(w.rec, w.graph)
    C, P, K = flat["poses"].shape[0], flat["points"].shape[0], flat["intr"].shape[0]
    pose, X = flat["poses"][:1].copy(), flat["points"][:1].copy()
    nan_pose, nan_X, nan_intr = pose.copy(), X.copy(), flat["intr"].copy()
    nan_pose[0, 5], nan_X[0, 1], nan_intr[0, 0] = np.nan, np.inf, np.nan
    pb = TracksProblem(flat)
    try:
        o = local_bundle_options(**expect["options"])
        good, state = pb.find_local_bundle(0, o), pb.state()
        assert list(good[1]) == expect["bundle"]
        calls = [lambda: pb.find_local_bundle(C, o), lambda: pb.find_local_bundle(-1, o),
                 lambda: pb.find_local_bundle(5, o),      # unregistered: the reference CHECKs it
                 lambda: pb.find_local_bundle(0, local_bundle_options(local_ba_num_images=1)),
                 lambda: pb.find_local_bundle(0, local_bundle_options(local_ba_min_tri_angle=-1.0)),
                 lambda: pb.update([C], pose), lambda: pb.update([-1], pose), lambda: pb.update([0], nan_pose),
                 lambda: pb.update((), None, [P], X), lambda: pb.update((), None, [-1], X), lambda: pb.update((), None, [0], nan_X),
                 lambda: pb.update([0], pose + 1.0, [0], nan_X),      # the bad point keeps the good pose out too
                 lambda: pb.update(intr=nan_intr)]
        for k, call in enumerate(calls):
            with pytest.raises(_capi.PPError) as e:
                call()
            assert e.value.code == _capi.PP_ERR_INVALID, k
            assert _same_result(good, pb.find_local_bundle(0, o)) and _same_state(state, pb.state()), k
    finally:
        pb.close()
    # a deleted point: a handle whose point 0 has an empty track
    w2, _ = scenes.strict(8)
    w2.rec.points3D[99] = type(w2.rec.points3D[0])(np.array([0.0, 0.0, 5.0]))
    flat2 = _flatten(w2.rec, w2.graph)
    dead = len(flat2["points"]) - 1
    p2 = TracksProblem(flat2)
    try:
        assert p2.state()["deleted"][dead] == 1
        with pytest.raises(_capi.PPError) as e:
            p2.update((), None, [dead], X)
        assert e.value.code == _capi.PP_ERR_INVALID
        p2.update((), None, [0], X)      # a live point is fine
        assert np.array_equal(p2.state()["points"][0], X[0])
    finally:
        p2.close()
