"""pp_tracks_bundle_setup (K16): BundleAdjuster::SetUp on a live tracks handle.  `BundleAdjuster.flatten_on(session)` must return what
`BundleAdjuster.flatten(reconstruction)` returns: every array compared with np.array_equal, the three index dictionaries equal in content and iteration
order.  No tolerance anywhere: integer logic and copies.  (tests/bundle_setup_worlds.py holds the worlds and the comparison.)

The shapes are the smallest at which the kernels can still go wrong: pass-A sizes around the wavefront (64), the line workgroups (256), the scan's
workgroup (1024: M = 1024 / 1025 observations, L = 1024 / 1026 lines) and the length above which a scan goes in tiles of 1024 (4096: with n = 2048 / 2049
L = 4096 / 4098 - the last of five tiles holds two elements -, with n = 4096 / 4097 M = 4096 / 4097 beside L = 8192 / 8194); tracks of 63 / 64 / 65 / 68
out-of-config elements around the 64-element chunk of the track walk; one config that has every bookkeeping case at once; the global config; a handle
that lived through the eight-image loop."""
import ctypes as C

import numpy as np
import pytest

import bundle_setup_worlds as bsw
import incremental_registration_scene as irs
from privacy_preserving_sfm_amd import _capi
from privacy_preserving_sfm_amd import bundle_adjustment as ba
from privacy_preserving_sfm_amd.bundle_adjustment import (BundleAdjuster, BundleAdjustmentConfig, FeatureLine, IncrementalMapperOptions,
                                                           IterativeGlobalRefinement, IterativeLocalRefinement)
from privacy_preserving_sfm_amd.incremental_mapper import IncrementalMapper
from privacy_preserving_sfm_amd.incremental_triangulator import CorrespondenceGraph, IncrementalTriangulator

pytestmark = pytest.mark.gpu


def _session(rec):
    tri = IncrementalTriangulator(CorrespondenceGraph(), rec)
    return tri._open(tri.Options())


def _compare(rec, cfg, opt):
    """both routes on the same reconstruction -> flatten()'s result"""
    want = bsw.flatten_and_restore(BundleAdjuster(opt, cfg), rec)
    ses = _session(rec)
    try:
        got = BundleAdjuster(opt, cfg).flatten_on(ses)
        rep = ses.last_bundle_setup_report
    finally:
        ses.close()
    bsw.assert_same_flatten(got, want)
    return want, rep


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097])
def test_pass_a_sizes(n):
    rec = bsw.world(2, n, 2)
    cfg = BundleAdjustmentConfig()
    cfg.AddImage(1)
    want, rep = _compare(rec, cfg, bsw.options(False))
    assert rep.num_obs == rep.num_config_obs == n and rep.num_points == n and rep.num_poses == rep.num_config_poses == 1 and rep.bad_line == -1
    assert want[0]["point_const"].all()      # every point is also seen from image 0, outside the config


def test_no_observation_is_none_on_both_routes():
    rec = bsw.world(3, 20, 3)
    bsw.strip_image(rec, 1)
    cfg = BundleAdjustmentConfig()
    cfg.AddImage(1)
    want, rep = _compare(rec, cfg, bsw.options(False))
    assert want is None and rep.num_obs == 0 and rep.num_poses == 0 and rep.num_points == 0


@pytest.fixture(scope="module")
def long_tracks():
    return bsw.world(70, 5, 70)


@pytest.mark.parametrize("num_config,outside", [(7, 63), (6, 64), (5, 65), (2, 68)])
def test_track_chunks(long_tracks, num_config, outside):
    rec = long_tracks
    cfg = BundleAdjustmentConfig()
    for i in range(num_config):
        cfg.AddImage(3 * i)      # (not the first images: the out-of-config elements lie on both sides of a chunk's border)
    for pid in rec.points3D:
        cfg.AddVariablePoint(pid)
    want, rep = _compare(rec, cfg, bsw.options(False))
    assert rep.num_config_obs == 5 * num_config and rep.num_obs == 5 * 70 and rep.num_poses == 70 and rep.num_config_poses == num_config
    assert (rep.num_obs - rep.num_config_obs) // 5 == outside
    assert not want[0]["point_const"].any()


@pytest.mark.parametrize("refine", [False, True], ids=["refine_off", "focal_extra"])
def test_bookkeeping(refine):
    rec, cfg = bsw.bookkeeping_world()
    want, rep = _compare(rec, cfg, bsw.options(refine))
    scene, pose_index, point_index, cam_index = want
    # the config is what it is meant to be
    assert 4 not in pose_index and list(pose_index)[:3] == [0, 1, 3] and rep.num_config_poses == 3 and rep.num_poses > 3
    num_a = int(rep.num_config_obs)
    first_b = [pid for pid, k in point_index.items() if k > scene["obs_point"][:num_a].max()]
    assert first_b and all(cfg.HasPoint(p) for p in first_b)                                       # a listed point with no observation in the config
    inside = bsw.points_of(rec, 0)[0]
    assert cfg.HasVariablePoint(inside) and not scene["point_const"][point_index[inside]]          # all its observations lie in the config
    both = [p for p in cfg.VariablePoints() if cfg.HasConstantPoint(p)]
    assert both and all(scene["point_const"][point_index[p]] for p in both)
    assert all(scene["point_const"][point_index[p]] for p in cfg.ConstantPoints())
    unlisted = [p for p in point_index if not cfg.HasPoint(p)]
    assert unlisted and all(scene["point_const"][point_index[p]] for p in unlisted)                # seen from outside: constant by track length
    assert scene["pose_const"].tolist()[:3] == [1, 0, 0] and scene["tvec_const_mask"].tolist()[:3] == [0, 1, 0]
    masks = dict(zip(cam_index, scene["camera_const_mask"].tolist()))
    assert masks[1] == masks[2] == 0xFFFF and (masks[0] != 0xFFFF) == refine


@pytest.mark.parametrize("refine", [False, True], ids=["refine_off", "focal_extra"])
def test_local_config_with_a_camera_only_seen_from_outside(refine):
    rec = bsw.world_a()
    _compare(rec, bsw.local_config(rec), bsw.options(refine))


def test_global_config():
    rec = bsw.world_a()
    want, rep = _compare(rec, bsw.global_config(rec), bsw.options(True))
    assert rep.num_obs == rep.num_config_obs == 1800 and rep.num_poses == 12 and rep.num_points == 300 and rep.num_cameras == 3


def test_a_living_handle():
    """the eight-image loop inside a session, then IterativeGlobalRefinement: at every bundle adjustment both routes are compared before the solve, on a handle
    that by then holds appended, merged and deleted points and newly registered images"""
    rec, graph, _ = irs.make_world(seed=0)
    tri = IncrementalTriangulator(graph, rec)
    mapper = IncrementalMapper(graph, rec, tri)
    options = IncrementalMapperOptions()
    options.abs_pose_min_num_inliers = irs.MIN_NUM_INLIERS
    options.print_summary = False
    compared = []
    solve = BundleAdjuster.Solve

    def checked(self, reconstruction, session=None):
        ses = session if session is not None else ba._live_session(reconstruction)
        assert ses is not None and ses.live
        want = bsw.flatten_and_restore(self, reconstruction)
        bsw.assert_same_flatten(self.flatten_on(ses), want)
        state = ses.pb.state()
        compared.append((self.config_.NumImages(), None if want is None else len(want[0]["lines"]), int(state["deleted"].sum()), len(ses.ids)))
        return solve(self, reconstruction, session=session)

    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(BundleAdjuster, "Solve", checked)
        with tri.Session(tri.Options()) as live:
            num_points_at_open = len(live.ids)
            for _ in range(20):
                ranked = mapper.FindNextImages(options)
                done = False
                for image_id in ranked:
                    if mapper.RegisterNextImage(options, image_id):
                        tri.TriangulateImage(tri.Options(), image_id)
                        IterativeLocalRefinement(rec, tri, image_id, options)
                        done = True
                        break
                if not done:
                    break
            num_local = len(compared)
            IterativeGlobalRefinement(rec, options, triangulator=tri, mapper=mapper)
    finally:
        mp.undo()
    print("compared (config images, observations, deleted points, points):", compared)
    assert len(rec.RegImageIds()) == 8
    assert len(compared) >= 10 and num_local >= 5 and len(compared) > num_local
    assert compared[-1][0] == 8 and compared[-1][3] > num_points_at_open      # the global config on a handle with appended points
    assert max(c[2] for c in compared) > 0                                      # ... and merged or deleted ones


def _raw(pb, flags, variable=(), constant=(), obs_capacity=None, point_capacity=None):
    """the call itself on sentinel-filled outputs -> (rc, report, outputs)"""
    P, T = pb.num_points()
    M = T if obs_capacity is None else obs_capacity
    Pn = P if point_capacity is None else point_capacity
    fl = np.ascontiguousarray(flags, dtype=np.uint8)
    vp, cp = np.ascontiguousarray(variable, dtype=np.int32), np.ascontiguousarray(constant, dtype=np.int32)
    ip, u8 = _capi.c_ip, _capi.c_u8p
    cfg = _capi.BundleConfig(fl.ctypes.data_as(u8), None, None, None, vp.ctypes.data_as(ip) if len(vp) else None, cp.ctypes.data_as(ip) if len(cp) else None,
                             len(vp), len(cp))
    out = dict(lines=np.full((T + 1, 3), -7.0), obs_pose=np.full(T + 1, -7, np.int32), obs_point=np.full(T + 1, -7, np.int32), obs_line=np.full(T + 1, -7, np.int32),
               pose_image=np.full(pb.num_images, -7, np.int32), pose_const=np.full(pb.num_images, 7, np.uint8), pose_tvec=np.full(pb.num_images, 7, np.uint8),
               pose_camera=np.full(pb.num_images, -7, np.int32), point_index=np.full(P + 1, -7, np.int32), point_const=np.full(P + 1, 7, np.uint8),
               points=np.full((P + 1, 3), -7.0), camera_index=np.full(pb.num_cameras, -7, np.int32), camera_mask=np.full(pb.num_cameras, 7, np.uint16))
    before = {k: v.copy() for k, v in out.items()}
    rep = _capi.BundleSetupReport()
    rep.num_obs = -7
    o = out
    rc = _capi.lib().pp_tracks_bundle_setup(pb._h, C.byref(cfg), C.byref(rep), o["lines"].ctypes.data_as(_capi.c_dp), o["obs_pose"].ctypes.data_as(ip),
                                            o["obs_point"].ctypes.data_as(ip), o["obs_line"].ctypes.data_as(ip), M, o["pose_image"].ctypes.data_as(ip),
                                            o["pose_const"].ctypes.data_as(u8), o["pose_tvec"].ctypes.data_as(u8), o["pose_camera"].ctypes.data_as(ip),
                                            o["point_index"].ctypes.data_as(ip), o["point_const"].ctypes.data_as(u8), o["points"].ctypes.data_as(_capi.c_dp), Pn,
                                            o["camera_index"].ctypes.data_as(ip), o["camera_mask"].ctypes.data_as(_capi.c_u16p))
    untouched = rep.num_obs == -7 and all(np.array_equal(out[k], before[k]) for k in out)
    return rc, rep, out, untouched


def test_read_only_and_errors():
    rec = bsw.world_a()
    rec.images[5].registered = False
    ses = _session(rec)
    try:
        pb = ses.pb
        P, T = pb.num_points()
        # a point the handle deleted: its observations fail a filter with a bound of nothing
        subset = np.zeros(P, dtype=np.uint8)
        subset[0] = 1
        pb.filter_points(1e-12, 0.0, point_subset=subset)
        assert pb.state()["deleted"][0] == 1 and pb.state()["deleted"].sum() == 1
        P, T = pb.num_points()
        flags = np.zeros(12, dtype=np.uint8)
        flags[[0, 1, 3]] = 1
        listed = [7, 9, 11, 250]
        state = pb.state()
        rc, rep, out, untouched = _raw(pb, flags, listed)
        assert rc == 0 and not untouched and rep.num_obs > rep.num_config_obs > 0
        after = pb.state()
        assert sorted(state) == sorted(after) and all(np.array_equal(state[k], after[k]) for k in state)      # the call never changes the handle
        M, N = int(rep.num_obs), int(rep.num_points)
        line_image = ses.flat["line_image"]
        assert np.array_equal(out["lines"][:M], ses.flat["lines"][out["obs_line"][:M]])                       # obs_line: the handle line of each observation
        assert np.array_equal(out["pose_image"][out["obs_pose"][:M]], line_image[out["obs_line"][:M]])
        assert np.array_equal(out["point_index"][out["obs_point"][:M]][: int(rep.num_config_obs)], after["line_point"][out["obs_line"][: int(rep.num_config_obs)]])
        assert (out["obs_pose"][M:] == -7).all() and (out["point_index"][N:] == -7).all()                     # nothing beyond what the report counts
        # the exact capacities pass, one less does not
        rc, rep2, out2, _ = _raw(pb, flags, listed, obs_capacity=M, point_capacity=N)
        assert rc == 0 and rep2.num_obs == M and all(np.array_equal(out[k], out2[k]) for k in out)
        for kw in (dict(obs_capacity=M - 1), dict(point_capacity=N - 1), dict(obs_capacity=M - 1, point_capacity=N)):
            rc, _, _, untouched = _raw(pb, flags, listed, **kw)
            assert rc == _capi.PP_ERR_INVALID and untouched, kw
        assert b"capacity" in _capi.lib().pp_last_error()
        # a deleted point in a list, an unregistered image in the config, an index out of range
        for variable, constant in (([7, 0], []), ([], [0]), ([P], []), ([-1], []), ([], [P + 5])):
            rc, _, _, untouched = _raw(pb, flags, variable, constant)
            assert rc == _capi.PP_ERR_INVALID and untouched, (variable, constant)
        bad = flags.copy()
        bad[5] = 1
        rc, _, _, untouched = _raw(pb, bad, listed)
        assert rc == _capi.PP_ERR_INVALID and untouched and b"not registered" in _capi.lib().pp_last_error()
        with pytest.raises(_capi.PPError):
            pb.bundle_setup(bad)
        # and the handle still works
        rc, rep3, out3, _ = _raw(pb, flags, listed)
        assert rc == 0 and all(np.array_equal(out[k], out3[k]) for k in out)
    finally:
        ses.close()


def test_create_refuses_a_line_that_fails_the_norm_test():
    """pp_tracks_create tests |(a, b)| itself, so no handle holds a line SetUp's CHECK_NEAR (:373) would stop at: bad_line stays -1 on every handle that
    exists.  The same world on the host route: flatten() raises."""
    rec = bsw.world(2, 8, 2)
    for idx in (2, 5):
        l = np.array(rec.images[1].lines[idx].Line(), dtype=np.float64)
        l[:2] *= (1.0 + 2e-6)
        old = rec.images[1].lines[idx]
        rec.images[1].lines[idx] = FeatureLine(l, old.IsAligned(), old.Point3DId())
    cfg = BundleAdjustmentConfig()
    cfg.AddImage(1)
    with pytest.raises(ValueError, match="CHECK_NEAR"):
        bsw.flatten(rec, cfg, bsw.options(False))
    with pytest.raises(_capi.PPError) as e:
        _session(rec)
    assert e.value.code == _capi.PP_ERR_INVALID and "not normalised" in str(e.value)
