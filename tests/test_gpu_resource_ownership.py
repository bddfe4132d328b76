"""Every handle gives back what it took: the pool's counts of live device blocks and live pinned blocks (pp_pool_stats) are, after a handle is closed,
what they were before it was built - whatever the handle allocated lazily in between (solver buffers, the wider J_pose, the conjugate-gradient vectors,
the intrinsics lists, the chunked pair lists, the block-sparse tile list, the packed system of a group exchange, the covariance's scratch) and also when
pp_ba_create refuses the problem half way.  Deltas, not zeros: a fixture of the session may hold a handle."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import mixed_models as mm
import tracks_image_scenes as scenes
from privacy_preserving_sfm_amd import _capi, synthetic
from privacy_preserving_sfm_amd.device import (BAProblem, CorrGraphBuilder, FourView2dProblem, LineFeatureGenerator, PairSelector, PlanarOffsetProblem,
                                               Pose2dProblem, PoseProblem, SiftMatcher, TracksProblem, _ba_desc, ba_options, device_count, tracks_image_options,
                                               tracks_options, triangulate_tracks, triangulation_options)
from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator

pytestmark = pytest.mark.gpu


def _live():
    """(live device blocks, live pinned blocks) of the process"""
    dev, pinned, cached = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert _capi.lib().pp_pool_stats(C.byref(dev), C.byref(pinned), C.byref(cached)) == 0
    assert dev.value >= 0 and pinned.value >= 0 and cached.value >= 0
    assert _capi.lib().pp_pool_stats(None, None, None) == 0      # null outputs are allowed
    return dev.value, pinned.value


def _host_view(pb, jac_mode):
    r, jp, jx, jc = _capi.c_dp(), _capi.c_dp(), _capi.c_dp(), _capi.c_dp()
    cost = C.c_double(0)
    _capi.check(_capi.lib().pp_ba_eval_host_view(pb._h, jac_mode, 0, 1, C.byref(r), C.byref(jp), C.byref(jx), C.byref(jc), C.cast(C.byref(cost), _capi.c_dp)))
    assert r and jp and jx and not jc and np.isfinite(cost.value)


def test_direct_handle_with_regrown_jacobians_host_view_and_covariance():
    sc = synthetic.make_ba_scene(6, 200, 6)
    before = _live()
    pb = BAProblem(sc)
    try:
        held = _live()
        assert held[0] > before[0] and held[1] > before[1]      # (the counts do see this handle: its blocks and its pinned scalars)
        assert pb.solve(ba_options(max_num_iterations=3)).num_iterations == 3
        pb.evaluate(ambient=False)
        grown = _live()
        pb.evaluate(ambient=True)                               # J_pose regrows from 12 to 14 doubles a row: one block back, one block out
        assert _live() == grown
        _host_view(pb, 1)                                       # the pinned mirrors (plain pinned memory: not the pool's)
        pc, xc = pb.covariance([(1, 1), (3, 2)], [0, 7, 199])
        assert np.isfinite(pc).all() and np.isfinite(xc).all()
    finally:
        pb.close()
    assert _live() == before


def test_iterative_handle():
    sc = synthetic.make_ba_scene(6, 200, 6)
    before = _live()
    pb = BAProblem(sc, linear_solver=2)
    try:
        assert pb.structure()["iterative"]
        s = pb.solve(ba_options(max_num_iterations=3))
        assert s.num_iterations == 3 and s.linear_solver_iterations > 0
        assert _live()[1] >= before[1] + 2                      # (the scalars' mirror and the conjugate-gradient state's)
    finally:
        pb.close()
    assert _live() == before


@pytest.mark.parametrize("cameras", ["shared", "per_image"])
def test_variable_intrinsics(cameras):
    """the settings of test_gpu_mixed_camera_models for variable intrinsics (rule "pair": n_v = 2 a camera, the variable parameters moved off their start):
    one camera for all images - the general block-pair lists (gen_*, kk_*) - and a camera per image - the wide rows beside the pose columns"""
    if cameras == "shared":
        sc = mm.mixed_ba_scene(8, 200, 5, models=[2], num_intrinsics=1, rule="pair", model=2, seed=9)
    else:
        sc = mm.mixed_ba_scene(8, 200, 5, models=[1, 2, 8, 4], num_intrinsics=8, rule="pair", model=2, seed=9)
    sc = mm.perturb_variable_intrinsics(sc, 8)
    before = _live()
    pb = BAProblem(sc)
    try:
        st = pb.structure()
        assert st["intrinsics_columns"] == (2 if cameras == "shared" else 16) and st["wide_intrinsics"] == (0 if cameras == "shared" else 2), st
        assert pb.solve(ba_options(max_num_iterations=3)).num_iterations >= 1
    finally:
        pb.close()
    assert _live() == before


def test_chunked_pair_lists(monkeypatch):
    """make_ba_scene(20, 400, 5): 190 lists of about 21 entries, 4000 in all - `latency_bound` of pp_ba_create, lists in chunks of 8.  Neither
    pp_ba_get_structure nor the solve summary says which path a handle took; the pool does: the same handle under PPSFM_BA_CHUNKED_PAIRS=0 holds exactly
    three blocks fewer (the chunks, the first chunk of every pair, the chunks' partial blocks)."""
    sc = synthetic.make_ba_scene(20, 400, 5)
    held = {}
    for chunked in ("0", "1"):
        with monkeypatch.context() as m:
            m.setenv("PPSFM_BA_CHUNKED_PAIRS", chunked)
            before = _live()
            pb = BAProblem(sc)
            try:
                assert pb.solve(ba_options(max_num_iterations=2)).num_iterations >= 1
                held[chunked] = _live()[0] - before[0]
            finally:
                pb.close()
            assert _live() == before
    assert held["1"] == held["0"] + 3, held


def test_block_sparse_handle_with_covariance():
    sc = synthetic.make_ba_scene(100, 1500, 5, window=8)
    before = _live()
    pb = BAProblem(sc)
    try:
        assert pb.structure()["block_sparse"]
        s = pb.solve(ba_options(max_num_iterations=2))
        assert s.num_iterations >= 1 and s.cholesky_fallbacks == 0
        pc, xc = pb.covariance([(4, 4), (50, 49)], [0, 700, 1499])
        assert np.isfinite(pc).all() and np.isfinite(xc).all()
    finally:
        pb.close()
    assert _live() == before


def test_host_allreduce_callback():
    sc = synthetic.make_ba_scene(6, 200, 6)
    calls = []
    before = _live()
    pb = BAProblem(sc, ordering=1)
    try:
        pb.set_allreduce(lambda p, n, op: calls.append(n) or 0, 0, 1)      # one rank: the sum over the group is what is there already
        assert pb.solve(ba_options(max_num_iterations=2)).num_iterations == 2
        assert calls                                                        # (the packed system went through the callback)
    finally:
        pb.close()
    assert _live() == before


def test_tracks_handle():
    spec = scenes.SYNTHETIC[0]
    rec, graph = scenes.synthetic_world(spec["cfg"], spec["seed"], spec["image"])
    flat, _, _ = IncrementalTriangulator(graph, rec).flatten()
    image = sorted(rec.images).index(spec["image"])
    before = _live()
    pb = TracksProblem(flat)
    try:
        assert _live()[0] > before[0]
        pb.complete(tracks_options())
        pb.merge(tracks_options())
        rep, _ = pb.triangulate_image(image, tracks_image_options(), flat["line_aligned"])
        assert rep.num_changed >= 0
    finally:
        pb.close()
    assert _live() == before


@pytest.mark.parametrize("lists", ["d", "h"])
def test_refused_create_gives_everything_back(monkeypatch, lists):
    """images that share points under a co-visibility matrix of zeros: PP_ERR_INVALID from pp_ba_create's check of the matrix.  With the pair lists built on
    the device (d) the refusal comes when the by-point lists and the lists' entries are on the device, on the host (h) when the handle holds its stream and
    events only."""
    sc = dict(synthetic.make_ba_scene(6, 200, 6))
    sc["covisibility"] = np.zeros((6, 6), dtype=np.uint8)
    monkeypatch.setenv("PPSFM_BA_PAIR_LISTS", lists)
    keep = []
    d = _ba_desc(sc, keep)
    h = C.c_void_p()
    before = _live()
    rc = _capi.lib().pp_ba_create(C.byref(d), 0, C.byref(h))
    assert rc == _capi.PP_ERR_INVALID and not h
    text = _capi.lib().pp_last_error().decode()
    m = re.search(r"images (\d+) and (\d+) share a point", text)
    assert m and m.group(1) != m.group(2) and all(0 <= int(g) < 6 for g in m.groups()), text
    assert _live() == before


def test_sift_handle():
    rng = np.random.default_rng(18)
    descriptors = [rng.integers(0, 256, size=(n, 128), dtype=np.uint8) for n in (3, 2)]
    before = _live()
    m = SiftMatcher(descriptors)
    try:
        assert _live()[0] > before[0]
        _, out = m.match_pairs([(0, 1)])
        assert len(out) == 1 and out[0].shape[1] == 2
    finally:
        m.close()
    assert _live() == before
    m.close()                                                   # a second close is harmless
    assert _live() == before


def test_corr_graph_handle():
    before = _live()
    g = CorrGraphBuilder([2, 2])
    try:
        assert _live()[0] > before[0]
        rep = g.build([(0, 1)], [np.array([[0, 1]], dtype=np.int32)], min_num_matches=0)
        assert rep.num_matches_accepted == 1
        assert list(g.get()["corr_start"]) == [0, 1, 1, 1, 2]   # line 0 of image 0 and line 1 of image 1 see each other
    finally:
        g.close()
    assert _live() == before
    g.close()
    assert _live() == before


def test_pairs_handle():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], dtype=np.float32)
    before = _live()
    sel = PairSelector()
    try:
        assert _live() == before                                # a fresh handle holds no blocks
        _, pairs, sqdist = sel.spatial(xyz, 2, 10.0)
        assert len(pairs) == 3 and len(sqdist) == 3             # every location and its one neighbour besides itself
        assert _live() == (before[0] + 2, before[1])            # the result: pairs and distances (the call's scratch went back)
        _, pairs = sel.transitive(3, [(0, 1), (1, 2)])
        assert [tuple(p) for p in pairs] == [(0, 2)]
        assert _live() == (before[0] + 1, before[1])            # the new result replaced the first one: pairs alone
    finally:
        sel.close()
    assert _live() == before
    sel.close()
    assert _live() == before


def _refuse_handle(cls, *args):
    """entry(device) -> (code, out handle) of the create function behind cls(*args, device=device)"""
    def entry(device):
        obj = cls.__new__(cls)
        with pytest.raises(_capi.PPError) as e:
            obj.__init__(*args, device=device)
        return e.value.code, obj._h
    return entry


def _refuse_call(call):
    def entry(device):
        with pytest.raises(_capi.PPError) as e:
            call(device)
        return e.value.code, None
    return entry


def _tiny_tracks_flat():
    """one image, one camera, no lines, no points"""
    return dict(poses=np.array([[1.0, 0, 0, 0, 0, 0, 0]]), pose_camera=[0], camera_model=[2], intr=_tiny_intr(), cam_size=[[100, 100]], lines=np.zeros((0, 3)),
                line_image=[], line_point=[], corr_start=[0], corr_line=[], points=np.zeros((0, 3)), track_start=[0], track_line=[])


def _tiny_intr():
    intr = np.zeros((1, _capi.CAM_STRIDE))
    intr[0, :3] = [100.0, 50.0, 50.0]                           # SIMPLE_RADIAL: f, cx, cy, k
    return intr


def _tiny_triangulation(device):
    P = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(1, 12), (3, 1))
    return triangulate_tracks([0, 3], np.tile([1.0, 0, 0], (3, 1)), [0, 1, 2], P, np.zeros((3, 3)), [0, 0, 0], [2], _tiny_intr(), [[100, 100]],
                              triangulation_options(max_error=1.0), device=device)


def _tiny_line_features(device):
    return LineFeatureGenerator(device=device).generate([1], [0, 1], [[10.0, 10.0]], [0], [2], _tiny_intr())


def _tiny_scan(device):
    a, out = np.arange(5, dtype=np.int32), np.zeros(6, dtype=np.int32)
    _capi.check(_capi.lib().pp_debug_exclusive_scan(device, 4, 5, a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), None, None))


@functools.lru_cache(maxsize=None)
def _device_entries():
    rng = np.random.default_rng(3)
    eye = np.tile(np.eye(3), (4, 1, 1))
    return {
        "pp_ba_create": _refuse_handle(BAProblem, synthetic.make_ba_scene(6, 200, 6)),
        "pp_pose_create": _refuse_handle(PoseProblem, rng.normal(size=(6, 3)), rng.normal(size=(6, 3))),
        "pp_planar_create": _refuse_handle(PlanarOffsetProblem, np.tile(np.eye(3, 4), (4, 1, 1)), rng.normal(size=(4, 5, 3)), eye),
        "pp_pose2d_create": _refuse_handle(Pose2dProblem, rng.normal(size=(5, 2)), rng.normal(size=(5, 2))),
        "pp_fourview2d_create": _refuse_handle(FourView2dProblem, rng.normal(size=(4, 5, 2))),
        "pp_tracks_create": _refuse_handle(TracksProblem, _tiny_tracks_flat()),
        "pp_sift_create": _refuse_handle(SiftMatcher, [np.zeros((1, 128), dtype=np.uint8)]),
        "pp_corr_graph_create": _refuse_handle(CorrGraphBuilder, [2, 2]),
        "pp_pairs_create": _refuse_handle(PairSelector),
        "pp_triangulate_tracks": _refuse_call(_tiny_triangulation),
        "pp_line_features_from_keypoints": _refuse_call(_tiny_line_features),
        "pp_debug_exclusive_scan": _refuse_call(_tiny_scan),
    }


DEVICE_ENTRIES = ("pp_ba_create", "pp_pose_create", "pp_planar_create", "pp_pose2d_create", "pp_fourview2d_create", "pp_tracks_create", "pp_sift_create",
                  "pp_corr_graph_create", "pp_pairs_create", "pp_triangulate_tracks", "pp_line_features_from_keypoints", "pp_debug_exclusive_scan")


@pytest.mark.parametrize("which", ["count", "minus_one"])
@pytest.mark.parametrize("entry", DEVICE_ENTRIES)
def test_refused_device(entry, which):
    """every entry that takes a device refuses one the process does not have in the same words, after its argument checks (the arguments here are valid)
    and before it takes anything: PP_ERR_INVALID, "<entry>: device <d> of <count>", a null handle, the pool as it was.  Nothing is launched."""
    count = device_count()
    device = count if which == "count" else -1
    call = _device_entries()[entry]
    before = _live()
    code, handle = call(device)
    assert code == _capi.PP_ERR_INVALID
    assert _capi.lib().pp_last_error().decode() == "%s: device %d of %d" % (entry, device, count)
    assert not handle
    assert _live() == before
