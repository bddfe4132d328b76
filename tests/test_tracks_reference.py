"""Track completion and merging without a GPU: the sequential oracle (tests/tracks_reference.py) on planted scenes, the descriptor flattening,
and the C ABI's behaviour without a device."""
import ctypes as C

import numpy as np
import pytest

import tracks_reference as tr
from privacy_preserving_sfm_amd import _capi, synthetic
from privacy_preserving_sfm_amd.device import TracksProblem, tracks_desc, tracks_options
from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator, reconstruction_from_completion_scene

QUIET = dict(noise_point=1e-4, noise_t=1e-5, noise_q=1e-5)      # start close to the truth: every planted line is a sub-pixel inlier
SCENES = [(20, 150, 10, 1), (20, 150, 10, 2), (24, 200, 12, 5)]


def _world(cfg):
    sc = synthetic.make_completion_scene(*cfg[:3], seed=cfg[3], **QUIET)
    rec, graph = reconstruction_from_completion_scene(sc)
    return sc, rec, graph


def _reachable_withheld(sc, rec, graph, max_transitivity, max_error=4.0):
    """Independent of the oracle's WALK, not of its arithmetic: per Point3D, a depth-limited search from its track over withheld lines of ITS true point
    whose planted error (at the point's start position) is below the threshold.  The error comes from tracks_reference.squared_line_reprojection_error, the
    oracle's own function; what this expectation adds is the planted truth (which lines, which true point) and a walk written separately."""
    ref = [(int(sc["line_image"][l]), k) for l, k in zip(range(len(sc["line_image"])), _idx_in_image(sc))]
    line_of = {r: l for l, r in enumerate(ref)}
    out = set()
    for pid, pt in rec.points3D.items():
        true_p = sc["line_true_point"][line_of[pt.track[0]]]
        frontier, seen = list(pt.track), set()
        for _ in range(max_transitivity):
            nxt = []
            for el in frontier:
                for c in graph.FindCorrespondences(*el):
                    l = line_of[c]
                    if c in seen or sc["line_point"][l] >= 0 or sc["line_true_point"][l] != true_p:
                        continue
                    image = rec.images[c[0]]
                    e = tr.squared_line_reprojection_error(image.lines[c[1]].Line(), pt.xyz, tr.projection_matrix(image.qvec, image.tvec), rec.cameras[image.camera_id])
                    if e > max_error * max_error:
                        continue
                    seen.add(c); nxt.append(c)
            frontier = nxt
        out |= set((pid, c) for c in seen)
    return out


def _idx_in_image(sc):
    idx, count = [], {}
    for c in sc["line_image"]:
        idx.append(count.get(int(c), 0)); count[int(c)] = idx[-1] + 1
    return idx


@pytest.mark.parametrize("cfg", SCENES)
def test_oracle_completes_the_withheld_lines_and_no_false_edge(cfg, oracle):
    sc, rec, graph = _world(cfg)
    o = tr.TracksOracle(graph, rec)
    n = o.CompleteAllTracks(tr.Options())
    assert n == len(o.completed) > 0
    # two Point3Ds of a split true point compete for its withheld lines: the claimed LINES are the reachable ones, each claimed once
    expect = _reachable_withheld(sc, rec, graph, 5)
    assert set(c for _, c in o.completed) == set(c for _, c in expect)
    assert len(set(c for _, c in o.completed)) == n
    ref = list(zip(sc["line_image"].tolist(), _idx_in_image(sc)))
    line_of = {r: l for l, r in enumerate(ref)}
    for pid, c in o.completed:      # every completed line is a withheld line of the point's own true point: no false edge was followed
        l = line_of[c]
        assert l in set(sc["withheld_lines"])
        assert sc["line_true_point"][l] == sc["line_true_point"][line_of[rec.points3D[pid].track[0]]]
    assert o.margin > 1e-6


@pytest.mark.parametrize("cfg", SCENES)
def test_oracle_merges_the_split_points_only(cfg, oracle):
    sc, rec, graph = _world(cfg)
    o = tr.TracksOracle(graph, rec)
    o.CompleteAllTracks(tr.Options())
    lengths = {p: len(pt.track) for p, pt in rec.points3D.items()}
    n = o.MergeAllTracks(tr.Options())
    assert sorted((a, b) if a < b else (b, a) for a, b, _ in o.merged) == sorted(sc["split_pairs"])
    assert n == sum(lengths[a] + lengths[b] for a, b, _ in o.merged)
    first_new = sc["points"].shape[0]
    assert [m for _, _, m in o.merged] == list(range(first_new, first_new + len(o.merged)))      # the next unused ids, in order
    for a, b, m in o.merged:
        assert a not in rec.points3D and b not in rec.points3D and len(rec.points3D[m].track) == lengths[a] + lengths[b]


def test_transitivity_one_reaches_less_than_five(oracle):
    sc, rec, graph = _world(SCENES[2])
    o5 = tr.TracksOracle(graph, rec)
    n5 = o5.CompleteAllTracks(tr.Options())
    sc1, rec1, graph1 = _world(SCENES[2])
    o1 = tr.TracksOracle(graph1, rec1)
    n1 = o1.CompleteAllTracks(tr.Options(complete_max_transitivity=1))
    assert 0 < n1 < n5
    assert set(c for _, c in o1.completed) < set(c for _, c in o5.completed)      # the planted chains: lines that hang on withheld lines only


def test_flattening_round_trips():
    sc, rec, graph = _world(SCENES[0])
    flat, point_ids, line_ref = IncrementalTriangulator(graph, rec).flatten()
    assert point_ids == list(range(sc["points"].shape[0]))
    assert np.array_equal(flat["line_point"], sc["line_point"]) and np.array_equal(flat["line_image"], sc["line_image"])
    assert np.array_equal(flat["lines"], sc["line_xyz"]) and np.array_equal(flat["corr_start"], sc["corr_start"]) and np.array_equal(flat["corr_line"], sc["corr_line"])
    assert np.array_equal(flat["points"], sc["points"]) and np.array_equal(flat["cam_size"], sc["cam_size"]) and not flat["camera_skip"].any()
    for p in point_ids:      # tracks in track order, consistent with line_point
        t = flat["track_line"][flat["track_start"][p]:flat["track_start"][p + 1]]
        assert [line_ref[l] for l in t] == rec.points3D[p].track and (flat["line_point"][t] == p).all()
    keep = []
    d = tracks_desc(flat, keep)
    assert (d.num_images, d.num_cameras, d.num_points, d.num_lines, d.num_corrs) == (20, 1, len(point_ids), len(line_ref), len(sc["corr_line"]))
    assert np.ctypeslib.as_array(d.corr_line, (d.num_corrs,)).tolist() == sc["corr_line"].tolist()


def test_camera_bogus_params():
    sc, rec, graph = _world(SCENES[0])
    cam = rec.cameras[0]
    assert not cam.HasBogusParams(0.1, 10.0, 1.0)
    assert cam.HasBogusParams(0.1, 0.5, 1.0) and cam.HasBogusParams(0.1, 10.0, 0.001)
    cam.params[1] = -1.0
    assert cam.HasBogusParams(0.1, 10.0, 1.0)


def test_c_abi_exports_and_fails_loudly_without_a_device():
    L = _capi.lib()
    names = ("pp_tracks_options_default", "pp_tracks_create", "pp_tracks_destroy", "pp_tracks_complete", "pp_tracks_merge", "pp_tracks_get_state")
    for n in names:
        assert n in _capi.exported_symbols() and hasattr(L, n)
    o = tracks_options()
    assert (o.merge_max_reproj_error, o.complete_max_reproj_error, o.complete_max_transitivity) == (4.0, 4.0, 5)
    sc, rec, graph = _world(SCENES[0])
    flat, _, _ = IncrementalTriangulator(graph, rec).flatten()
    # bad arguments are PP_ERR_INVALID before any device work, with or without a GPU
    h = C.c_void_p()
    assert L.pp_tracks_create(None, 0, C.byref(h)) == _capi.PP_ERR_INVALID
    for key, bad in (("line_point", len(flat["points"])), ("corr_line", len(flat["line_image"])), ("line_image", -1), ("track_line", 10 ** 6)):
        f = dict(flat); f[key] = flat[key].copy(); f[key][3] = bad
        keep = []
        d = tracks_desc(f, keep)
        assert L.pp_tracks_create(C.byref(d), 0, C.byref(h)) == _capi.PP_ERR_INVALID, key
    f = dict(flat); f["line_point"] = flat["line_point"].copy(); f["line_point"][np.flatnonzero(flat["line_point"] < 0)[0]] = 0      # a line with a point but in no track
    keep = []
    d = tracks_desc(f, keep)
    assert L.pp_tracks_create(C.byref(d), 0, C.byref(h)) == _capi.PP_ERR_INVALID
    rep = _capi.TracksReport()
    assert L.pp_tracks_complete(None, C.byref(o), None, C.byref(rep), None, None, 0) == _capi.PP_ERR_INVALID
    assert L.pp_tracks_merge(None, C.byref(o), None, C.byref(rep), None, None, None, 0) == _capi.PP_ERR_INVALID
    n = C.c_int()
    L.pp_device_count(C.byref(n))
    if n.value == 0:      # no CPU path: a valid descriptor cannot become a handle without a device
        with pytest.raises(_capi.PPError) as e:
            TracksProblem(flat)
        assert e.value.code == _capi.PP_ERR_HIP
