"""pp_corr_graph_build (K18, csrc/corr_graph.hip) against feature_matching.build_correspondence_graph: EXACT equality of the CSR, the connected images, the
per-image and per-pair counts and the report's counts - no tolerance anywhere.

The kernels' real edges, which the shapes straddle:
  64     a wavefront: k_corr_count adds a wavefront's accepted matches to its pair in one atomic when all 64 lanes lie in one pair, lane by lane otherwise;
         the wave sums of k_corr_first and k_corr_image
  256    a workgroup: every kernel covers matches, entries or lines in blocks of 256; k_corr_first and k_corr_image stride a pair's matches / an image's
         lines by 256
  1024   a tile of the degree scan (LaunchExclusiveScan, csrc/scan.hpp): the edge problem has more than 4096 lines, so the tile sums are scanned and every
         tile starts from its offset
  4096   the LDS first-occurrence table of k_corr_first (kCorrTile): an image of 4097 lines puts a pair on two tiles, with first occurrences and repeats
         on both sides of the tile edge
Images of 1, 63, 64, 65 and 257 lines, one of 0 lines and one of 4097 share one problem.  A line's neighbour list has no edge of its own - k_corr_order
places an entry by counting the smaller pair ranks of its list - but the 72-image problem makes every list 71 long, longer than a wavefront, with the
pairs given shuffled and in both orientations, so any order but pair order shows.

Every input whose pairs repeat indices on at most one side must report 0 replayed pairs: these tests do not pass by way of the host loop.  The input
with k both-sided pairs (the shadow case among them) must report exactly k."""
import ctypes as C
import itertools

import numpy as np
import pytest

from privacy_preserving_sfm_amd import _capi, feature_matching as fm, synthetic
from privacy_preserving_sfm_amd.device import CorrGraphBuilder
from privacy_preserving_sfm_amd.incremental_triangulator import FlatCorrespondenceGraph, IncrementalTriangulator, reconstruction_from_completion_scene

pytestmark = pytest.mark.gpu

BAD = [-1, -7, -2 ** 31, 2 ** 31 - 1]


def _independent_counts(matches, num_lines, min_num_matches):
    """(accepted, bad index, duplicate, pairs with repeats on both sides) over the used pairs that are no self pair, by a plain loop over the input"""
    accepted = bad = dup = both = 0
    for (a, b), m in matches.items():
        if len(m) <= min_num_matches or a == b:
            continue
        seen_a, seen_b, rep_a, rep_b, taken_a, taken_b = set(), set(), 0, 0, set(), set()
        for xa, xb in np.asarray(m, dtype=np.int64).reshape(-1, 2):
            if not (0 <= xa < num_lines[a] and 0 <= xb < num_lines[b]):
                bad += 1
                continue
            rep_a, rep_b = rep_a + (xa in seen_a), rep_b + (xb in seen_b)
            seen_a.add(xa); seen_b.add(xb)
            if xa in taken_a or xb in taken_b:
                dup += 1
                continue
            taken_a.add(xa); taken_b.add(xb)
            accepted += 1
        both += rep_a > 0 and rep_b > 0
    return accepted, bad, dup, both


def _reference(matches, num_lines, min_num_matches):
    graph, connected = fm.build_correspondence_graph(matches, num_lines, min_num_matches)
    return graph, connected, FlatCorrespondenceGraph.from_graph(graph, num_lines)


def _device(builder, matches, ids, min_num_matches):
    index = {i: k for k, i in enumerate(ids)}
    pairs = [(index[a], index[b]) for a, b in matches]
    rep = builder.build(pairs, list(matches.values()), min_num_matches)
    return rep, builder.get(), builder.pair_counts()


def _assert_equal(rep, out, pair_counts, matches, num_lines, min_num_matches, reference, replayed=0):
    graph, connected, flat = reference
    ids = sorted(num_lines)
    assert out["corr_start"].dtype == np.int32 and out["corr_line"].dtype == np.int32
    assert np.array_equal(out["corr_start"], flat.corr_start) and np.array_equal(out["corr_line"], flat.corr_line)
    assert [i for i, c in zip(ids, out["image_connected"]) if c] == connected
    assert out["image_num_observations"].tolist() == [graph.NumObservationsForImage(i) for i in ids]
    assert out["image_num_correspondences"].tolist() == [graph.NumCorrespondencesForImage(i) for i in ids]
    assert pair_counts.tolist() == [0 if a == b else graph.NumCorrespondencesBetweenImages(a, b) for a, b in matches]
    accepted, bad, dup, both = _independent_counts(matches, num_lines, min_num_matches)
    assert 2 * accepted == len(flat.corr_line)
    assert (rep.num_matches_accepted, rep.num_matches_bad_index, rep.num_matches_duplicate) == (accepted, bad, dup)
    assert rep.num_matches_in == sum(len(m) for m in matches.values())
    used = sum(len(m) > min_num_matches for m in matches.values())
    assert (rep.num_pairs_used, rep.num_pairs_ignored) == (used, len(matches) - used)
    assert rep.num_pairs_replayed == replayed == both
    assert rep.device_ms > 0 and rep.total_ms >= rep.device_ms


def _run(matches, num_lines, min_num_matches, replayed=0):
    ids = sorted(num_lines)
    reference = _reference(matches, num_lines, min_num_matches)
    builder = CorrGraphBuilder([num_lines[i] for i in ids])
    try:
        rep, out, pair_counts = _device(builder, matches, ids, min_num_matches)
    finally:
        builder.close()
    _assert_equal(rep, out, pair_counts, matches, num_lines, min_num_matches, reference, replayed)
    return rep, out, reference


def _one_sided(rng, n1, n2, count, side, num_bad=0):
    """count matches between images of n1 and n2 lines: distinct indices on both sides, but random ones (repeats) on `side` (None: neither); num_bad rows
    then get an index that does not exist"""
    cols = [rng.integers(0, n, count) if side == k else rng.permutation(n)[:count] for k, n in enumerate((n1, n2))]
    m = np.stack(cols, axis=1).astype(np.int64)
    assert m.shape == (count, 2)
    for r in rng.permutation(count)[:num_bad]:
        m[r, int(rng.integers(0, 2))] = BAD[int(rng.integers(0, len(BAD)))]
    return m.astype(np.int32)


def _edge_problem():
    """image id: lines.  min_num_matches = 3."""
    num_lines = {2: 1, 3: 63, 5: 64, 7: 65, 11: 257, 13: 0, 17: 4097, 19: 10, 23: 12, 29: 300}
    rng = np.random.default_rng(7)
    m = {}
    m[(2, 3)] = _one_sided(rng, 1, 63, 9, 0)                       # the image of one line: nine matches name it, one is accepted
    m[(3, 5)] = _one_sided(rng, 63, 64, 63, None, num_bad=5)
    m[(7, 5)] = _one_sided(rng, 65, 64, 64, 0, num_bad=4)          # (larger, smaller): stored as (5, 7) with the columns swapped
    m[(5, 11)] = _one_sided(rng, 64, 257, 200, 0)
    m[(7, 11)] = _one_sided(rng, 65, 257, 65, 1, num_bad=6)
    m[(3, 7)] = np.zeros((0, 2), dtype=np.int32)                   # no match at all
    m[(3, 11)] = _one_sided(rng, 63, 257, 3, None)                 # exactly min_num_matches: not used
    m[(2, 11)] = _one_sided(rng, 1, 257, 4, 0)                     # one above
    m[(13, 3)] = np.array([(0, 1), (0, 2), (-1, 3), (5, 4), (2, 2)], dtype=np.int32)      # the image without lines: used, every match invalid
    m[(11, 11)] = _one_sided(rng, 257, 257, 30, None)              # a used self pair: connected, nothing added
    m[(23, 23)] = _one_sided(rng, 12, 12, 2, None)                 # an unused self pair
    m[(19, 5)] = np.stack([np.arange(10, 18), np.arange(8)], axis=1).astype(np.int32)      # every index of image 19 out of range: connected, no observation
    # two table tiles on image 17's side.  (17, 11) repeats on that side, lines 4095 and 4096 - either side of the tile edge - among the repeated ones
    first = np.concatenate([[4096, 4095, 4096, 4095, 0, 4096, 0, 4095], rng.integers(0, 4097, 249)])
    m[(17, 11)] = np.stack([first, rng.permutation(257)], axis=1).astype(np.int32)
    # (17, 29) repeats on image 29's side: 299 matches, more than a workgroup's stride, distinct lines of 17 up to the one past the tile edge
    by_hand = np.array([(4096, 7), (4095, 7), (4094, 8), (4093, 299), (4092, 299), (4091, 1), (4090, 1), (4089, 8), (4088, 2)])
    rest = _one_sided(rng, 4088, 300, 290, 1, num_bad=9)
    m[(17, 29)] = np.concatenate([by_hand, rest]).astype(np.int32)
    return m, num_lines, 3


@pytest.fixture(scope="module")
def edge():
    m, num_lines, min_num = _edge_problem()
    assert _independent_counts(m, num_lines, min_num)[3] == 0      # (no pair of this problem repeats on both sides)
    return m, num_lines, min_num, _run(m, num_lines, min_num)


def test_every_edge_in_one_problem(edge):
    m, num_lines, min_num, (rep, out, (graph, connected, flat)) = edge
    ids = sorted(num_lines)
    assert connected == [2, 3, 5, 7, 11, 13, 17, 19, 29] and rep.num_pairs_replayed == 0
    obs = dict(zip(ids, out["image_num_observations"].tolist()))
    assert obs[19] == 0 and obs[13] == 0 and obs[23] == 0 and obs[2] == 1 and obs[17] > 256      # connected without an observation: 13 and 19
    assert not graph.ExistsImage(19) and graph.NumCorrespondencesBetweenImages(5, 7) > 30
    assert rep.num_matches_bad_index == 5 + 4 + 6 + 5 + 8 + 9 and rep.num_matches_duplicate > 100
    far = flat.FindCorrespondences(17, 4096)      # the first line of the second table tile
    assert (29, 7) in far and len(far) <= 2


def test_two_builds_are_byte_equal_and_a_handle_takes_another_input(edge):
    m, num_lines, min_num, (rep, out, reference) = edge
    ids = sorted(num_lines)
    other = {pair: v for pair, v in list(m.items())[::2]}
    other_reference = _reference(other, num_lines, min_num)
    builder = CorrGraphBuilder([num_lines[i] for i in ids])
    try:
        for _ in range(2):
            r1, o1, p1 = _device(builder, m, ids, min_num)
            for key in out:
                assert o1[key].tobytes() == out[key].tobytes(), key
            _assert_equal(r1, o1, p1, m, num_lines, min_num, reference)
            r2, o2, p2 = _device(builder, other, ids, min_num)
            _assert_equal(r2, o2, p2, other, num_lines, min_num, other_reference)
        assert len(o2["corr_line"]) < len(o1["corr_line"])
    finally:
        builder.close()


def test_all_pairs_of_72_images_keep_pair_order():
    """every line has 71 neighbours, one per other image: a list longer than a wavefront, in ascending pair order whatever order the pairs came in"""
    rng = np.random.default_rng(11)
    ids = [3 * k + 1 for k in range(72)]
    num_lines = {i: 20 for i in ids}
    pairs = list(itertools.combinations(ids, 2))
    assert len(pairs) == 2556
    m = {}
    for k in rng.permutation(len(pairs)):
        a, b = pairs[int(k)]
        v = np.stack([rng.permutation(20), rng.permutation(20)], axis=1).astype(np.int32)
        m[(b, a) if rng.integers(0, 2) else (a, b)] = v
    reference = _reference(m, num_lines, 15)
    builder = CorrGraphBuilder([20] * 72)
    try:
        rep, out, pair_counts = _device(builder, m, ids, 15)
        rep2, out2, _ = _device(builder, m, ids, 15)
    finally:
        builder.close()
    _assert_equal(rep, out, pair_counts, m, num_lines, 15, reference)
    assert np.array_equal(np.diff(out["corr_start"]), np.full(72 * 20, 71))
    owner_image = out["corr_line"].reshape(72 * 20, 71) // 20
    assert all(np.array_equal(row, np.delete(np.arange(72), l // 20)) for l, row in enumerate(owner_image))      # pair order = ascending other image
    assert all(out2[key].tobytes() == out[key].tobytes() for key in out)


def test_pairs_with_repeats_on_both_sides_go_through_the_host_loop():
    rng = np.random.default_rng(5)
    num_lines = {1: 8, 2: 8, 3: 40, 4: 40, 5: 9}
    m = {(1, 2): np.array([(3, 2), (3, 7), (5, 7), (0, 0), (1, 1)], dtype=np.int32),      # the shadow case: (5, 7) is accepted because (3, 7) was not
         (4, 3): np.stack([rng.integers(-1, 41, 300), rng.integers(-1, 41, 300)], axis=1).astype(np.int32),      # both-sided, given (larger, smaller)
         (3, 5): np.stack([rng.integers(0, 40, 50), rng.integers(0, 9, 50)], axis=1).astype(np.int32),             # both-sided
         (1, 3): _one_sided(rng, 8, 40, 30, 0, num_bad=3),                                                         # one-sided: stays on the device
         (2, 4): _one_sided(rng, 8, 40, 8, None),
         (1, 5): np.array([(3, 2), (3, 7), (5, 7)], dtype=np.int32)}                                                 # both-sided but NOT used (3 matches)
    rep, out, (graph, _, _) = _run(m, num_lines, 3, replayed=3)
    assert graph.FindCorrespondences(1, 5)[0] == (2, 7) and graph.FindCorrespondences(1, 3)[0] == (2, 2)
    assert rep.replay_ms >= 0


def _call(builder, min_num_matches, pairs, start, matches):
    pr, st, mt = (np.ascontiguousarray(pairs, dtype=np.int32), np.ascontiguousarray(start, dtype=np.int64), np.ascontiguousarray(matches, dtype=np.int32))
    rep = _capi.CorrGraphReport()
    return _capi.lib().pp_corr_graph_build(builder._h, min_num_matches, len(pr), pr.ctypes.data_as(_capi.c_ip), st.ctypes.data_as(C.POINTER(C.c_int64)),
                                           mt.ctypes.data_as(_capi.c_ip), C.byref(rep))


def test_bad_arguments_are_refused_and_leave_the_graph_readable():
    num_lines = {1: 6, 2: 6, 3: 6}
    m = {(1, 2): np.array([(1, 4), (2, 5), (3, 0)], dtype=np.int32), (3, 1): np.array([(0, 1), (1, 2), (2, 3)], dtype=np.int32)}
    reference = _reference(m, num_lines, 2)
    seq = np.stack([np.arange(4), np.arange(4)], axis=1).reshape(-1)
    builder = CorrGraphBuilder([6, 6, 6])
    try:
        L, E = C.c_int64(), C.c_int64()
        assert _capi.lib().pp_corr_graph_num_entries(builder._h, C.byref(L), C.byref(E)) == _capi.PP_ERR_INVALID      # nothing built yet
        rep, out, pair_counts = _device(builder, m, [1, 2, 3], 2)
        _assert_equal(rep, out, pair_counts, m, num_lines, 2, reference)
        bad_calls = [(2, [(0, 1), (1, 0)], [0, 2, 4], seq),          # the same unordered pair twice
                     (2, [(0, 3)], [0, 4], seq), (2, [(-1, 1)], [0, 4], seq),      # an image position out of range
                     (2, [(0, 1)], [1, 4], seq),                     # match_start does not start at 0
                     (2, [(0, 1), (1, 2)], [0, 4, 2], seq),          # match_start decreases
                     (-1, [(0, 1)], [0, 4], seq)]                    # a negative min_num_matches
        for call in bad_calls:
            assert _call(builder, *call) == _capi.PP_ERR_INVALID, call
            again = builder.get()
            assert all(again[key].tobytes() == out[key].tobytes() for key in out)
            assert np.array_equal(builder.pair_counts(), pair_counts)
        small = np.zeros(1, dtype=np.int32)
        assert len(out["corr_line"]) == 12
        assert _capi.lib().pp_corr_graph_get(builder._h, None, small.ctypes.data_as(_capi.c_ip), 11, None, None, None) == _capi.PP_ERR_INVALID
        assert small[0] == 0
        assert _capi.lib().pp_corr_graph_get(builder._h, None, None, 0, None, None, None) == 0      # any pointer may be NULL
        assert _call(builder, 2, [(0, 1)], [0, 4], seq) == 0                                            # and a good call still builds
        assert len(builder.get()["corr_line"]) == 8
    finally:
        builder.close()


def test_an_empty_problem_and_an_empty_pair_list():
    for lines in ([], [5, 0, 3]):
        builder = CorrGraphBuilder(lines)
        try:
            rep = builder.build(np.zeros((0, 2), dtype=np.int32), [], 15)
            out = builder.get()
        finally:
            builder.close()
        assert rep.num_matches_in == 0 and rep.num_pairs_used == 0 and len(out["corr_line"]) == 0
        assert out["corr_start"].tolist() == [0] * (sum(lines) + 1) and not out["image_connected"].any()


def test_the_wrapper_ignores_pairs_of_unknown_images_and_returns_the_mirrors_graph(edge):
    m, num_lines, min_num, (_, out, (graph, connected, flat)) = edge
    with_unknown = dict(m)
    with_unknown[(2, 1000)] = np.stack([np.zeros(6), np.arange(6)], axis=1).astype(np.int32)
    reports = []
    got, got_connected = fm.build_correspondence_graph_on_device(with_unknown, num_lines, min_num, report=reports)
    assert got_connected == connected == fm.build_correspondence_graph(with_unknown, num_lines, min_num)[1]
    assert np.array_equal(got.corr_start, flat.corr_start) and np.array_equal(got.corr_line, flat.corr_line) and got.image_ids == flat.image_ids
    assert reports[0].num_pairs_replayed == 0 and reports[0].num_matches_in == sum(len(v) for v in m.values())
    for i in (2, 5, 17):
        for x in (0, num_lines[i] - 1):
            assert got.FindCorrespondences(i, x) == graph.FindCorrespondences(i, x)


def test_from_the_descriptors_to_the_graph_through_match_to_graph():
    """the matcher's own output (ascending, distinct first indices; distinct second indices under the cross-check) never needs the host loop"""
    import bundle_setup_worlds as bsw
    rec = bsw.world(5, 60, 4)
    rng = np.random.default_rng(3)
    point_ids = sorted(rec.points3D)
    unit = rng.gamma(0.6, 1.0, size=(len(point_ids), 128))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    row = {p: k for k, p in enumerate(point_ids)}
    descriptors, num_lines = {}, {}
    for iid in sorted(rec.images):
        lines = rec.images[iid].lines
        d = synthetic.sift_like_descriptors(rng, len(lines))
        with_point = [x for x, l in enumerate(lines) if l.HasPoint3D()]
        d[with_point] = synthetic.sift_like_descriptors(rng, len(with_point), base=unit[[row[lines[x].Point3DId()] for x in with_point]], noise=0.6)
        descriptors[iid], num_lines[iid] = d, len(lines)
    pairs = fm.exhaustive_image_pairs(sorted(descriptors), block_size=2)
    matcher = fm.FeatureMatcher(fm.SiftMatchingOptions(), descriptors)
    try:
        matches = matcher.Match(pairs)
        got, got_connected = matcher.MatchToGraph(pairs, num_lines, min_num_matches=15)
    finally:
        matcher.close()
    want, want_connected = fm.build_correspondence_graph(matches, num_lines, min_num_matches=15)
    flat = FlatCorrespondenceGraph.from_graph(want, num_lines)
    assert got_connected == want_connected and len(want_connected) >= 4 and len(flat.corr_line) > 50
    assert np.array_equal(got.corr_start, flat.corr_start) and np.array_equal(got.corr_line, flat.corr_line)
    a, _, _ = IncrementalTriangulator(got, rec).flatten()
    b, _, _ = IncrementalTriangulator(want, rec).flatten()
    assert np.array_equal(a["corr_start"], b["corr_start"]) and np.array_equal(a["corr_line"], b["corr_line"])
    assert _independent_counts(matches, num_lines, 15)[3] == 0


def test_tracks_handle_from_the_device_built_graph_completes_and_merges_alike():
    """a small completion scene: its graph is turned into match lists per image pair, and the graph built from them on the device must drive
    CompleteAllTracks and MergeAllTracks to the result the dict graph built from the same lists gives"""
    import copy
    sc = synthetic.make_completion_scene(20, 150, 10, seed=1, noise_point=1e-4, noise_t=1e-5, noise_q=1e-5)
    rec, scene_graph = reconstruction_from_completion_scene(sc)
    ids = sorted(rec.images)
    num_lines = {i: len(rec.images[i].lines) for i in ids}
    matches = {}
    for a, b in itertools.combinations(ids, 2):
        v = scene_graph.FindCorrespondencesBetweenImages(a, b)
        if v:
            matches[(a, b)] = np.array(v, dtype=np.int32)
    reports = []
    dict_graph, _ = fm.build_correspondence_graph(matches, num_lines, min_num_matches=0)
    flat_graph, _ = fm.build_correspondence_graph_on_device(matches, num_lines, min_num_matches=0, report=reports)
    assert reports[0].num_matches_accepted > 500
    results = []
    for graph in (dict_graph, flat_graph):
        r = copy.deepcopy(rec)
        t = IncrementalTriangulator(graph, r)
        done = t.CompleteAndMergeAllTracks(IncrementalTriangulator.Options())
        results.append((done, {p: (pt.xyz.tolist(), list(pt.track)) for p, pt in r.points3D.items()}))
    assert results[0][0] == results[1][0] and results[0][1] == results[1][1]
    assert results[0][0][0] > 0 and results[0][0][1] > 0
