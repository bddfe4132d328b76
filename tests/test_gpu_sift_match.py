"""K17 on the device: pp_sift_top2 and pp_sift_match_pairs against tests/sift_match_reference.py (MatchSiftFeaturesCPUBruteForce in numpy, acosf from
this process's libm) with NO tolerance anywhere: integers, indices and match lists must be equal.

The kernel's tile edges: the i8 MFMA's 32 x 32 block, the workgroup's ROW tile of 128 query rows (4 wavefronts x 32) and its COLUMN tile of 64 scanned
rows staged in LDS (two MFMA blocks).  The sizes below lie on both sides of each - 31/32/33, 63/64/65, 127/128/129 - and of the next multiples (255/256/257:
more than one workgroup per direction, several column tiles), always with N1 != N2, each pair both ways round."""
import ctypes as C
import itertools

import numpy as np
import pytest

import sift_match_reference as ref
from privacy_preserving_sfm_amd import _capi, feature_matching as fm, synthetic
from privacy_preserving_sfm_amd.device import SiftMatcher, sift_match_options

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]
SIZE_PAIRS = [(1, 2), (31, 33), (32, 63), (64, 65), (127, 129), (128, 255), (256, 257), (2, 257), (33, 128), (65, 31)]


def _pool_images(sizes, seed, noise=0.8, pool=None):
    """one descriptor set per size: noisy copies of the first rows of a common pool at permuted positions, so that any two images share features"""
    rng = np.random.default_rng(seed)
    n = max(max(sizes), 1) if pool is None else pool
    unit = rng.gamma(0.6, 1.0, size=(n, 128))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    return [synthetic.sift_like_descriptors(rng, s, base=unit[rng.permutation(n)[:s]], noise=noise) if s else np.zeros((0, 128), dtype=np.uint8) for s in sizes]


def _equal_matches(got, want):
    assert got.shape == want.shape and np.array_equal(got, want), (got[:8], want[:8])


@pytest.fixture(scope="module")
def sized():
    images = _pool_images(SIZES, seed=5)
    m = SiftMatcher(images)
    yield images, m, {s: k for k, s in enumerate(SIZES)}
    m.close()


@pytest.mark.parametrize("n1,n2", SIZE_PAIRS + [(b, a) for a, b in SIZE_PAIRS], ids=lambda v: str(v))
def test_sizes_on_both_sides_of_every_tile_edge(sized, n1, n2):
    images, m, index = sized
    a, b = index[n1], index[n2]
    dists = ref.dist_matrix(images[a], images[b])
    for got, want in zip(m.top2(a, b), ref.top2(dists)):
        assert np.array_equal(got, want)
    rep, out = m.match_pairs([(a, b)], sift_match_options(min_num_matches=0))
    _equal_matches(out[0], ref.match(images[a], images[b]))
    assert rep.num_matches == len(out[0]) and rep.num_batches == 1 and rep.num_pairs_emptied == 0


def test_every_size_is_used():
    assert set(SIZES) == {n for p in SIZE_PAIRS for n in p}


def test_an_empty_image_on_either_side_gives_no_match():
    images = _pool_images([0, 40], seed=6)
    m = SiftMatcher(images)
    try:
        bj, b, s = m.top2(1, 0)
        assert np.array_equal(bj, np.full(40, -1)) and not b.any() and not s.any()
        assert all(len(x) == 0 for x in m.top2(0, 1))
        rep, out = m.match_pairs([(0, 1), (1, 0), (0, 0)], sift_match_options(min_num_matches=0))
        assert [len(x) for x in out] == [0, 0, 0] and rep.num_matches == 0
        rep, out = m.match_pairs([], sift_match_options())
        assert out == [] and rep.num_batches == 0
    finally:
        m.close()


def test_the_operand_layout_with_asymmetric_data():
    """each row of d1 carries its index in byte 0 and one large byte at a position of its own; d2 is a pattern that is symmetric in nothing.  A swapped
    row / column in the C map, or a fragment read with the wrong k stride, changes best_j."""
    n1, n2 = 40, 70
    d1 = np.zeros((n1, 128), dtype=np.uint8)
    d1[:, 0] = np.arange(n1) + 1
    d1[np.arange(n1), (3 * np.arange(n1) + 1) % 128] = 200
    j, k = np.meshgrid(np.arange(n2), np.arange(128), indexing="ij")
    d2 = ((7 * j + 13 * k * k + j * k) % 251).astype(np.uint8)
    dists = ref.dist_matrix(d1, d2)
    want = ref.top2(dists)
    assert len(set(want[0].tolist())) > 10      # the answer depends on the row
    m = SiftMatcher([d1, d2])
    try:
        for got, w in zip(m.top2(0, 1), want):
            assert np.array_equal(got, w)
        for got, w in zip(m.top2(1, 0), ref.top2(dists.T)):
            assert np.array_equal(got, w)
        for cross in (1, 0):
            _, out = m.match_pairs([(0, 1), (1, 0)], sift_match_options(min_num_matches=0, cross_check=cross, max_distance=3.0, max_ratio=1.0))
            _equal_matches(out[0], ref.match(d1, d2, 1.0, 3.0, bool(cross)))
            _equal_matches(out[1], ref.match(d2, d1, 1.0, 3.0, bool(cross)))
    finally:
        m.close()


@pytest.mark.parametrize("n2", [64, 70, 129])
def test_extremes(n2):
    """all-255 rows (dist 8 323 200: the clamp to 1), all-zero rows (no match, best_j -1), the maximum in the first, the last and the last column before the
    padding of a column tile, and duplicated columns (a tie on the maximum takes the lowest index, second == best)"""
    rng = np.random.default_rng(n2)
    d2 = synthetic.sift_like_descriptors(rng, n2)
    d2[9] = 0
    d2[11] = d2[3]
    d2[n2 - 2] = d2[7]
    d1 = synthetic.sift_like_descriptors(rng, 12)
    d1[0] = 255                 # best is the all-255 column: 128 * 255^2
    d1[1] = 0                   # no positive dist
    d1[2] = d2[0]               # first column
    d1[3] = d2[n2 - 1]          # last column (with n2 = 70 or 129 the last before the padding, with 64 the last of a full tile)
    d1[4] = d2[3]               # columns 3 and 11 are equal
    d1[5] = d2[7]               # columns 7 and n2 - 2 are equal
    d3 = d2.copy()
    d3[5] = 255                 # (an all-255 column is every row's best: it gets an image of its own)
    dists = ref.dist_matrix(d1, d2)
    want = ref.top2(dists)
    assert want[0][1] == -1 and want[1][1] == 0 and want[2][1] == 0
    assert want[1][4] == want[2][4] and want[1][5] == want[2][5]
    want3 = ref.top2(ref.dist_matrix(d1, d3))
    assert want3[1][0] == 128 * 255 * 255 and want3[0][0] == 5 and (want3[0][[0, 2, 3, 4, 5]] == 5).all()
    m = SiftMatcher([d1, d2, d3])
    try:
        for g, w in zip(m.top2(0, 2), want3):
            assert np.array_equal(g, w)
        for g, w in zip(m.top2(2, 0), ref.top2(ref.dist_matrix(d3, d1))):
            assert np.array_equal(g, w)
        got = m.top2(0, 1)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        # the self products of the copies dominate (checked on the reference, stated here on the device's answer)
        assert got[0][2] == 0 and got[0][3] == n2 - 1 and got[0][4] == 3 and got[0][5] == 7
        assert got[1][4] == got[2][4] and got[1][5] == got[2][5]
        for g, w in zip(m.top2(1, 0), ref.top2(dists.T)):
            assert np.array_equal(g, w)
        for ratio in (0.8, 1.5):
            for cross in (1, 0):
                _, out = m.match_pairs([(0, 1), (1, 0), (0, 2), (2, 0)], sift_match_options(min_num_matches=0, max_ratio=ratio, cross_check=cross))
                _equal_matches(out[0], ref.match(d1, d2, ratio, 0.7, bool(cross)))
                _equal_matches(out[1], ref.match(d2, d1, ratio, 0.7, bool(cross)))
                _equal_matches(out[2], ref.match(d1, d3, ratio, 0.7, bool(cross)))
                _equal_matches(out[3], ref.match(d3, d1, ratio, 0.7, bool(cross)))
    finally:
        m.close()


@pytest.fixture(scope="module")
def generated():
    """300 x 280 with 200 shared features, duplicates and all-zero rows: distance rejections, ratio rejections, accepted rows, rows that fail the
    cross-check and rows whose best and second are equal are all present (asserted below on the reference)"""
    p = synthetic.make_descriptor_pair(300, 280, 200, 0.8, seed=1, duplicates=5, zero_rows=2)
    d1, d2 = p["d1"], p["d2"]
    d1[17] = d1[4]      # a duplicate on the first side too: with ties accepted the lowest index decides the cross-check
    m = SiftMatcher([d1, d2])
    yield d1, d2, m
    m.close()


def test_the_generated_pair_exercises_every_branch(generated):
    d1, d2, _ = generated
    bj, b, s = ref.top2(ref.dist_matrix(d1, d2))
    has = bj >= 0
    far = has & (ref.angle(b) > np.float32(0.7))
    ok = has & ref.accept(np.maximum(b, 1), s)
    assert far.sum() > 0 and (has & ~far & ~ok).sum() > 0 and ok.sum() > 0 and (~has).sum() > 0 and (has & (b == s)).sum() > 0
    assert len(ref.match(d1, d2)) < min(ok.sum(), len(ref.match(d1, d2, cross_check=False)))      # the cross-check drops some


@pytest.mark.parametrize("kw", [dict(), dict(max_ratio=1.5), dict(cross_check=0), dict(max_ratio=1.5, cross_check=0), dict(max_distance=1e-3),
                                dict(max_distance=3.0), dict(max_distance=3.0, max_ratio=1.5), dict(max_ratio=1e-3)], ids=str)
def test_options(generated, kw):
    d1, d2, m = generated
    o = sift_match_options(min_num_matches=0, **kw)
    _, out = m.match_pairs([(0, 1), (1, 0)], o)
    args = (o.max_ratio, o.max_distance, bool(o.cross_check))
    _equal_matches(out[0], ref.match(d1, d2, *args))
    _equal_matches(out[1], ref.match(d2, d1, *args))
    if kw == dict(max_ratio=1.5):
        assert len(out[0]) > len(ref.match(d1, d2))      # ties and weak ratios come through


def test_min_num_matches_one_above_and_one_below_the_count(generated):
    d1, d2, m = generated
    want = ref.match(d1, d2)
    n = len(want)
    assert n > 2
    rep, out = m.match_pairs([(0, 1)], sift_match_options(min_num_matches=n - 1))
    _equal_matches(out[0], want)
    assert rep.num_pairs_emptied == 0
    rep, out = m.match_pairs([(0, 1)], sift_match_options(min_num_matches=n))
    _equal_matches(out[0], want)
    rep, out = m.match_pairs([(0, 1), (1, 0), (0, 1)], sift_match_options(min_num_matches=n + 1))
    assert [len(x) for x in out] == [0, 0, 0] and rep.num_pairs_emptied == 3 and rep.num_matches == 0


BATCH_SIZES = [37, 0, 64, 129, 200, 90]


@pytest.fixture(scope="module")
def batch():
    images = _pool_images(BATCH_SIZES, seed=9, noise=0.5)
    pairs = [(a, b) for a, b in itertools.product(range(len(images)), repeat=2) if a != b]
    want = [ref.match_pair_rule(images[a], images[b]) for a, b in pairs]
    m = SiftMatcher(images)
    yield images, pairs, want, m
    m.close()


def test_thirty_ordered_pairs_in_one_call(batch):
    images, pairs, want, m = batch
    assert len(pairs) == 30 and sum(len(w) > 0 for w in want) >= 10 and sum(len(w) == 0 for w in want) >= 10
    rep, out = m.match_pairs(pairs)
    assert rep.num_batches == 1 and rep.num_matches == sum(len(w) for w in want)
    for got, w in zip(out, want):
        _equal_matches(got, w)
    for p in pairs[::4]:      # the per-pair calls
        _, single = m.match_pairs([p])
        _equal_matches(single[0], want[pairs.index(p)])
    raw = [ref.match(images[a], images[b]) for a, b in pairs]
    assert rep.num_pairs_emptied == sum(0 < len(r) < 15 for r in raw)


@pytest.mark.parametrize("workspace_bytes", [1, 6000, 20000])
def test_several_batches_under_a_small_workspace(batch, workspace_bytes):
    images, pairs, want, m = batch
    rep, out = m.match_pairs(pairs, sift_match_options(workspace_bytes=workspace_bytes))
    assert rep.num_batches > 1 and (workspace_bytes > 1 or rep.num_batches == 30)
    assert rep.num_matches == sum(len(w) for w in want)
    for got, w in zip(out, want):
        _equal_matches(got, w)


def test_a_capacity_one_short_is_refused_with_untouched_outputs(batch):
    images, pairs, want, m = batch
    need = sum(len(w) for w in want)
    pr = np.ascontiguousarray(pairs, dtype=np.int32)
    o, rep = sift_match_options(), _capi.SiftMatchReport()
    rep.num_matches = -7
    start, out = np.full(len(pairs) + 1, -3, dtype=np.int64), np.full((need, 2), -9, dtype=np.int32)
    call = lambda cap: _capi.lib().pp_sift_match_pairs(m._h, C.byref(o), len(pairs), _capi.ptr(pr, _capi.c_ip), C.byref(rep),
                                                       _capi.ptr(start, C.POINTER(C.c_int64)), _capi.ptr(out, _capi.c_ip), cap)
    assert call(need - 1) == _capi.PP_ERR_INVALID
    assert b"capacity" in _capi.lib().pp_last_error()
    assert (start == -3).all() and (out == -9).all() and rep.num_matches == -7
    assert call(need) == _capi.PP_OK and rep.num_matches == need and start[-1] == need
    assert np.array_equal(out, np.concatenate([w for w in want if len(w)]))


def test_a_self_pair_and_a_repeated_pair_are_matched_like_any_other(batch):
    images, pairs, want, m = batch
    _, out = m.match_pairs([(3, 3), (2, 4), (2, 4)], sift_match_options(min_num_matches=0))
    _equal_matches(out[0], ref.match(images[3], images[3]))
    _equal_matches(out[1], ref.match(images[2], images[4]))
    _equal_matches(out[2], out[1])


def test_bad_image_indices_are_refused(batch):
    _, _, _, m = batch
    i3 = (C.c_int32 * 300)()
    assert _capi.lib().pp_sift_top2(m._h, 0, 6, i3, i3, i3) == _capi.PP_ERR_INVALID
    assert _capi.lib().pp_sift_top2(m._h, -1, 0, i3, i3, i3) == _capi.PP_ERR_INVALID
    pr = (C.c_int32 * 2)(0, 6)
    rep, start = _capi.SiftMatchReport(), (C.c_int64 * 2)()
    o = sift_match_options()
    assert _capi.lib().pp_sift_match_pairs(m._h, C.byref(o), 1, pr, C.byref(rep), start, i3, 100) == _capi.PP_ERR_INVALID


def test_match_sift_features_is_the_reference_rule():
    p = synthetic.make_descriptor_pair(70, 45, 30, 0.5, seed=4, duplicates=2, zero_rows=1)
    for kw in (dict(), dict(cross_check=False), dict(max_ratio=1.5, min_num_matches=1000)):      # (min_num_matches is the pair rule, not this function's)
        o = fm.SiftMatchingOptions(**kw)
        _equal_matches(fm.MatchSiftFeatures(o, p["d1"], p["d2"]), ref.match(p["d1"], p["d2"], o.max_ratio, o.max_distance, o.cross_check))


def test_from_the_matches_to_the_correspondence_graph():
    """five images of a small world: every line gets a descriptor - noisy copies of its point's - and FeatureMatcher.Match over the exhaustive pairs,
    then build_correspondence_graph, gives the graph the reference's matches give: the same _corrs, lists in order, and the same flattened corr_start /
    corr_line"""
    import bundle_setup_worlds as bsw
    from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator
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
    ids = sorted(descriptors)
    pairs = fm.exhaustive_image_pairs(ids, block_size=2)
    assert len(pairs) == 10
    options = fm.SiftMatchingOptions()
    matcher = fm.FeatureMatcher(options, descriptors)
    try:
        got = matcher.Match(pairs + [(ids[0], ids[0]), (pairs[0][1], pairs[0][0])])      # a self pair and a duplicate: dropped
    finally:
        matcher.close()
    assert list(got) == pairs
    want = {(a, b): ref.match_pair_rule(descriptors[a], descriptors[b], options.min_num_matches) for a, b in pairs}
    for p in pairs:
        _equal_matches(got[p], want[p])
    g_got, c_got = fm.build_correspondence_graph(got, num_lines, min_num_matches=15)
    g_want, c_want = fm.build_correspondence_graph(want, num_lines, min_num_matches=15)
    assert c_got == c_want and len(c_want) >= 4 and len(g_want._corrs) > 50
    assert g_got._corrs == g_want._corrs
    flat_got, _, _ = IncrementalTriangulator(g_got, rec).flatten()
    flat_want, _, _ = IncrementalTriangulator(g_want, rec).flatten()
    assert np.array_equal(flat_got["corr_start"], flat_want["corr_start"]) and np.array_equal(flat_got["corr_line"], flat_want["corr_line"])
    assert len(flat_want["corr_line"]) > 50
