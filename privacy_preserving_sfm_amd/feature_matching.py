"""Host mirror of the reference's descriptor matching up to the correspondence graph, on top of pp_sift_* (include/ppsfm_hip.h, K17):
`SiftMatchingOptions` (feature/sift.h:117-145), `MatchSiftFeatures` (the rule of MatchSiftFeaturesCPUBruteForce, feature/sift.cc:957-970),
the pairs of `ExhaustiveFeatureMatcher::Run` (feature/matching.cc:436-498), `SiftFeatureMatcher::Match` (:345-422) and the part of
`DatabaseCache::Load` that turns the stored matches into a `CorrespondenceGraph` (base/database_cache.cc:82-191, base/correspondence_graph.cc:56-163).

The privacy-preserving pipeline has no geometric verification: what the matcher emits goes unchanged into the database and from there into the graph.
Feature extraction and the SQLite database are not mirrored.  There is no host fall-back for the
match itself: every call needs the device.  The graph has both forms: `build_correspondence_graph` on the host, dict-based, and
`build_correspondence_graph_on_device` (pp_corr_graph_*, K18), which returns the same graph as arrays.

Which pairs are matched (K20): besides the exhaustive list, the sequential, spatial and transitive selections of feature/matching.cc:512-874.  Each has
a host mirror in numpy (`sequential_image_pairs`, `spatial_image_pairs`, `transitive_image_pairs`); the spatial and the transitive one also run on the
device (pp_pairs_*, `spatial_image_pairs_on_device`, `transitive_image_pairs_on_device`) with the same result, pair for pair and bit for bit.  The
vocabulary-tree selection and the image-pairs / feature-pairs files are not mirrored."""
import numpy as np

from .device import CorrGraphBuilder, PairSelector, SiftMatcher, sift_match_options
from .incremental_triangulator import CorrespondenceGraph, FlatCorrespondenceGraph


class SiftMatchingOptions:
    """feature/sift.h:117-145, the reference's defaults.  num_threads, use_gpu and gpu_index are carried for completeness; max_num_matches only truncates
    the inputs of the reference's SiftGPU path and is not read by the brute-force rule, nor here."""

    def __init__(self, **kw):
        self.num_threads = -1
        self.use_gpu = True
        self.gpu_index = "-1"
        self.max_ratio = 0.8
        self.max_distance = 0.7
        self.cross_check = True
        self.max_num_matches = 32768
        self.min_num_matches = 15
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)

    def Check(self):
        if self.use_gpu and not [x for x in str(self.gpu_index).split(",") if x.strip()]:
            return False
        return self.max_ratio > 0.0 and self.max_distance > 0.0 and self.min_num_matches >= 0

    def device_options(self, min_num_matches=None, workspace_bytes=0):
        return sift_match_options(max_ratio=float(self.max_ratio), max_distance=float(self.max_distance), cross_check=int(bool(self.cross_check)),
                                  min_num_matches=int(self.min_num_matches if min_num_matches is None else min_num_matches),
                                  workspace_bytes=int(workspace_bytes))


def MatchSiftFeatures(options, descriptors1, descriptors2, device=0):
    """MatchSiftFeaturesCPUBruteForce: -> [n, 2] int32 (line_idx1, line_idx2), ascending in line_idx1.  min_num_matches is the pair rule of
    SiftFeatureMatcher::Match, not of this function: every match is returned."""
    if not options.Check():
        raise ValueError("SiftMatchingOptions.Check() failed")
    m = SiftMatcher([descriptors1, descriptors2], device=device)
    try:
        _, out = m.match_pairs([(0, 1)], options.device_options(min_num_matches=0))
    finally:
        m.close()
    return out[0]


def exhaustive_image_pairs(image_ids, block_size=50):
    """The pairs ExhaustiveFeatureMatcher::Run hands to the matcher (feature/matching.cc:455-488), block by block, in its order: every unordered pair of
    image_ids exactly once."""
    if block_size <= 1:
        raise ValueError("block_size must be larger than 1")      # ExhaustiveMatchingOptions::Check
    ids = list(image_ids)
    n, pairs = len(ids), []
    for start1 in range(0, n, block_size):
        end1 = min(n, start1 + block_size) - 1
        for start2 in range(0, n, block_size):
            end2 = min(n, start2 + block_size) - 1
            for idx1 in range(start1, end1 + 1):
                for idx2 in range(start2, end2 + 1):
                    b1, b2 = idx1 % block_size, idx2 % block_size
                    if (idx1 > idx2 and b1 <= b2) or (idx1 < idx2 and b1 < b2):
                        pairs.append((ids[idx1], ids[idx2]))
    return pairs


class _Options:
    def __init__(self, **kw):
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


class SequentialMatchingOptions(_Options):
    """feature/matching.h:56-64, Check() of matching.cc:63-66"""
    overlap = 10
    quadratic_overlap = True

    def Check(self):
        return self.overlap > 0


class SpatialMatchingOptions(_Options):
    """feature/matching.h:66-82, Check() of matching.cc:68-72"""
    is_gps = True
    ignore_z = True
    max_num_neighbors = 50
    max_distance = 100.0

    def Check(self):
        return self.max_num_neighbors > 0 and self.max_distance > 0.0


class TransitiveMatchingOptions(_Options):
    """feature/matching.h:84-92, Check() of matching.cc:74-78"""
    batch_size = 1000
    num_iterations = 3

    def Check(self):
        return self.batch_size > 0 and self.num_iterations > 0


def sequential_image_pairs(names_by_image_id, overlap=10, quadratic_overlap=True):
    """The pairs SequentialFeatureMatcher::RunSequentialMatching hands to the matcher (feature/matching.cc:551-592), image by image in the order of the
    image names: (i1, i1 + i) for i < overlap and, with quadratic_overlap, (i1, i1 + 2**i) behind each.  Self pairs (i = 0) and repeats are emitted as the
    reference emits them; FeatureMatcher.Match drops them.  2**i is a Python integer: it does not wrap as the reference's 1 << i does from i = 31 on."""
    if overlap <= 0:
        raise ValueError("overlap must be positive")      # SequentialMatchingOptions::Check
    ids = sorted(sorted(names_by_image_id), key=lambda i: names_by_image_id[i])
    n, pairs = len(ids), []
    for i1 in range(n):
        for i in range(overlap):
            if i1 + i >= n:
                break
            pairs.append((ids[i1], ids[i1 + i]))
            if quadratic_overlap and i1 + 2 ** i < n:
                pairs.append((ids[i1], ids[i1 + 2 ** i]))
    return pairs


class GPSTransform:
    """base/gps.cc:38-83: ellipsoidal (latitude, longitude in degrees, altitude in metres) to earth-centred cartesian metres, in float64."""
    GRS80, WGS84 = 0, 1

    def __init__(self, ellipsoid=1):
        if ellipsoid == self.GRS80:
            self.a_, self.b_, self.f_ = 6378137.0, 6.356752314140356e+06, 0.003352810681182
        elif ellipsoid == self.WGS84:
            self.a_, self.b_, self.f_ = 6378137.0, 6.356752314245179e+06, 0.003352810664747
        else:
            raise ValueError("Ellipsoid not defined")
        self.e2_ = (self.a_ * self.a_ - self.b_ * self.b_) / (self.a_ * self.a_)

    def EllToXYZ(self, ell):
        ell = np.asarray(ell, dtype=np.float64).reshape(-1, 3)
        deg = 0.0174532925199432954743716805978692718781530857086181640625      # util/math.h DegToRad
        lat, lon, alt = ell[:, 0] * deg, ell[:, 1] * deg, ell[:, 2]
        sin_lat, sin_lon, cos_lat, cos_lon = np.sin(lat), np.sin(lon), np.cos(lat), np.cos(lon)
        N = self.a_ / np.sqrt(1 - self.e2_ * sin_lat * sin_lat)
        return np.stack([(N + alt) * cos_lat * cos_lon, (N + alt) * cos_lat * sin_lon, (N * (1 - self.e2_) + alt) * sin_lat], axis=1)


def spatial_locations(tvec_prior_by_image_id, options):
    """The location matrix of SpatialFeatureMatcher::Run (feature/matching.cc:626-670) -> (location_image_ids, xyz float32 [m, 3]).  The images in
    ascending id; one is skipped when its prior is unset: (0, 0, *) with ignore_z, (0, 0, 0) without.  GPS priors go through GPSTransform.EllToXYZ, the
    third component zeroed before when ignore_z; the cast to float32 comes last.  Host only: the mirror and the device route read this one array."""
    ids, rows = [], []
    for image_id in sorted(tvec_prior_by_image_id):
        p = np.asarray(tvec_prior_by_image_id[image_id], dtype=np.float64).reshape(3)
        if p[0] == 0 and p[1] == 0 and (options.ignore_z or p[2] == 0):
            continue
        ids.append(image_id)
        rows.append((p[0], p[1], 0.0 if options.ignore_z else p[2]))
    ell = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    xyz = GPSTransform().EllToXYZ(ell) if options.is_gps else ell
    return ids, np.ascontiguousarray(xyz, dtype=np.float32)


def spatial_pair_positions(xyz, max_num_neighbors, max_distance, block=512):
    """The neighbour lists of feature/matching.cc:705-768 over location INDICES -> (pairs [n, 2] int32 (query, neighbour), sqdist [n] float32), query by
    query.  The search is FLANN's LinearIndex with L2<float>: the squared distance is ((d0*d0) + d1*d1) + d2*d2 in float32, every operation rounded on its
    own (numpy never fuses), and the candidates of a query come ordered by (squared distance, index) - KNNSimpleResultSet::addPoint puts a point behind
    those of equal distance and the points arrive in index order.  A distance is >= +0 and never NaN, so its bits order as an unsigned integer and
    bits << 32 | index is the whole order in one uint64.  Of the first knn = min(max_num_neighbors, m) the query itself is dropped and the list is cut at
    the first distance > float32(max_distance**2)."""
    if max_num_neighbors <= 0 or not max_distance > 0:
        raise ValueError("SpatialMatchingOptions.Check() failed")
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    if not np.isfinite(xyz).all():
        raise ValueError("a location is not finite")
    m = xyz.shape[0]
    knn = min(int(max_num_neighbors), m)
    cut = np.float32(float(max_distance) * float(max_distance))
    index = np.arange(m, dtype=np.uint64)
    out_pairs, out_dist = [], []
    for q0 in range(0, m, block):
        a = xyz[q0:q0 + block]
        with np.errstate(over="ignore"):
            d0, d1, d2 = (a[:, None, k] - xyz[None, :, k] for k in range(3))
            sq = ((d0 * d0) + d1 * d1) + d2 * d2
        keys = (sq.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index[None, :]
        if knn < m:
            keys = np.partition(keys, knn - 1, axis=1)[:, :knn]
        keys = np.sort(keys, axis=1)
        nn = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        dist = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
        query = np.arange(q0, q0 + a.shape[0], dtype=np.int64)[:, None]
        keep = (nn != query) & ~np.maximum.accumulate(dist > cut, axis=1)
        rows, cols = np.nonzero(keep)      # row-major: query by query, in list order
        out_pairs.append(np.stack([rows + q0, nn[rows, cols]], axis=1).astype(np.int32))
        out_dist.append(dist[rows, cols])
    if not out_pairs:
        return np.zeros((0, 2), dtype=np.int32), np.zeros(0, dtype=np.float32)
    return np.concatenate(out_pairs), np.concatenate(out_dist)


def _pairs_of_ids(location_image_ids, positions):
    ids = list(location_image_ids)
    return [(ids[a], ids[b]) for a, b in positions.tolist()]


def spatial_image_pairs(location_image_ids, xyz, options):
    """spatial_pair_positions in image ids: -> ([(image_id, nn_image_id)], sqdist float32), the pairs SpatialFeatureMatcher::Run hands to the matcher."""
    if not options.Check():
        raise ValueError("SpatialMatchingOptions.Check() failed")
    positions, sqdist = spatial_pair_positions(xyz, options.max_num_neighbors, options.max_distance)
    return _pairs_of_ids(location_image_ids, positions), sqdist


def spatial_image_pairs_on_device(location_image_ids, xyz, options, device=0, report=None):
    """spatial_image_pairs on the device (pp_pairs_spatial, K20): the same arguments, the same pairs in the same order, the same distance bits."""
    if not options.Check():
        raise ValueError("SpatialMatchingOptions.Check() failed")
    selector = PairSelector(device=device)
    try:
        rep, positions, sqdist = selector.spatial(xyz, options.max_num_neighbors, options.max_distance)
    finally:
        selector.close()
    if report is not None:
        report.append(rep)
    return _pairs_of_ids(location_image_ids, positions), sqdist


def _image_ids(num_or_ids):
    return list(range(num_or_ids)) if isinstance(num_or_ids, (int, np.integer)) else sorted(num_or_ids)


def transitive_pair_lists(num_or_ids, matches_so_far):
    """-> (image ids ascending, matched [k, 2], tried [t, 2]) as image POSITIONS: what one iteration of the transitive selection reads of the matches.
    matched: the pairs with a non-empty list (Database::ReadNumMatches reads WHERE rows > 0); tried: every key - an empty list means the pair has been
    matched before with no result, and Database::ExistsMatches answers true for it."""
    ids = _image_ids(num_or_ids)
    index = {i: k for k, i in enumerate(ids)}
    tried = np.asarray([(index[a], index[b]) for a, b in matches_so_far], dtype=np.int32).reshape(-1, 2)
    filled = np.asarray([len(m) > 0 for m in matches_so_far.values()], dtype=bool)
    return ids, np.ascontiguousarray(tried[filled]), tried


def transitive_pair_positions(num_images, matched, tried):
    """One iteration of TransitiveFeatureMatcher::Run (feature/matching.cc:818-869) over image positions: adjacency from `matched`; a candidate is {a, c},
    a != c, with a common neighbour; it is dropped when it is in `tried` or `matched`, in either orientation -> [n, 2] int32, a < c, ascending.  (The
    reference leaves order and orientation to unordered_map iteration; the set is the same.)"""
    matched = np.asarray(matched, dtype=np.int64).reshape(-1, 2)
    done = np.concatenate([matched, np.asarray(tried, dtype=np.int64).reshape(-1, 2)])

    def lists(pairs):
        ends = np.concatenate([pairs, pairs[:, ::-1]])
        ends = ends[np.argsort(ends[:, 0], kind="stable")]
        start = np.searchsorted(ends[:, 0], np.arange(num_images + 1))
        return start, ends[:, 1]

    mstart, madj = lists(matched)
    tstart, tadj = lists(done)
    out = []
    for a in range(num_images):
        if mstart[a] == mstart[a + 1]:
            continue
        two = np.unique(np.concatenate([madj[mstart[b]:mstart[b + 1]] for b in madj[mstart[a]:mstart[a + 1]]]))
        two = np.setdiff1d(two[two > a], tadj[tstart[a]:tstart[a + 1]])
        if two.size:
            out.append(np.stack([np.full(two.size, a, dtype=np.int64), two], axis=1))
    return np.concatenate(out).astype(np.int32) if out else np.zeros((0, 2), dtype=np.int32)


def transitive_image_pairs(num_or_ids, matches_so_far):
    """One iteration of the transitive selection on {(image_id1, image_id2): matches}: -> [(a, c)], a < c, ascending, in image ids.  num_or_ids: the
    image ids, or their number n for the ids 0 .. n - 1."""
    ids, matched, tried = transitive_pair_lists(num_or_ids, matches_so_far)
    return _pairs_of_ids(ids, transitive_pair_positions(len(ids), matched, tried))


def transitive_image_pairs_on_device(num_or_ids, matches_so_far, device=0, report=None):
    """transitive_image_pairs on the device (pp_pairs_transitive, K20): the same arguments, the same list."""
    ids, matched, tried = transitive_pair_lists(num_or_ids, matches_so_far)
    selector = PairSelector(device=device)
    try:
        rep, positions = selector.transitive(len(ids), matched, tried)
    finally:
        selector.close()
    if report is not None:
        report.append(rep)
    return _pairs_of_ids(ids, positions)


def run_transitive_matching(matcher, matches_so_far, options, on_device=False, device=0):
    """TransitiveFeatureMatcher::Run's loop: num_iterations times select the pairs from the matches so far, match them, merge the result -> the merged
    {pair: matches}.  matcher: anything with image_ids_ and Match(image_pairs).  batch_size only slices the Match calls: the adjacency is read once per
    iteration, so it cannot change the set."""
    if not options.Check():
        raise ValueError("TransitiveMatchingOptions.Check() failed")
    matches = dict(matches_so_far)
    for _ in range(options.num_iterations):
        if on_device:
            pairs = transitive_image_pairs_on_device(matcher.image_ids_, matches, device=device)
        else:
            pairs = transitive_image_pairs(matcher.image_ids_, matches)
        for start in range(0, len(pairs), options.batch_size):
            matches.update(matcher.Match(pairs[start:start + options.batch_size]))
    return matches


class FeatureMatcher:
    """SiftFeatureMatcher on one device: the descriptors of all images are uploaded once, Match() matches a list of image-id pairs in one call."""

    def __init__(self, options, descriptors_by_image_id, device=0, workspace_bytes=0):
        if not options.Check():
            raise ValueError("SiftMatchingOptions.Check() failed")
        self.options_ = options
        self.image_ids_ = sorted(descriptors_by_image_id)
        self._index = {i: k for k, i in enumerate(self.image_ids_)}
        self._workspace_bytes = workspace_bytes
        self._device = device
        self._matcher = SiftMatcher([descriptors_by_image_id[i] for i in self.image_ids_], device=device)
        self.last_report = None

    @classmethod
    def from_matcher(cls, options, image_ids, sift_matcher, device=0, workspace_bytes=0):
        """A FeatureMatcher over a device.SiftMatcher that exists already (SiftExtractor.extract_to_matcher): image_ids[k] is the id of the matcher's
        image k.  The matcher is owned from here on: close() closes it.  device: the matcher's, for the pair selections that run there."""
        if not options.Check():
            raise ValueError("SiftMatchingOptions.Check() failed")
        image_ids = list(image_ids)
        if len(image_ids) != sift_matcher.num_images or len(set(image_ids)) != len(image_ids):
            raise ValueError("one distinct image id per image of the matcher")
        self = cls.__new__(cls)
        self.options_ = options
        self.image_ids_ = sorted(image_ids)
        self._index = {i: k for k, i in enumerate(image_ids)}
        self._workspace_bytes = workspace_bytes
        self._device = device
        self._matcher = sift_matcher
        self.last_report = None
        return self

    def close(self):
        self._matcher.close()

    def Match(self, image_pairs):
        """-> {(image_id1, image_id2): [n, 2] matches} in the order given.  Self pairs and pairs seen before - in either order - are dropped
        (feature/matching.cc:369-382); a pair with fewer than min_num_matches matches gets an empty list (:414-416)."""
        seen, kept = set(), []
        for id1, id2 in image_pairs:
            if id1 == id2:
                continue
            key = (min(id1, id2), max(id1, id2))
            if key in seen:
                continue
            seen.add(key)
            kept.append((id1, id2))
        if not kept:
            return {}
        rep, out = self._matcher.match_pairs([(self._index[a], self._index[b]) for a, b in kept],
                                             self.options_.device_options(workspace_bytes=self._workspace_bytes))
        self.last_report = rep
        return {pair: m for pair, m in zip(kept, out)}

    def MatchSequential(self, names_by_image_id, options=None):
        """SequentialFeatureMatcher::Run: Match on sequential_image_pairs."""
        options = options or SequentialMatchingOptions()
        if not options.Check():
            raise ValueError("SequentialMatchingOptions.Check() failed")
        return self.Match(sequential_image_pairs(names_by_image_id, options.overlap, options.quadratic_overlap))

    def MatchSpatial(self, tvec_prior_by_image_id, options=None, on_device=True):
        """SpatialFeatureMatcher::Run: Match on the spatial selection over the location priors (K20 on this matcher's device, or the host mirror)."""
        options = options or SpatialMatchingOptions()
        ids, xyz = spatial_locations(tvec_prior_by_image_id, options)
        if on_device:
            pairs, _ = spatial_image_pairs_on_device(ids, xyz, options, device=self._device)
        else:
            pairs, _ = spatial_image_pairs(ids, xyz, options)
        return self.Match(pairs)

    def MatchTransitive(self, matches_so_far, options=None, on_device=True):
        """TransitiveFeatureMatcher::Run on the matches so far: run_transitive_matching with this matcher -> matches_so_far with the new pairs merged in."""
        return run_transitive_matching(self, matches_so_far, options or TransitiveMatchingOptions(), on_device=on_device, device=self._device)

    def MatchToGraph(self, image_pairs, num_lines_by_image, min_num_matches=15):
        """Match, then build_correspondence_graph_on_device on its output -> (FlatCorrespondenceGraph, the sorted ids of the connected images).
        min_num_matches is the mapper's option (a pair is used with MORE matches), not the matcher's of the same name."""
        return build_correspondence_graph_on_device(self.Match(image_pairs), num_lines_by_image, min_num_matches, device=self._device)


def build_correspondence_graph(matches, num_lines_by_image, min_num_matches=15):
    """DatabaseCache::Load's graph (base/database_cache.cc:82-191) from {(image_id1, image_id2): [n, 2] matches}: the database stores a pair under
    image_id1 < image_id2 (the columns swapped otherwise) and reads the pairs back in ascending pair id; a pair is USED when it has MORE than
    min_num_matches matches (the mapper's option, strict - not the matcher's option of the same name); only images of a used pair are added;
    AddCorrespondences (base/correspondence_graph.cc:79-163) skips a match whose line index does not exist and one whose line already corresponds to
    the other image.  -> (incremental_triangulator.CorrespondenceGraph, the sorted ids of the connected images)."""
    stored = {}
    for (id1, id2), m in matches.items():
        m = np.asarray(m, dtype=np.int64).reshape(-1, 2)
        if id1 > id2:
            id1, id2, m = id2, id1, m[:, ::-1]
        if len(m) == 0:
            continue      # (ReadAllMatches: WHERE rows > 0)
        stored[(id1, id2)] = m
    used = [pair for pair in sorted(stored) if len(stored[pair]) > min_num_matches and pair[0] in num_lines_by_image and pair[1] in num_lines_by_image]
    connected = sorted({i for pair in used for i in pair})
    graph = CorrespondenceGraph()
    for id1, id2 in used:
        if id1 == id2:
            continue      # "Cannot use self-matches"
        n1, n2 = num_lines_by_image[id1], num_lines_by_image[id2]
        for x1, x2 in stored[(id1, id2)]:
            x1, x2 = int(x1), int(x2)
            if not (0 <= x1 < n1 and 0 <= x2 < n2):
                continue
            if any(i == id2 for i, _ in graph.FindCorrespondences(id1, x1)) or any(i == id1 for i, _ in graph.FindCorrespondences(id2, x2)):
                continue
            graph.AddCorrespondence(id1, x1, id2, x2)
            graph.AddCorrespondence(id2, x2, id1, x1)
    return graph, connected


def build_correspondence_graph_on_device(matches, num_lines_by_image, min_num_matches=15, device=0, report=None):
    """build_correspondence_graph on the device (pp_corr_graph_build, K18): the same arguments, the same graph - as arrays.
    -> (incremental_triangulator.FlatCorrespondenceGraph over the images of num_lines_by_image, the sorted ids of the connected images).  A pair that
    names an image without an entry in num_lines_by_image is ignored.  report: a list the pp_corr_graph_report is appended to."""
    image_ids = sorted(num_lines_by_image)
    index = {i: k for k, i in enumerate(image_ids)}
    pairs, lists = [], []
    for (id1, id2), m in matches.items():
        if id1 in index and id2 in index:
            pairs.append((index[id1], index[id2]))
            lists.append(m)
    builder = CorrGraphBuilder([num_lines_by_image[i] for i in image_ids], device=device)
    try:
        rep = builder.build(pairs, lists, min_num_matches)
        out = builder.get()
    finally:
        builder.close()
    if report is not None:
        report.append(rep)
    graph = FlatCorrespondenceGraph(image_ids, builder.num_lines, out["corr_start"], out["corr_line"], out["image_connected"])
    return graph, [i for i, c in zip(image_ids, out["image_connected"]) if c]
