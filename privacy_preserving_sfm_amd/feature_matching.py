"""Host mirror of the reference's descriptor matching up to the correspondence graph, on top of pp_sift_* (include/ppsfm_hip.h, K17):
`SiftMatchingOptions` (feature/sift.h:117-145), `MatchSiftFeatures` (the rule of MatchSiftFeaturesCPUBruteForce, feature/sift.cc:957-970),
the pairs of `ExhaustiveFeatureMatcher::Run` (feature/matching.cc:436-498), `SiftFeatureMatcher::Match` (:345-422) and the part of
`DatabaseCache::Load` that turns the stored matches into a `CorrespondenceGraph` (base/database_cache.cc:82-191, base/correspondence_graph.cc:56-163).

The privacy-preserving pipeline has no geometric verification: what the matcher emits goes unchanged into the database and from there into the graph.
Feature extraction, the SQLite database and the sequential / spatial / transitive pair selections are not mirrored.  There is no host fall-back for the
match itself: every call needs the device.  The graph has both forms: `build_correspondence_graph` on the host, dict-based, and
`build_correspondence_graph_on_device` (pp_corr_graph_*, K18), which returns the same graph as arrays."""
import numpy as np

from .device import CorrGraphBuilder, SiftMatcher, sift_match_options
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
