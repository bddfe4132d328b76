"""CPU-only checks of the host mirror in privacy_preserving_sfm_amd/feature_matching.py: exhaustive_image_pairs against a brute-force enumeration of the
block rule of ExhaustiveFeatureMatcher::Run (feature/matching.cc:455-488) - every unordered pair exactly once, also for image counts the block size does not
divide - and build_correspondence_graph (base/database_cache.cc:82-191, base/correspondence_graph.cc:79-163) on hand-made match lists: a duplicate, an
out-of-range index, a pair at exactly min_num_matches (unused) and an image left unconnected."""
import itertools

import numpy as np
import pytest

from privacy_preserving_sfm_amd import feature_matching as fm


def _brute_force_pairs(ids, block_size):
    """the rule restated without the block loops' bounds: all (idx1, idx2) with the duplicate filter, sorted by (block of idx1, block of idx2, idx1, idx2)"""
    n = len(ids)
    keep = []
    for idx1, idx2 in itertools.product(range(n), range(n)):
        b1, b2 = idx1 % block_size, idx2 % block_size
        if (idx1 > idx2 and b1 <= b2) or (idx1 < idx2 and b1 < b2):
            keep.append((idx1 // block_size, idx2 // block_size, idx1, idx2))
    return [(ids[a], ids[b]) for _, _, a, b in sorted(keep)]


@pytest.mark.parametrize("count,block_size", [(0, 3), (1, 3), (2, 2), (5, 2), (7, 3), (10, 4), (11, 50), (9, 3), (13, 5)])
def test_exhaustive_pairs_are_every_unordered_pair_once(count, block_size):
    ids = [3 * k + 11 for k in range(count)]      # ids are not indices
    pairs = fm.exhaustive_image_pairs(ids, block_size)
    assert pairs == _brute_force_pairs(ids, block_size)
    unordered = [frozenset(p) for p in pairs]
    assert all(len(p) == 2 for p in unordered)      # no self pair
    assert len(set(unordered)) == len(unordered) == count * (count - 1) // 2
    assert set(unordered) == {frozenset(p) for p in itertools.combinations(ids, 2)}


def test_exhaustive_pairs_refuse_a_block_size_of_one():
    with pytest.raises(ValueError):
        fm.exhaustive_image_pairs([1, 2, 3], 1)


def _seq(n, shift=0):
    return np.array([(k, k + shift) for k in range(n)], dtype=np.int32)


def test_the_graph_applies_the_database_cache_rules():
    num_lines = {1: 10, 2: 10, 3: 10, 4: 10, 5: 10}
    m12 = np.array([(0, 0), (1, 1), (2, 2), (2, 5), (6, 1), (3, 12), (11, 3), (4, 4)], dtype=np.int32)
    #   (2, 5): line 2 of image 1 already corresponds to image 2 - skipped;  (6, 1): line 1 of image 2 already corresponds to image 1 - skipped;
    #   (3, 12) and (11, 3): a line index that does not exist - skipped
    m31 = np.array([(5, 7), (6, 8), (7, 9)], dtype=np.int32)      # stored as (1, 3) with the columns swapped
    m24 = _seq(3)                                                   # exactly min_num_matches: NOT used (strict)
    m45 = _seq(2)                                                   # below
    graph, connected = fm.build_correspondence_graph({(1, 2): m12, (3, 1): m31, (2, 4): m24, (4, 5): m45}, num_lines, min_num_matches=3)
    assert connected == [1, 2]      # (3, 1) has 3 matches: not more than min_num_matches either
    assert graph.FindCorrespondences(1, 0) == [(2, 0)] and graph.FindCorrespondences(2, 0) == [(1, 0)]
    assert graph.FindCorrespondences(1, 2) == [(2, 2)] and graph.FindCorrespondences(2, 5) == []
    assert graph.FindCorrespondences(2, 1) == [(1, 1)] and graph.FindCorrespondences(1, 6) == []
    assert graph.FindCorrespondences(1, 3) == [] and graph.FindCorrespondences(2, 3) == []
    assert graph.FindCorrespondences(1, 4) == [(2, 4)]
    assert graph.FindCorrespondences(4, 0) == [] and graph.FindCorrespondences(5, 0) == []
    assert sorted(graph._corrs) == [(1, 0), (1, 1), (1, 2), (1, 4), (2, 0), (2, 1), (2, 2), (2, 4)]


def test_the_graph_reads_pairs_in_pair_id_order_with_swapped_columns():
    num_lines = {1: 6, 2: 6, 3: 6}
    m31 = np.array([(0, 1), (1, 2), (2, 3)], dtype=np.int32)      # image 3 first: the database stores (1, 3) with (line of 1, line of 3)
    m12 = np.array([(1, 4), (2, 5), (3, 0)], dtype=np.int32)
    m23 = np.array([(4, 0), (5, 1), (0, 2)], dtype=np.int32)
    graph, connected = fm.build_correspondence_graph({(3, 1): m31, (2, 3): m23, (1, 2): m12}, num_lines, min_num_matches=2)
    assert connected == [1, 2, 3]
    # image 1, line 1: pair (1, 2) comes before pair (1, 3) whatever the order of the dict
    assert graph.FindCorrespondences(1, 1) == [(2, 4), (3, 0)]
    assert graph.FindCorrespondences(3, 0) == [(1, 1), (2, 4)]
    assert graph.FindCorrespondences(2, 4) == [(1, 1), (3, 0)]
    assert graph.FindCorrespondences(1, 3) == [(2, 0), (3, 2)]


def test_an_image_without_lines_entry_is_ignored():
    graph, connected = fm.build_correspondence_graph({(1, 9): _seq(5)}, {1: 10}, min_num_matches=2)
    assert connected == [] and graph._corrs == {}
