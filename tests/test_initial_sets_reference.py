"""The plain-Python reference of the image-set search (initial_sets_reference.py) on the hand-built graphs of initial_sets_scenes.py, against counts worked
out by hand here.  CPU only: this is the yardstick the device result and the replay header are compared with, so it is checked on its own first."""
from math import comb

import initial_sets_reference as ref
import initial_sets_scenes as scenes


def _run(scene):
    return ref.find_initial_sets(scene, **scene["options"])


def _summary(got):
    return [(tuple(s["images"]), s["num_aligned"], s["num_random"]) for s in got["sets"]]


def test_fewer_than_three_neighbours_give_no_track():
    got = _run(scenes.two_neighbours())
    assert got["num_candidates"] == 0 and got["work_lines"] == 0 and got["num_aligned_sets"] == 0 and got["sets"] == []


def test_three_neighbours_in_three_other_images_give_one_track():
    got = _run(scenes.three_neighbours())
    assert got["num_candidates"] == 1 and got["num_aligned_tracks"] == 1 and got["num_random_tracks"] == 0
    assert got["counts"] == {(0, 1, 2, 3): (1, 0)}
    assert got["sets"] == []      # no unaligned track: the set does not qualify, whatever the thresholds


def test_a_triple_with_two_lines_of_one_image_is_dropped():
    # r in image 0, neighbours in images 1, 1, 2, 3: of the C(4,3) = 4 triples the two holding both lines of image 1 go
    got = _run(scenes.two_neighbours_in_one_image())
    assert got["num_candidates"] == 2 and got["counts"] == {(0, 1, 2, 3): (2, 0)}


def test_a_neighbour_in_the_lines_own_image_is_dropped():
    # neighbours in images 0, 1, 2, 3: the three triples holding the line of image 0 collide with r's image
    got = _run(scenes.neighbour_in_own_image())
    assert got["num_candidates"] == 1 and got["counts"] == {(0, 1, 2, 3): (1, 0)}


def test_the_other_alignment_and_the_subset_filter_the_list():
    for scene in (scenes.neighbour_of_other_alignment(), scenes.neighbour_outside_subset()):
        got = _run(scene)      # four neighbours, one filtered: C(3,3) = 1 triple, not C(4,3) = 4
        assert got["num_candidates"] == 1 and got["counts"] == {(0, 1, 2, 3): (1, 0)}, scene


def test_a_one_directional_edge_counts_from_its_source_only():
    got = _run(scenes.one_directional())      # all four images are checked, only r has neighbours
    assert got["num_candidates"] == 1 and got["work_lines"] == 1 and got["num_aligned_tracks"] == 1


def test_a_track_reached_from_several_members_counts_once():
    for num_check in (1, 2, 4):
        got = _run(scenes.shared_track(num_check))
        assert got["num_candidates"] == 2 * num_check      # one per class and check image
        assert got["num_aligned_tracks"] == 1 and got["num_random_tracks"] == 1
        assert _summary(got) == [((0, 1, 2, 3), 1, 1)]
        assert got["sets"][0]["aligned"] == [(0, 2, 4, 6)] and got["sets"][0]["random"] == [(1, 3, 5, 7)]      # two lines per image, the aligned one first


def test_each_threshold_is_inclusive_and_separate():
    got = _run(scenes.thresholds())
    assert got["counts"] == {(0, 1, 2, 3): (3, 3), (0, 1, 2, 4): (2, 3), (0, 1, 3, 4): (3, 2), (0, 2, 3, 4): (5, 0)}
    assert got["num_aligned_sets"] == 4 and got["num_random_sets"] == 3 and got["num_qualified"] == 1
    assert _summary(got) == [((0, 1, 2, 3), 3, 3)]


def test_ties_are_ordered_by_ascending_image_set():
    got = _run(scenes.tied_sets())
    assert _summary(got) == [((1, 2, 3, 4), 4, 2), ((0, 1, 2, 3), 3, 2), ((0, 1, 2, 4), 3, 5)]


def test_only_the_first_ten_sets_are_returned():
    got = _run(scenes.more_sets_than_returned())
    assert got["num_qualified"] == 15 and len(got["sets"]) == 10
    # aligned counts 2 + k % 5 over the 15 quadruples in lexicographic order: three sets each of 6, 5, 4, 3, 2 - the tenth is the first of the 3s
    assert [s["num_aligned"] for s in got["sets"]] == [6, 6, 6, 5, 5, 5, 4, 4, 4, 3]
    sixes = [tuple(s["images"]) for s in got["sets"][:3]]
    assert sixes == sorted(sixes) and sixes == [(0, 1, 3, 5), (0, 3, 4, 5), (2, 3, 4, 5)]      # the 5th, 10th and 15th quadruple


def test_the_long_list():
    got = _run(scenes.long_list())
    assert got["work_lines"] == 2 and got["overflow_lines"] == 2
    assert got["num_candidates"] == 2 * comb(79, 3) and got["num_aligned_tracks"] == comb(79, 3) == got["num_random_sets"]
    assert got["num_qualified"] == comb(79, 3) and [tuple(s["images"]) for s in got["sets"]] == [(0, 1, 2, 3 + k) for k in range(10)]


def test_the_fuzz_qualifies_sets():
    """the fuzz is worth running only if sets qualify, some scenes cut the list and ties occur"""
    qualified = cut = ties = 0
    for s in range(scenes.NUM_FUZZ):
        scene = scenes.fuzz(s)
        got = _run(scene)
        assert got["overflow_lines"] == 0
        qualified += got["num_qualified"] > 0
        cut += got["num_qualified"] > len(got["sets"])
        counts = [x["num_aligned"] for x in got["sets"]]
        ties += len(set(counts)) < len(counts)
    assert qualified >= 10 and ties >= 3, (qualified, cut, ties)
