"""tests/local_bundle_reference.py (FindLocalBundle in plain Python, the yardstick of the host replay test and of the GPU test) against expectations
worked out by hand from src/sfm/incremental_mapper.cc:993-1160 and written into tests/local_bundle_scenes.py: the bundle in the reference's order, the
last threshold level reached, the images the fill-up took, the number of lazily computed angles and NumPoints3D.  Every scene keeps every compared
angle at least 1e-6 (relative) away from its threshold - in fact 8 % - so that no decision can hang on the last bits of an angle."""
import math

import pytest

import local_bundle_reference as ref
import local_bundle_scenes as scenes


@pytest.mark.parametrize("scene", scenes.SCENES, ids=lambda f: f.__name__)
def test_reference_gives_the_hand_written_result(scene):
    w, want = scene()
    got = ref.find_local_bundle(w.rec, ref.Options(**want["options"]), want["image"])
    assert got["bundle"] == want["bundle"]
    assert (got["level"], got["filled"], got["lazy"], got["num_points3D"]) == (want["level"], want["filled"], want["lazy"], want["num_points3D"])
    assert got["margin"] > 1e-6
    assert sum(1 for a in got["tri_angle"] if a >= 0) == want["lazy"]
    assert [c for _, c in got["overlap"]] == sorted((c for _, c in got["overlap"]), reverse=True)


def test_the_three_layouts_do_not_take_the_top_of_the_overlap_list():
    for scene in (scenes.relax, scenes.fill, scenes.strict):
        w, want = scene()
        got = ref.find_local_bundle(w.rec, ref.Options(**want["options"]), want["image"])
        top = [iid for iid, _ in got["overlap"]][: len(got["bundle"])]
        assert got["bundle"] != top and got["margin"] >= 0.08


def test_percentile_index_rounds_halves_away_from_zero():
    assert [ref.percentile_index(n) for n in (1, 2, 3, 7, 64, 65, 300)] == [0, 1, 2, 5, 47, 48, 224]
    assert round(4.5) == 4 and ref.percentile_index(7) == 5


def test_nan_sorts_above_every_number():
    nan = float("nan")
    assert ref.percentile75([nan, 0.4, 0.2, 0.3]) == 0.4
    assert math.isnan(ref.percentile75([nan, 0.3, nan, nan]))
