"""IterativeLocalRefinement (reference src/controllers/incremental_mapper.cc:72-100 over src/sfm/incremental_mapper.cc:781-891, 993-1160) through the
Python mirror on the device against the same loop run with the CPU oracles (tests/local_refinement_oracle.py), on one small noisy scene:
make_completion_scene(8, 60, 6) with 0.5 px line noise, 5 % outlier observations and float32-stored lines; the image is the last one registered and its
TriangulateImage runs first, so that GetModifiedPoints3D is not empty.

The seed was picked on the CPU with the oracle alone (tests/local_refinement_oracle.py SCENE: margin 2.1e-2 over completion, merge, the image's
RANSACs, both filters and the local bundle's angles; no RANSAC with an arbitrary winner); the test asserts the margin above 1e-6.
Equal: the bundle, the variable points, the counts of every round's report, the deleted observations and points, the round count.  Poses and points:
1e-5 relative in the array norm, the bound of tests/test_gpu_global_refinement.py for device against oracle (`_rel` there)."""
import numpy as np
import pytest

import local_refinement_oracle as lro
import refinement_oracle
from privacy_preserving_sfm_amd import device
from privacy_preserving_sfm_amd.bundle_adjustment import AdjustLocalBundle, FindLocalBundle, IncrementalMapperOptions, IterativeLocalRefinement
from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _options():
    o = IncrementalMapperOptions()
    o.print_summary = False
    return o


def test_iterative_local_refinement_matches_the_oracle_loop(oracle):
    image = lro.SCENE["image"]
    ref_rec, ref_graph = lro.scene_world()
    ref = lro.iterative_local_refinement(ref_rec, ref_graph, image, _options())
    assert ref["margin"] > 1e-6 and ref["arbitrary"] == 0, ref["margin"]
    rec, graph = lro.scene_world()
    tri = IncrementalTriangulator(graph, rec)
    assert tri.TriangulateImage(tri.Options(), image) == ref["num_tris"] > 0
    assert len(tri.GetModifiedPoints3D()) > 0
    reports = IterativeLocalRefinement(rec, tri, image, _options())
    print("rounds: %s (oracle margin %.3e)" % ([(r.local_bundle, r.num_merged_observations, r.num_completed_observations, r.num_filtered_observations,
                                                 r.num_adjusted_observations, r.changed) for r in reports], ref["margin"]))
    assert len(reports) == len(ref["rounds"])
    for k, (r, want) in enumerate(zip(reports, ref["rounds"])):
        assert r.local_bundle == want["local_bundle"], k
        assert r.variable_point3D_ids == want["variable"], k
        assert (r.num_merged_observations, r.num_completed_observations, r.num_filtered_observations, r.num_adjusted_observations) == \
               (want["num_merged"], want["num_completed"], want["num_filtered"], want["num_adjusted"]), k
        assert r.changed == want["changed"], k
        assert r.obs_deleted == want["obs_deleted"] and r.point_deleted == want["point_deleted"], k
    assert tri.GetModifiedPoints3D() == set()      # ClearModifiedPoints3D at the end
    assert refinement_oracle.observations(rec) == refinement_oracle.observations(ref_rec)
    poses, pts, ids = refinement_oracle.parameters(rec)
    rposes, rpts, rids = refinement_oracle.parameters(ref_rec)
    assert ids == rids
    print("poses %.3e points %.3e" % (_rel(poses, rposes), _rel(pts, rpts)))
    assert _rel(poses, rposes) <= 1e-5 and _rel(pts, rpts) <= 1e-5


def test_adjust_local_bundle_opens_exactly_one_tracks_handle(oracle, monkeypatch):
    """FindLocalBundle, the update after the bundle adjustment, MergeTracks, CompleteTracks and CompleteImage share one flattening and one upload"""
    import privacy_preserving_sfm_amd.incremental_triangulator as it
    opened = []

    class Counting(device.TracksProblem):
        def __init__(self, *a, **kw):
            opened.append(1)
            super().__init__(*a, **kw)

    image = lro.SCENE["image"]
    rec, graph = lro.scene_world()
    tri = IncrementalTriangulator(graph, rec)
    tri.TriangulateImage(tri.Options(), image)
    monkeypatch.setattr(it, "TracksProblem", Counting)
    o = _options()
    bundle = FindLocalBundle(rec, tri, o, image)
    assert len(opened) == 1 and len(bundle) == 5
    del opened[:]
    report = AdjustLocalBundle(rec, tri, o, o.LocalBundleAdjustment(), tri.Options(), image, tri.GetModifiedPoints3D())
    assert len(opened) == 1
    assert report.local_bundle == bundle and report.num_adjusted_observations > 0 and report.num_completed_observations > 0
    kinds = [type(r).__name__ for r in tri.last_reports]
    assert kinds == ["LocalBundleReport", "TracksReport", "TracksReport", "TracksImageReport"]      # find, merge, complete, complete_image on that handle
