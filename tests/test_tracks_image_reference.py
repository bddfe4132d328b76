"""The oracle of TriangulateImage / CompleteImage (tests/tracks_image_reference.py) alone, on the hand-built scenes of tests/tracks_image_scenes.py,
against results worked out by hand (each scene's docstring says why).  No device."""
import numpy as np
import pytest

import tracks_image_reference as tir
import tracks_image_scenes as scenes
from privacy_preserving_sfm_amd.incremental_triangulator import CorrespondenceGraph


def run_oracle(w, want):
    oracle = tir.ImageOracle(w.graph, w.rec)
    oo = tir.Options(max_transitivity=want.get("transitivity", 1), **scenes.TIGHT)
    n = 0
    for op in want["ops"]:
        n += oracle.TriangulateImage(oo, want["image"]) if op == "t" else oracle.CompleteImage(oo, want["image"])
    return oracle, n


@pytest.mark.parametrize("scene", scenes.HAND_BUILT, ids=lambda f: f.__name__)
def test_hand_built_scene(scene, oracle):
    w, want = scene()
    before = tir.tr.state(w.rec)
    o, n = run_oracle(w, want)
    assert o.events == want["events"]
    assert n == want["num_changed"]
    assert o.arbitrary == 0 and o.margin > 1e-6
    if not want["events"]:
        assert tir.tr.state(w.rec) == before
    for pid in o.created:      # the scenes are exact: a created point lies on one of the three places
        assert min(np.abs(w.rec.points3D[pid].xyz - p).max() for p in (scenes.X, scenes.Y, scenes.Z)) < 1e-9


def test_find_transitive_correspondences_order(oracle):
    g = CorrespondenceGraph()
    for a, b in [(0, 1), (0, 2), (1, 3), (2, 4), (3, 0), (4, 5)]:
        g.AddCorrespondence(a, 0, b, 0)
    el = lambda ids: [(i, 0) for i in ids]
    for f in (lambda *a: tir.find_transitive_correspondences(g, *a), g.FindTransitiveCorrespondences):
        assert f(0, 0, 1) == el([1, 2])                      # the direct list as it is
        assert f(0, 0, 2) == el([4, 1, 2, 3])                # [0, 1, 2, 3, 4]: the query overwritten by the last element
        assert f(0, 0, 3) == el([5, 1, 2, 3, 4])             # 3 -> 0 is seen already; 4 -> 5 on the third level
        assert f(5, 0, 2) == []                              # no correspondences at all
        assert f(4, 0, 2) == el([5])                         # [4, 5]: the query overwritten by 5, the tail popped

def test_two_view_observation(oracle):
    g = CorrespondenceGraph()
    g.AddCorrespondence(0, 0, 1, 0); g.AddCorrespondence(1, 0, 0, 0)
    g.AddCorrespondence(2, 0, 3, 0); g.AddCorrespondence(3, 0, 2, 0); g.AddCorrespondence(3, 0, 4, 0)
    for f in (lambda *a: tir.is_two_view_observation(g, *a), g.IsTwoViewObservation):
        assert f(0, 0) and f(1, 0) and not f(2, 0) and not f(3, 0) and not f(4, 0)


def test_complete_image_carries_min_num_trials(oracle):
    """a set of more than 15 observations runs with the min_num_trials the last shorter set left behind (one options object over the loop)"""
    w = scenes.World()
    r0 = w.add_line(0, scenes.Y)
    for c in (5, 6, 7):
        w.link(r0, w.add_line(c, scenes.Y))
    r1 = w.add_line(0, scenes.X)
    for i in range(20):
        w.link(r1, w.add_line(1 + (i % 11), scenes.X))
    seen = []
    o = tir.ImageOracle(w.graph, w.rec)
    est = o._estimate
    o._estimate = lambda options, corrs, rt, me, mt: (seen.append((len(corrs), mt)), est(options, corrs, rt, me, mt))[1]
    assert o.CompleteImage(tir.Options(), 0) == 4 + 21
    assert seen == [(4, 6), (21, 6)]
