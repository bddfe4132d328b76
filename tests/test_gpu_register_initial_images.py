"""IncrementalMapper.RegisterInitialLineImages on the device mirrors, on the scene of tests/initial_images_scene.py: a reconstruction from ZERO registered
images and no points to four registered images with points, and on from there with the per-image loop - everything on one tracks handle.

The image sets tried, and their order, must be the ones the plain-Python reference of the search ranks (tests/initial_sets_reference.py).  The four poses
are compared with the truth in the gauge of initialize_reconstruction (relative to the set's first image, translations scaled by |t_1|) within 1e-6: the
bound tests/test_gpu_host_mirrors.py::test_initialize_reconstruction holds this solver to on exact lines, itself the bound of the reference's own test."""
import numpy as np
import pytest

import initial_images_scene as iis
import initial_sets_reference as ref
from privacy_preserving_sfm_amd.bundle_adjustment import IncrementalMapperOptions, _quat_to_rot
from privacy_preserving_sfm_amd.incremental_mapper import IncrementalMapper
from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator

pytestmark = pytest.mark.gpu

POSE_TOLERANCE = 1e-6


def _options():
    o = IncrementalMapperOptions()
    o.abs_pose_min_num_inliers = iis.MIN_NUM_INLIERS
    o.print_summary = False
    return o


def _snapshot(rec):
    return (sorted(rec.RegImageIds()), {i: (im.qvec.copy(), im.tvec.copy()) for i, im in rec.images.items()},
            {p: (pt.xyz.copy(), list(pt.track)) for p, pt in rec.points3D.items()})


def _same(a, b):
    return (a[0] == b[0] and all(np.array_equal(a[1][i][0], b[1][i][0]) and np.array_equal(a[1][i][1], b[1][i][1]) for i in a[1]) and
            sorted(a[2]) == sorted(b[2]) and all(np.array_equal(a[2][p][0], b[2][p][0]) and a[2][p][1] == b[2][p][1] for p in a[2]))


def _initialise(in_session):
    rec, graph, info = iis.make_world()
    tri = IncrementalTriangulator(graph, rec)
    mapper = IncrementalMapper(graph, rec, tri)
    options = _options()
    log = {}

    def run():
        log["ok"] = mapper.RegisterInitialLineImages(options)
        log["after_init"] = _snapshot(rec)
        log["ranked"] = mapper.FindNextImages(options)
        log["next"] = log["ranked"][0] if log["ranked"] else None
        log["registered_next"] = bool(log["ranked"]) and mapper.RegisterNextImage(options, log["next"])
        log["points_before"] = len(rec.points3D)
        log["num_tris"] = tri.TriangulateImage(tri.Options(), log["next"]) if log["registered_next"] else 0
        log["end"] = _snapshot(rec)

    if in_session:
        with tri.Session():
            run()
    else:
        run()
    return rec, info, mapper, log


@pytest.fixture(scope="module")
def outside():
    return _initialise(False)


@pytest.fixture(scope="module")
def reference_sets():
    rec, graph, _ = iis.make_world()
    scene, line_ref = iis.flat_scene(rec, graph)
    return ref.find_initial_sets(scene, **scene["options"]), line_ref


def test_four_images_are_registered_from_zero(outside, reference_sets):
    rec, info, mapper, log = outside
    want, _ = reference_sets
    init = mapper.last_init
    print("tried", [(s["image_ids"], s["num_aligned"], s["num_random"], s["success"], "%.3f" % s["inlier_ratio"]) for s in init["sets"]], "chosen", init["chosen"])
    print("device report: candidates", init["report"].num_candidates, "device_ms %.3f total_ms %.3f" % (init["report"].device_ms, init["report"].total_ms))
    assert log["ok"] is True
    reg, _, points = log["after_init"]
    assert len(reg) == 4 and reg == sorted(init["chosen"])
    assert init["check_image_ids"] == list(range(iis.NUM_IMAGES))
    # the sets tried are the reference's, in its order, with its counts
    assert [(s["image_ids"], s["num_aligned"], s["num_random"]) for s in init["sets"]] == [(s["images"], s["num_aligned"], s["num_random"]) for s in want["sets"]]
    assert init["chosen"] in [s["images"] for s in want["sets"]]
    assert (init["report"].num_candidates, init["report"].num_qualified) == (want["num_candidates"], want["num_qualified"])
    tried = {tuple(s["image_ids"]): s for s in init["sets"]}
    best = max((s for s in init["sets"] if s["success"]), key=lambda s: s["inlier_ratio"])
    assert tried[tuple(init["chosen"])]["inlier_ratio"] == best["inlier_ratio"]
    assert [rec.images[i].reg_index for i in sorted(init["chosen"])] == [0, 1, 2, 3]      # registered in ascending id
    assert mapper.num_reg_images_per_camera_ == {0: 4 + int(log["registered_next"])}
    assert len(points) >= 1


def test_the_poses_equal_the_truth_in_the_solvers_gauge(outside):
    rec, info, mapper, log = outside
    ids = sorted(mapper.last_init["chosen"])
    _, poses, _ = log["after_init"]
    R = {i: _quat_to_rot(poses[i][0]) for i in ids}
    t = {i: poses[i][1] for i in ids}
    got, want = iis.relative_poses(R, t, ids), iis.relative_poses(info["R"], info["t"], ids)
    errors = [float(np.linalg.norm(got[k] - want[k])) for k in range(4)]
    print("pose errors (Frobenius, relative to image %d, |t_1| = 1):" % ids[0], ["%.3e" % e for e in errors])
    assert max(errors) < POSE_TOLERANCE


def test_every_track_joins_the_lines_of_one_true_point(outside):
    rec, info, mapper, log = outside
    _, _, points = log["after_init"]
    for p, (_, track) in points.items():
        assert len({info["line_point"][el] for el in track}) == 1, p
        assert len(track) >= 2 and {i for i, _ in track} <= set(mapper.last_init["chosen"])


def test_the_mapper_goes_on_from_there(outside):
    rec, info, mapper, log = outside
    reg = log["after_init"][0]
    assert sorted(log["ranked"]) == [i for i in range(iis.NUM_IMAGES) if i not in reg] and len(log["ranked"]) == 3
    assert log["next"] == 4 and log["registered_next"] is True
    assert log["num_tris"] > 0 and len(log["end"][2]) > log["points_before"]      # the points seen by images 3-6 had one registered view until now
    assert log["end"][0] == sorted(reg + [log["next"]])
    for _, (_, track) in log["end"][2].items():
        assert len({info["line_point"][el] for el in track}) == 1


def test_inside_a_session_everything_is_identical(outside):
    _, _, mapper_a, a = outside
    _, _, mapper_b, b = _initialise(True)
    assert a["ok"] == b["ok"] and a["ranked"] == b["ranked"] and a["registered_next"] == b["registered_next"] and a["num_tris"] == b["num_tris"]
    assert mapper_a.last_init["sets"] == mapper_b.last_init["sets"] and mapper_a.last_init["chosen"] == mapper_b.last_init["chosen"]
    assert _same(a["after_init"], b["after_init"]) and _same(a["end"], b["end"])


def test_too_few_aligned_tracks_return_false_and_change_nothing():
    rec, graph, _ = iis.make_world(few_aligned=12)
    mapper = IncrementalMapper(graph, rec, IncrementalTriangulator(graph, rec))
    before = _snapshot(rec)
    assert mapper.RegisterInitialLineImages(_options()) is False
    assert _same(before, _snapshot(rec)) and rec.RegImageIds() == [] and mapper.num_reg_images_per_camera_ == {}
    init = mapper.last_init
    assert init["sets"] == [] and init["chosen"] is None and init["report"].num_qualified == 0 and init["report"].num_aligned_tracks > 0


def test_more_inliers_asked_for_than_there_are_tracks_returns_false():
    """init_min_num_inliers above every set's track count: no solve can pass it - the solver's own gate, and behind it the gate of :538"""
    rec, graph, _ = iis.make_world()
    mapper = IncrementalMapper(graph, rec, IncrementalTriangulator(graph, rec))
    options = _options()
    options.init_min_num_inliers = 10 * iis.NUM_POINTS
    before = _snapshot(rec)
    assert mapper.RegisterInitialLineImages(options) is False
    assert _same(before, _snapshot(rec)) and mapper.last_init["chosen"] is None and len(mapper.last_init["sets"]) >= 3
