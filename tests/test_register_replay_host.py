"""csrc/register_replay.hpp - the sequential half of pp_tracks_find_next_images / pp_tracks_estimate_image_pose / pp_tracks_register_image - without a
device and under the sanitizers: the header is std only, tests/register_replay_host_driver.cpp compiles with g++ -fsanitize=address,undefined and
is fed the counts, RANSAC reports and correspondence lists of the scenes of register_image_scenes.py.  Its decisions must equal the transcription's
(tests/register_image_reference.py; test_register_image_reference.py checks that one against the hand-written expectations): the ranked list with
its buckets and ties, every gate, the quaternion bit for bit, the commit rule and its validation.  A sanitizer report ends the driver with a
non-zero status, which fails the test."""
import os
import subprocess

import numpy as np
import pytest

import register_image_reference as ref
import register_image_scenes as scenes
from privacy_preserving_sfm_amd import synthetic
from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("register_replay") / "register_replay_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "register_replay_host_driver.cpp")])
    return exe


def _run(exe, script):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    return [l.split() for l in out.stdout.splitlines()]


def _images(rec, graph, num_reg_trials, filtered):
    script = ["images %d" % len(rec.images)]
    for iid in sorted(rec.images):
        im = rec.images[iid]
        script.append("image %d %d %d %d %d %d" % (iid, ref.is_registered(im), ref.num_visible_points3D(rec, graph, im), ref.num_observations(graph, im),
                                                  num_reg_trials.get(iid, 0), iid in filtered))
    return script


def test_ranking_equals_the_transcription(driver):
    w, want = scenes.ranking()
    assert sorted(w.rec.images) == list(range(len(w.rec.images)))
    m = ref.Mapper(w.rec, w.graph)
    m.num_reg_trials, m.filtered_images = dict(want["num_reg_trials"]), set(want["filtered"])
    o = want["options"]
    script = _images(w.rec, w.graph, m.num_reg_trials, m.filtered_images)
    script += ["rank %d %d 0 1" % (o["abs_pose_min_num_inliers"], o["max_reg_trials"]), "rank %d %d 1 1" % (o["abs_pose_min_num_inliers"], o["max_reg_trials"]),
               "rank %d %d 1 0" % (o["abs_pose_min_num_inliers"], o["max_reg_trials"]), "rank 1 1 0 1", "rank 7 3 1 1"]
    out = _run(driver, script)
    ranked = [[int(x) for x in r[1:]] for r in out if r[0] == "ranked"]
    buckets = [(int(r[1]), int(r[2])) for r in out if r[0] == "buckets"]
    assert ranked[0] == want["num"] == m.find_next_images(ref.Options(image_selection_method=0, **o))
    assert ranked[1] == want["ratio"] == m.find_next_images(ref.Options(image_selection_method=1, **o))
    assert buckets[0] == buckets[1] == (4, 9)
    fresh = ref.Mapper(w.rec, w.graph)      # no trials, nothing filtered: one bucket
    assert ranked[2] == fresh.find_next_images(ref.Options(image_selection_method=1, **o)) and buckets[2] == (len(ranked[2]), 9)
    assert ranked[3] == m.find_next_images(ref.Options(image_selection_method=0, abs_pose_min_num_inliers=1, max_reg_trials=1))
    assert ranked[4] == m.find_next_images(ref.Options(image_selection_method=1, abs_pose_min_num_inliers=7, max_reg_trials=3)) == [6, 9]


def test_an_image_without_observations_never_ranks(driver):
    """observed == 0 (the ratio is 0 / 0): visible is 0 too and fails `visible >= abs_pose_min_num_inliers > 0` before the rank is taken"""
    out = _run(driver, ["images 3", "image 0 1 0 0 0 0", "image 1 0 0 0 0 0", "image 2 0 1 1 0 0", "rank 1 3 1 1"])
    assert ["ranked", "2"] in out and ["buckets", "1", "2"] in out


def test_gates(driver):
    cases = [(29, 100, 30), (30, 29, 30), (30, 30, 30), (5, 5, 4), (6, 6, 4), (0, 0, 1)]
    out = _run(driver, ["gates %d %d %d" % c for c in cases])
    want = [[str(int(v >= m)), str(int(not (n < m or n < 6)))] for v, n, m in cases]
    assert [r[1:] for r in out] == want


def _pose_line(min_inliers, num_inliers, model, mask, aligned=None):
    toks = ["pose", str(min_inliers), str(num_inliers), str(len(mask)), "0" if aligned is None else "1"]
    toks += ["nan" if x != x else float(x).hex() for x in np.asarray(model, dtype=np.float64).reshape(12)]
    toks += [str(int(x)) for x in mask]
    if aligned is not None:
        toks += [str(int(x)) for x in aligned]
    return " ".join(toks)


def _transcription_pose(min_inliers, num_inliers, model, mask, aligned):
    lines = [scenes.FeatureLine(np.array([1.0, 0.0, 0.0]), bool(a)) for a in (aligned if aligned is not None else [0] * len(mask))]
    o = ref.RANSACOptions(); o.max_error = 1.0
    site, q, t, n, _ = ref.estimate_absolute_pose_from_lines(lambda *a: (num_inliers, mask, model), o, lines, [None] * len(mask))
    if site == ref.OK and n < min_inliers:
        site = ref.FEW_INLIERS
    return site, q, t


def test_pose_gates_and_the_quaternion_bit_for_bit(driver):
    rng = np.random.default_rng(3)
    cases = []
    for k in range(40):      # rotations of every kind: both branches of the conversion, every choice of the largest diagonal entry
        q = rng.normal(size=4)
        if k % 4 == 1:
            q[0] = 1e-3 * rng.normal()      # a rotation by about pi: the trace is negative
        q /= np.linalg.norm(q)
        model = np.concatenate([synthetic.quat_to_rot(q), rng.normal(size=(3, 1))], axis=1)
        n = 50
        mask = (rng.uniform(size=n) < 0.8).astype(int)
        cases.append((30, int(mask.sum()), model, mask, None if k % 2 else (rng.uniform(size=n) < 0.3).astype(int)))
    model = cases[0][2]
    ones = np.ones(50, dtype=int)
    al46, al45 = np.array([1] * 46 + [0] * 4), np.array([1] * 45 + [0] * 5)
    nan_model = model.copy(); nan_model[2, 3] = np.nan
    nan_rot = model.copy(); nan_rot[0, 0] = np.nan
    cases += [(30, 0, model, np.zeros(50, dtype=int), None), (30, 50, model, ones, al46), (30, 50, model, ones, al45), (30, 50, nan_model, ones, None),
              (30, 50, nan_rot, ones, None), (30, 29, model, np.array([1] * 29 + [0] * 21), None), (30, 30, model, np.array([1] * 30 + [0] * 20), None),
              (10, 10, model, np.array([1] * 10), np.array([1] * 9 + [0]))]      # 9 > 10 * 0.9 = 9.0 is false
    out = _run(driver, [_pose_line(*c) for c in cases])
    sites = []
    for c, r in zip(cases, out):
        site, q, t = _transcription_pose(*c)
        sites.append(site)
        assert int(r[1]) == site, (r, site)
        if site in (ref.OK, ref.FEW_INLIERS):
            got = np.array([float.fromhex(x) for x in r[3:10]])
            assert np.array_equal(got, np.concatenate([q, t]))      # the same doubles
    assert sites[40:] == [ref.NO_INLIERS, ref.ALIGNED, ref.OK, ref.NAN, ref.NAN, ref.FEW_INLIERS, ref.OK, ref.OK]
    assert set(sites[:40]) == {ref.OK}


def _state_script(rec, graph):
    flat, point_ids, line_ref = IncrementalTriangulator(graph, rec).flatten()
    assert point_ids == list(range(len(point_ids))) and sorted(rec.images) == list(range(len(rec.images)))
    script = ["images %d" % len(rec.images)] + ["image %d %d 0 0 0 0" % (i, ref.is_registered(rec.images[i])) for i in sorted(rec.images)]
    script.append("state %d %d" % (len(line_ref), len(point_ids)))
    # tracks in track order: feed the lines point by point, then the free ones
    order = [line_ref.index(el) for p in point_ids for el in rec.points3D[p].track]
    order += [l for l in range(len(line_ref)) if flat["line_point"][l] < 0]
    script += ["line %d %d %d" % (l, flat["line_image"][l], flat["line_point"][l]) for l in order]
    return script, flat, line_ref


def _commit_line(image, pose, rows, with_mask=1):
    return "commit %d %d %s %d %s" % (image, with_mask, " ".join(float(x).hex() if x == x else "nan" for x in pose), len(rows),
                                      " ".join("%d %d %d" % r for r in rows))


@pytest.mark.parametrize("scene", scenes.COMMIT_SCENES, ids=lambda f: f.__name__)
def test_commit_rule_equals_the_transcription(driver, scene):
    w, want = scene()
    script, flat, line_ref = _state_script(w.rec, w.graph)
    q = want["image"]
    rows = [(line_ref.index((q, idx)), pid, m) for (idx, pid), m in zip(want["tri_corrs"], want["inlier_mask"])]
    out = _run(driver, script + [_commit_line(q, scenes.QUERY_POSE, rows)])
    events = ref.Mapper(w.rec, w.graph).commit(q, want["tri_corrs"], want["inlier_mask"])
    assert events == want["events"]
    assert ["check", "0"] in out
    assert [(int(r[1]), line_ref[int(r[2])]) for r in out if r[0] == "event"] == events
    assert ["added", str(len(events))] in out
    after = IncrementalTriangulator(w.graph, w.rec).flatten()[0]      # the transcription's updated reconstruction
    assert [int(x) for x in [r for r in out if r[0] == "state"][0][1:]] == after["line_point"].tolist()
    tracks = {int(r[1]): [int(x) for x in r[2:]] for r in out if r[0] == "track"}
    for p in range(len(after["points"])):
        assert tracks[p] == after["track_line"][after["track_start"][p]:after["track_start"][p + 1]].tolist()
    assert [int(x) for x in [r for r in out if r[0] == "registered"][0][1:]] == after["image_registered"].tolist()


def test_commit_without_a_mask_takes_every_correspondence(driver):
    w, want = scenes.commit_first_inlier_wins()
    script, flat, line_ref = _state_script(w.rec, w.graph)
    q = want["image"]
    rows = [(line_ref.index((q, idx)), pid, 0) for (idx, pid) in want["tri_corrs"]]
    out = _run(driver, script + [_commit_line(q, scenes.QUERY_POSE, rows, with_mask=0)])
    assert [(int(r[1]), line_ref[int(r[2])]) for r in out if r[0] == "event"] == [(want["tri_corrs"][0][1], (q, 0)), (want["tri_corrs"][2][1], (q, 1))]


def test_commit_validation(driver):
    """each invalid argument gives its code and leaves the state alone (the driver commits only after code 0, as the library does)"""
    w, want = scenes.commit_two_lines_one_point()
    w.rec.points3D[len(w.rec.points3D)] = type(w.rec.points3D[0])(np.array([0.0, 0.0, 5.0]))      # a point without a track: deleted
    script, flat, line_ref = _state_script(w.rec, w.graph)
    q = want["image"]
    dead = len(flat["points"]) - 1
    good = [(line_ref.index((q, idx)), pid, m) for (idx, pid), m in zip(want["tri_corrs"], want["inlier_mask"])]
    other = line_ref.index((scenes.HOST_A, 0))
    nan_pose = scenes.QUERY_POSE.copy(); nan_pose[5] = np.nan
    inf_pose = scenes.QUERY_POSE.copy(); inf_pose[0] = np.inf
    L, P = len(line_ref), len(flat["points"])
    bad = [(len(w.rec.images), scenes.QUERY_POSE, good, 1), (-1, scenes.QUERY_POSE, good, 1), (scenes.HOST_A, scenes.QUERY_POSE, [], 1),
           (q, scenes.QUERY_POSE, good + [(other, 0, 1)], 2), (q, scenes.QUERY_POSE, [(L, 0, 1)], 2), (q, scenes.QUERY_POSE, [(-1, 0, 1)], 2),
           (q, scenes.QUERY_POSE, [(good[0][0], P, 1)], 3), (q, scenes.QUERY_POSE, [(good[0][0], -1, 1)], 3), (q, scenes.QUERY_POSE, [(good[0][0], dead, 0)], 3),
           (q, nan_pose, good, 4), (q, inf_pose, good, 4)]
    out = _run(driver, script + [_commit_line(im, pose, rows) for im, pose, rows, _ in bad] + [_commit_line(q, scenes.QUERY_POSE, good)])
    checks = [int(r[1]) for r in out if r[0] == "check"]
    assert checks == [code for _, _, _, code in bad] + [0]
    assert [(int(r[1]), line_ref[int(r[2])]) for r in out if r[0] == "event"] == want["events"]      # the state was as at the start
