"""csrc/local_bundle_replay.hpp - the sequential half of pp_tracks_find_local_bundle - without a device and under the sanitizers: the header is std only,
tests/local_bundle_replay_host_driver.cpp compiles with g++ -fsanitize=address,undefined and is fed the counts and the per-point angles of every scene
of local_bundle_scenes.py, computed by the plain-Python reference's own functions.  Its decisions must equal the reference's (and with them the
hand-written expectations that test_local_bundle_reference.py checks): the sorted list, the lazily computed percentiles bit for bit, the bundle in order,
the level, the fill-up.  A sanitizer report ends the driver with a non-zero status, which fails the test."""
import os
import subprocess

import numpy as np
import pytest

import local_bundle_reference as ref
import local_bundle_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("local_bundle_replay") / "local_bundle_replay_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "local_bundle_replay_host_driver.cpp")])
    return exe


def _run(exe, script):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    return [l.split() for l in out.stdout.splitlines()]


def _script(rec, image_id, options):
    """counts and per-point angles of every other image, as FindLocalBundle's first loop and CalculateTriangulationAngles give them"""
    image = rec.images[image_id]
    ids = sorted(rec.images)
    point_ids = [l.Point3DId() for l in image.lines if l.HasPoint3D()]
    points = [rec.points3D[p].xyz for p in point_ids]
    center = ref.projection_center(image)
    script = ["images %d" % (max(ids) + 1)]
    for iid in ids:
        if iid == image_id:
            continue
        n = sum(1 for p in point_ids for (i2, _) in rec.points3D[p].track if i2 == iid)
        script.append("count %d %d" % (iid, n))
        if points:
            a = ref.triangulation_angles(center, ref.projection_center(rec.images[iid]), points)
            script.append("angles %d %s ;" % (iid, " ".join("nan" if x != x else float(x).hex() for x in a)))
    script.append("find %d %d %r" % (len(point_ids), options.local_ba_num_images, float(options.local_ba_min_tri_angle)))
    return script


def _compare(out, want):
    overlap = [r for r in out if r[0] == "overlap"]
    assert [(int(r[1]), int(r[2])) for r in overlap] == want["overlap"]
    got = [float(r[3]) for r in overlap]
    for g, w in zip(got, want["tri_angle"]):
        assert g == w or (g != g and w != w), (g, w)      # the same element of the same doubles
    assert [int(x) for r in out if r[0] == "bundle" for x in r[1:]] == want["bundle"]
    res = [r for r in out if r[0] == "result"][0]
    assert (int(res[2]), int(res[4]), int(res[6])) == (want["level"], want["filled"], want["lazy"])
    assert not [r for r in out if r[0] == "missing"]
    asked = [int(r[1]) for r in out if r[0] == "asked"]
    assert len(asked) == len(set(asked)) == want["lazy"]      # lazy: every angle once


@pytest.mark.parametrize("scene", scenes.SCENES, ids=lambda f: f.__name__)
def test_replay_equals_the_reference(driver, scene):
    w, expect = scene()
    options = ref.Options(**expect["options"])
    want = ref.find_local_bundle(w.rec, options, expect["image"])
    assert want["bundle"] == expect["bundle"]
    _compare(_run(driver, _script(w.rec, expect["image"], options)), want)


def test_a_nan_angle_sorts_above_every_number_and_a_nan_percentile_fails(driver):
    """image 1: four angles, one NaN: the percentile index 2 of (0.2, 0.3, 0.4, NaN) is 0.4 rad - passes; image 2: three NaN of four: the percentile is NaN,
    fails every level and the image comes in through the fill-up; image 3 exists so that there is no early return"""
    out = _run(driver, ["images 4", "count 1 4", "count 2 3", "count 3 2", "angles 1 nan 0.4 0.2 0.3 ;", "angles 2 nan 0.3 nan nan ;", "angles 3 0.001 0.001 0.001 0.001 ;",
                        "find 4 3 6.0"])
    assert [r for r in out if r[0] == "bundle"] == [["bundle", "1", "2"]]
    angles = [float(r[3]) for r in out if r[0] == "overlap"]
    assert angles[0] == 0.4 and angles[1] != angles[1]
    assert ["result", "level", "7", "filled", "1", "used", "3", "eff", "2"] in out
    assert [r[1] for r in out if r[0] == "asked"] == ["1", "2", "3"]


def test_percentile_index_is_round_half_away_from_zero(driver):
    """N = 7: 0.75 * 6 = 4.5 -> 5.  Seven angles 0.01 .. 0.07 rad and a threshold between the fifth and the sixth (6 deg / 1.0 = 0.1047 is above both, so
    use 3 deg = 0.0524 rad): index 5 (0.06) passes level 0, index 4 (0.05) would not"""
    out = _run(driver, ["images 3", "count 1 7", "count 2 6", "angles 1 0.03 0.07 0.01 0.05 0.02 0.06 0.04 ;", "angles 2 0.001 0.001 0.001 0.001 0.001 0.001 0.001 ;",
                        "find 7 2 3.0"])
    assert [r for r in out if r[0] == "bundle"] == [["bundle", "1"]]
    assert ["result", "level", "0", "filled", "0", "used", "1", "eff", "1"] in out
    assert float([r[3] for r in out if r[0] == "overlap"][0]) == 0.06
    assert np.floor(0.75 * 6 + 0.5) == 5
