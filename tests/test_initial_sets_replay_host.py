"""csrc/initial_sets_replay.hpp - the sequential end of pp_tracks_find_initial_sets: the qualifying rule, the ranking with its pinned tie order, the
truncation - without a device and under the sanitizers: the header is std only, tests/initial_sets_replay_host_driver.cpp compiles with
g++ -fsanitize=address,undefined as a stand-alone program and is fed, for every scene of initial_sets_scenes.py, the per-set counts the plain-Python
reference gives (what the device's run-length encoding delivers).  The ranked sets must equal the reference's.  The driver's --time mode (the std::map of
std::sets search that DESIGN.md's measurement compares the device with) is held to the same reference here.  A sanitizer report ends the driver with a
non-zero status, which fails the test."""
import os
import subprocess

import pytest

import initial_sets_reference as ref
import initial_sets_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("initial_sets_replay") / "initial_sets_replay_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "initial_sets_replay_host_driver.cpp")])
    return exe


def _run(exe, script, args=()):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe] + list(args), input="\n".join(script) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    return [l.split() for l in out.stdout.splitlines()]


def _ints(a):
    return " ".join(str(int(x)) for x in a)


def runs_of(got):
    """the (image set, class, count) runs in ascending key order: per set the aligned run, then the random one"""
    runs = []
    for images in sorted(got["counts"]):
        a, r = got["counts"][images]
        runs += [(images, 0, a)] if a else []
        runs += [(images, 1, r)] if r else []
    return runs


def graph_script(scene):
    """the --time mode's input"""
    start = [0]
    for c in scene["corr"]:
        start.append(start[-1] + len(c))
    o = scene["options"]
    subset = "subset -1" if scene["subset"] is None else "subset %d %s" % (len(scene["subset"]), _ints(scene["subset"]))
    return ["graph %d %d %d" % (scene["num_images"], len(scene["line_image"]), start[-1]), "line_image " + _ints(scene["line_image"]),
            "aligned " + _ints(scene["line_aligned"]), "corr_start " + _ints(start), "corr_line " + _ints(n for c in scene["corr"] for n in c), subset,
            "check %d %s" % (len(scene["check_images"]), _ints(scene["check_images"])),
            "options %d %d %d" % (o["min_num_aligned_tracks"], o["min_num_random_tracks"], o["max_num_sets"])]


def _sets(out):
    return [[int(x) for x in r[1:7]] for r in out if r[0] == "set"]


@pytest.mark.parametrize("name,build", scenes.all_scenes(), ids=[n for n, _ in scenes.all_scenes()])
def test_replay_equals_the_reference(driver, name, build):
    scene = build()
    o = scene["options"]
    got = ref.find_initial_sets(scene, **o)
    runs = runs_of(got)
    script = ["replay %d %d %d %d" % (o["min_num_aligned_tracks"], o["min_num_random_tracks"], o["max_num_sets"], len(runs))]
    script += ["%s %d %d" % (_ints(images), cls, n) for images, cls, n in runs]
    out = _run(driver, script)
    assert [[int(x) for x in r[1:]] for r in out if r[0] == "unpacked"] == [list(images) + [cls] for images, cls, _ in runs]
    totals = [int(x) for x in [r for r in out if r[0] == "totals"][0][1:]]
    assert totals == [got["num_aligned_tracks"], got["num_random_tracks"], got["num_aligned_sets"], got["num_random_sets"], got["num_qualified"]]
    assert _sets(out) == [s["images"] + [s["num_aligned"], s["num_random"]] for s in got["sets"]]
    for r in (r for r in out if r[0] == "set"):      # the runs the device downloads the tracks from
        assert runs[int(r[7])] == (tuple(int(x) for x in r[1:5]), 0, int(r[5])) and runs[int(r[8])] == (tuple(int(x) for x in r[1:5]), 1, int(r[6]))


def test_the_key_holds_the_largest_image_index(driver):
    top = (1 << 15) - 1
    out = _run(driver, ["replay 1 1 10 4", "0 1 2 %d 0 5" % top, "0 1 2 %d 1 7" % top, "%d %d %d %d 0 9" % (top - 3, top - 2, top - 1, top),
                        "%d %d %d %d 1 1" % (top - 3, top - 2, top - 1, top)])
    assert _sets(out) == [[top - 3, top - 2, top - 1, top, 9, 1], [0, 1, 2, top, 5, 7]]


def test_zero_sets_asked_for_and_no_runs(driver):
    out = _run(driver, ["replay 1 1 0 2", "0 1 2 3 0 5", "0 1 2 3 1 5", "replay 1 1 10 0"])
    assert [r[1:] for r in out if r[0] == "totals"] == [["5", "5", "1", "1", "1"], ["0", "0", "0", "0", "0"]] and _sets(out) == []


@pytest.mark.parametrize("name,build", scenes.all_scenes(), ids=[n for n, _ in scenes.all_scenes()])
def test_the_timing_partner_computes_the_reference(driver, name, build):
    scene = build()
    got = ref.find_initial_sets(scene, **scene["options"])
    out = _run(driver, graph_script(scene), args=["--time"])
    totals = [int(x) for x in [r for r in out if r[0] == "totals"][0][1:]]
    assert totals == [got["num_candidates"], got["num_aligned_tracks"], got["num_random_tracks"], got["num_aligned_sets"], got["num_random_sets"], got["num_qualified"]]
    assert _sets(out) == [s["images"] + [s["num_aligned"], s["num_random"]] for s in got["sets"]]
