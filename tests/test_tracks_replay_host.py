"""csrc/tracks_replay.hpp - the sequential half of pp_tracks_complete / pp_tracks_merge - without a device and under the sanitizers: the header is std
only, tests/tracks_replay_host_driver.cpp compiles with g++ -fsanitize=address,undefined and is fed speculative lists and per-pair flags by hand.  Every
expectation below is worked out from the reference's Complete / Merge (src/sfm/incremental_triangulator.cc:606-765) on the scripted state, not from the
code under test.  A sanitizer report ends the driver with a non-zero status, which fails the test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tracks_replay") / "tracks_replay_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "tracks_replay_host_driver.cpp")])
    return exe


def _run(exe, script):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    return [l.split() for l in out.stdout.splitlines()]


def _sym(a, b):
    return ["corr %d %d" % (a, b), "corr %d %d" % (b, a)]


# points 0 and 1 with tracks {0, 1} and {2, 3}; free lines 4 (f1), 5 (f2), 6 (f3), 7 (f4: passes for nobody)
CONFLICT = (["images 8"] + ["line %d %d" % (i, p) for i, p in enumerate((0, 0, 1, 1, -1, -1, -1, -1))] + ["point 0 0 0", "point 1 1 1", "track 0 0 1 ;", "track 1 2 3 ;"] +
            _sym(0, 4) + _sym(2, 4) + _sym(4, 5) + _sym(3, 6) + _sym(2, 7))


def test_completion_conflict_walk(driver):
    """both points' speculative closures hold f1 and f2 (f2 through f1 only); point 1's also f3.  Point 0 takes its list as is; point 1 lost f1, so its walk is
    redone: f1 is taken, f2 is reachable through f1 only, f3 stays.  f4 is free but not in the pass set."""
    out = _run(driver, CONFLICT + ["spec 0 4 5 ;", "spec 1 4 6 5 ;", "complete 5 ;", "state"])
    assert [r for r in out if r[0] == "pair"] == [["pair", "0", "4"], ["pair", "0", "5"], ["pair", "1", "6"]]
    assert ["completed", "3", "conflicts", "1"] in out
    assert out[4] == ["lp", "0", "0", "1", "1", "0", "0", "1", "-1"]
    assert out[5][-4:] == ["0", "1", "4", "5"] and out[6][-3:] == ["2", "3", "6"]


def test_completion_without_conflict_and_with_a_subset(driver):
    """only point 1 is visited: nothing it lists was taken, so its list is appended in list order and no walk is redone"""
    out = _run(driver, CONFLICT + ["spec 0 4 5 ;", "spec 1 4 6 5 ;", "complete 5 1 ;"])
    assert out == [["pair", "1", "4"], ["pair", "1", "6"], ["pair", "1", "5"], ["completed", "3", "conflicts", "0"]]


def test_completion_conflict_respects_the_transitivity_limit(driver):
    """a chain t -> a -> b -> c behind point 1, whose line a0 point 0 takes first.  With max_transitivity 2 the redone walk reaches level 1 only:
    point 1 keeps g (level 0) and h (level 1, behind g), not i (level 2)"""
    lines = ["images 4"] + ["line 0 %d" % p for p in (0, 1, -1, -1, -1, -1)] + ["point 0 0 0", "point 1 1 1", "track 0 0 ;", "track 1 1 ;"]
    graph = _sym(0, 2) + _sym(1, 2) + _sym(1, 3) + _sym(3, 4) + _sym(4, 5)
    out = _run(driver, lines + graph + ["spec 0 2 ;", "spec 1 2 3 4 ;", "complete 2 ;"])      # (the device's list at transitivity 2 has no line 5)
    assert out == [["pair", "0", "2"], ["pair", "1", "3"], ["pair", "1", "4"], ["completed", "3", "conflicts", "1"]]
    out = _run(driver, lines + graph + ["spec 0 2 ;", "spec 1 2 3 4 5 ;", "complete 1 ;"])      # transitivity 1: level 0 only, even if the list held more
    assert out == [["pair", "0", "2"], ["pair", "1", "3"], ["completed", "2", "conflicts", "1"]]


# points 0 (lines 0, 1), 1 (2, 3), 2 (4, 5), 3 (6, 7): a0 - b0, b1 - c0, d0 - a1
CHAIN = (["images 8"] + ["line %d %d" % (i, i // 2) for i in range(8)] + ["point 0 0 0", "point 2 2 2", "point 4 4 4", "point 9 9 9"] +
         ["track %d %d %d ;" % (p, 2 * p, 2 * p + 1) for p in range(4)] + _sym(0, 2) + _sym(3, 4) + _sym(6, 1))


def test_merge_chain_recursion_and_stale_candidate(driver):
    """Merge(0): a0 -> point 1, ok: 0 + 1 -> 4 (track 0 1 2 3, position (2 * 0 + 2 * 2) / 4 = 1).  Merge(4): a0 -> b0 is its own; a1 -> d0: (4, 3) fails;
    b1 -> c0: (4, 2) ok: 4 + 2 -> 5 (track 0 1 2 3 4 5, position (4 * 1 + 2 * 4) / 6 = 2).  Merge(5): a1 -> d0: (5, 3) fails.  The recursion's count is 0, so
    Merge(4) returns 6 and Merge(0) returns that, not its own 4 (:684-689).  Points 1 and 2 are gone; point 3's only candidate is point 5, already tried."""
    out = _run(driver, CHAIN + ["ok 0 1 1", "ok 4 3 0", "ok 4 2 1", "ok 5 3 0", "merge ;", "state"])
    assert [r for r in out if r[0] in ("eval", "merge", "missing")] == [["eval", "0", "1"], ["merge", "0", "1", "4"], ["eval", "4", "3"], ["eval", "4", "2"],
                                                                           ["merge", "4", "2", "5"], ["eval", "5", "3"]]
    assert ["merged", "6", "merges", "2", "error", "0"] in out
    st = [r for r in out if r[0] in ("lp", "track")]
    assert st[0] == ["lp", "5", "5", "5", "5", "5", "5", "3", "3"]
    assert [r[3] for r in st[1:]] == ["0", "0", "0", "1", "0", "1"]      # exists: only point 3 and the last merged point
    assert st[5][5:8] == ["1", "1", "1"] and st[6][5:8] == ["2", "2", "2"] and st[6][9:] == ["0", "1", "2", "3", "4", "5"]


def test_merge_trials_are_kept_for_the_call_and_subsets_are_honoured(driver):
    """(0, 1) fails at point 0's turn and is not evaluated again from point 1's side; with the subset {1, 2} point 0 is not visited, so point 1 asks"""
    out = _run(driver, CHAIN + ["ok 0 1 0", "ok 1 0 0", "ok 1 2 0", "ok 2 1 0", "ok 0 3 0", "ok 3 0 0", "merge ;"])
    assert [r[1:] for r in out if r[0] == "eval"] == [["0", "1"], ["0", "3"], ["1", "2"]]
    out = _run(driver, CHAIN + ["ok 0 1 0", "ok 1 0 0", "ok 1 2 0", "ok 2 1 0", "ok 0 3 0", "ok 3 0 0", "merge 1 2 ;"])
    assert [r[1:] for r in out if r[0] == "eval"] == [["1", "0"], ["1", "2"]]
    assert ["merged", "0", "merges", "0", "error", "0"] in out


def test_merge_skips_unregistered_images_and_stops_at_an_evaluation_error(driver):
    # b0 (line 2) lies in the unregistered image 2: point 0 does not see point 1 through it, but point 1 sees point 0 through a0 (image 0)
    out = _run(driver, CHAIN + ["unreg 2", "ok 0 3 0", "ok 1 0 0", "ok 1 2 1", "ok 4 0 0", "merge ;"])
    assert [r[1:] for r in out if r[0] in ("eval", "missing")] == [["0", "3"], ["1", "0"], ["1", "2"], ["4", "0"]]
    assert ["merge", "1", "2", "4"] in out and ["merged", "4", "merges", "1", "error", "0"] in out
    # an evaluation that reports an error ends the call at once, after the first merge has been applied
    out = _run(driver, CHAIN + ["ok 0 1 1", "ok 4 3 -2", "merge ;", "state"])
    assert [r for r in out if r[0] in ("eval", "merge")] == [["eval", "0", "1"], ["merge", "0", "1", "4"], ["eval", "4", "3"]]
    assert ["merged", "4", "merges", "1", "error", "-2"] in out      # (the applied merge counts its 2 + 2 observations; the caller sees the error code)
    assert [r for r in out if r[0] == "lp"] == [["lp", "4", "4", "4", "4", "2", "2", "3", "3"]]
