"""csrc/corr_graph_replay.hpp - the host half of the correspondence-graph builder (K18) - without a device and under the sanitizers: the header is std
only, tests/corr_graph_replay_host_driver.cpp compiles with g++ -fsanitize=address,undefined and runs as its own program.  The sequential rule
(CorrReplayPair) must equal feature_matching.build_correspondence_graph on the hand-made lists of test_feature_matching_host.py, on the shadow case
(a, x) (a, y) (b, y) and on random lists with repeats on both sides; the classifier (CorrClassifyPair / CorrNeedsReplay) must name exactly the pairs with
repeats on both sides, and wherever it does not, the parallel rule (first occurrence on both sides) must equal the sequential one; the pair plan must store,
order and refuse pairs as DatabaseCache::Load would.  A sanitizer report ends the driver with a non-zero status."""
import os
import subprocess

import numpy as np
import pytest

from privacy_preserving_sfm_amd import feature_matching as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("corr_graph_replay") / "corr_graph_replay_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "corr_graph_replay_host_driver.cpp")])
    return exe


def _run(exe, script):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    return out.stdout.splitlines()


def _pair(exe, n1, n2, m):
    m = np.asarray(m, dtype=np.int64).reshape(-1, 2)
    line = _run(exe, ["pair %d %d %d %s" % (n1, n2, len(m), " ".join(str(int(v)) for v in m.reshape(-1)))])[0]
    head, seq, first = (part.split() for part in line.split("|"))
    assert head[0] == "pair"
    valid, rep1, rep2, needs = (int(v) for v in head[1:])
    seq, first = [int(v) for v in seq], [int(v) for v in first]
    assert seq[0] == sum(seq[1:]) and first[0] == sum(first[1:]) and len(seq) == len(first) == len(m) + 1
    return dict(valid=valid, rep1=rep1, rep2=rep2, needs=bool(needs), seq=seq[1:], first=first[1:])


def _mirror_flags(n1, n2, m):
    """which matches build_correspondence_graph lets into the graph of the single pair (1, 2)"""
    m = np.asarray(m, dtype=np.int64).reshape(-1, 2)
    graph, _ = fm.build_correspondence_graph({(1, 2): m}, {1: n1, 2: n2}, min_num_matches=0)
    flags, taken = [], set()
    for x1, x2 in m:
        hit = (2, int(x2)) in graph.FindCorrespondences(1, int(x1)) and (int(x1), int(x2)) not in taken
        taken.add((int(x1), int(x2)))
        flags.append(int(hit))
    assert sum(flags) == sum(1 for k in graph._corrs if k[0] == 1)
    return flags


def _independent_class(n1, n2, m):
    valid = [(int(a), int(b)) for a, b in np.asarray(m).reshape(-1, 2) if 0 <= a < n1 and 0 <= b < n2]
    return len(valid), len(valid) - len({a for a, _ in valid}), len(valid) - len({b for _, b in valid})


def test_the_hand_made_lists(driver):
    m12 = [(0, 0), (1, 1), (2, 2), (2, 5), (6, 1), (3, 12), (11, 3), (4, 4)]      # test_feature_matching_host.py
    got = _pair(driver, 10, 10, m12)
    assert got["seq"] == [1, 1, 1, 0, 0, 0, 0, 1] == _mirror_flags(10, 10, m12)
    assert (got["valid"], got["rep1"], got["rep2"]) == (6, 1, 1) and got["needs"]      # repeats on both sides: (2, 5) and (6, 1)
    for m in ([(7, 5), (8, 6), (9, 7)], [(1, 4), (2, 5), (3, 0)], [(4, 0), (5, 1), (0, 2)]):
        got = _pair(driver, 10, 10, m)
        assert got["seq"] == got["first"] == [1, 1, 1] == _mirror_flags(10, 10, m) and not got["needs"]
    assert _pair(driver, 4, 4, np.zeros((0, 2)))["seq"] == []
    got = _pair(driver, 0, 4, [(0, 0), (-1, 2)])      # an image without lines: nothing is valid
    assert got["seq"] == [0, 0] and got["valid"] == 0 and not got["needs"]


def test_the_shadow_case(driver):
    a, b, x, y = 3, 5, 2, 7
    m = [(a, x), (a, y), (b, y)]
    got = _pair(driver, 8, 8, m)
    assert got["seq"] == [1, 0, 1] == _mirror_flags(8, 8, m)      # the third is accepted because the second was rejected
    assert got["first"] == [1, 0, 0]                               # the parallel rule alone would lose it
    assert got["needs"] and (got["rep1"], got["rep2"]) == (1, 1)


@pytest.mark.parametrize("seed", range(6))
def test_random_lists_with_repeats_on_both_sides(driver, seed):
    rng = np.random.default_rng(seed)
    n1, n2 = int(rng.integers(3, 12)), int(rng.integers(3, 12))
    m = np.stack([rng.integers(-1, n1 + 1, 60), rng.integers(-1, n2 + 1, 60)], axis=1)      # out-of-range indices on both ends too
    got = _pair(driver, n1, n2, m)
    assert got["seq"] == _mirror_flags(n1, n2, m)
    assert (got["valid"], got["rep1"], got["rep2"]) == _independent_class(n1, n2, m)
    assert got["needs"] and got["rep1"] > 0 and got["rep2"] > 0


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("side", [0, 1, None])
def test_the_classifier_and_the_parallel_rule_on_one_sided_repeats(driver, seed, side):
    rng = np.random.default_rng(100 + seed)
    n1 = n2 = 40
    m = np.stack([rng.permutation(n1)[:30], rng.permutation(n2)[:30]], axis=1)      # no repeat on either side
    if side is not None:
        m[:, side] = rng.integers(0, 12, 30)                                        # repeats on this side only
    m[rng.integers(0, 30, 4), int(rng.integers(0, 2))] = [-1, 40, 41, -7]             # and some indices that do not exist
    got = _pair(driver, n1, n2, m)
    valid, rep1, rep2 = _independent_class(n1, n2, m)
    assert (got["valid"], got["rep1"], got["rep2"]) == (valid, rep1, rep2)
    assert not got["needs"] and (rep1 == 0 or rep2 == 0)
    assert got["seq"] == got["first"] == _mirror_flags(n1, n2, m)


def _plan(exe, num_images, min_num_matches, pairs):
    return _run(exe, ["plan %d %d %d %s" % (num_images, min_num_matches, len(pairs), " ".join("%d %d %d" % p for p in pairs))])[0]


def test_the_pair_plan(driver):
    pairs = [(3, 1, 5), (1, 2, 4), (2, 2, 9), (0, 4, 3), (4, 3, 0), (2, 3, 4)]      # (a, b, matches); min_num_matches = 3
    head, connected, rows = (part.split() for part in _plan(driver, 5, 3, pairs).split("|"))
    assert head == ["plan", "3"]
    assert [int(v) for v in connected] == [0, 1, 1, 1, 0]      # the used self pair (2, 2) connects image 2; (0, 4) has exactly 3: unused
    rows = np.array(rows, dtype=np.int64).reshape(-1, 5)
    #                              image1 image2 swapped used rank: ascending (image1, image2) over the used pairs that are no self pair
    assert rows.tolist() == [[1, 3, 1, 1, 1], [1, 2, 0, 1, 0], [2, 2, 0, 1, -1], [0, 4, 0, 0, -1], [3, 4, 1, 0, -1], [2, 3, 0, 1, 2]]


@pytest.mark.parametrize("num_images,min_num_matches,pairs,why", [
    (3, 0, [(0, 1, 2), (1, 0, 2)], "listed twice"), (3, 0, [(0, 1, 2), (2, 2, 1), (2, 2, 0)], "listed twice"),
    (3, 0, [(0, 3, 2)], "out of range"), (3, 0, [(-1, 1, 2)], "out of range"), (3, -1, [(0, 1, 2)], "negative"),
    (3, 0, [(0, 1, 2), (1, 2, -1)], "decreases")])
def test_the_plan_refuses_bad_input(driver, num_images, min_num_matches, pairs, why):
    line = _plan(driver, num_images, min_num_matches, pairs)
    assert line.startswith("refused") and why in line
