"""csrc/pair_selection_replay.hpp - the host half of the image-pair selection (K20) - without a device and under the sanitizers: the header is std
only, tests/pair_selection_replay_host_driver.cpp compiles with g++ -fsanitize=address,undefined and runs as its own program.  The argument checks must
refuse what pp_pairs_spatial / pp_pairs_transitive refuse, one case at a time; the uint64 key must order as (distance, index) tuples do; the literal host
rules must equal the independent references of pair_selection_cases.py, bit for bit.  A sanitizer report ends the driver with a non-zero status."""
import os
import subprocess

import numpy as np
import pytest

import pair_selection_cases as cases
from privacy_preserving_sfm_amd import feature_matching as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pair_selection_replay") / "pair_selection_replay_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "pair_selection_replay_host_driver.cpp")])
    return exe


def _run(exe, script):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    return out.stdout.splitlines()


def _bits(a):
    return " ".join(str(int(v)) for v in np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32))


def _spatial_line(exe, xyz, knn, max_distance, m=None, null_xyz=0):
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    return _run(exe, ["spatial %d %d %s %d %s" % (len(xyz) if m is None else m, knn, max_distance, null_xyz, _bits(xyz))])[0]


def _spatial(exe, xyz, knn, max_distance):
    head, body = _spatial_line(exe, xyz, knn, repr(float(max_distance))).split("|")
    name, n, visited = head.split()
    assert name == "spatial" and int(visited) == len(xyz) ** 2
    rows = np.array(body.split(), dtype=np.int64).reshape(-1, 3)
    assert len(rows) == int(n)
    return rows[:, :2].astype(np.int32), rows[:, 2].astype(np.uint32).view(np.float32)


def _transitive_line(exe, n, matched, tried, null_matched=0, null_tried=0, num_matched=None, num_tried=None):
    flat = lambda pairs: " ".join(str(int(v)) for v in np.asarray(pairs, dtype=np.int64).reshape(-1))
    return _run(exe, ["transitive %d %d %d %s %d %d %s" % (n, len(matched) if num_matched is None else num_matched, null_matched, flat(matched),
                                                           len(tried) if num_tried is None else num_tried, null_tried, flat(tried))])[0]


@pytest.mark.parametrize("args,why", [
    (dict(xyz=[(0, 0, 0)], knn=3, max_distance="1", m=-1), "negative number of locations"),
    (dict(xyz=[(0, 0, 0)], knn=3, max_distance="1", null_xyz=1), "null locations"),
    (dict(xyz=[(0, 0, 0)], knn=0, max_distance="1"), "max_num_neighbors"),
    (dict(xyz=[(0, 0, 0)], knn=-2, max_distance="1"), "max_num_neighbors"),
    (dict(xyz=[(0, 0, 0)], knn=3, max_distance="0"), "max_distance"),
    (dict(xyz=[(0, 0, 0)], knn=3, max_distance="-4"), "max_distance"),
    (dict(xyz=[(0, 0, 0)], knn=3, max_distance="nan"), "max_distance"),
    (dict(xyz=[(0, 0, 0), (1, np.nan, 0)], knn=3, max_distance="1"), "location 1"),
    (dict(xyz=[(0, 0, -np.inf), (1, 0, 0)], knn=3, max_distance="1"), "location 0"),
])
def test_the_spatial_refusals(driver, args, why):
    line = _spatial_line(driver, **args)
    assert line.startswith("refused") and why in line


def test_the_spatial_check_accepts_the_edges(driver):
    assert _spatial_line(driver, np.zeros((0, 3)), 5, "inf", null_xyz=1).startswith("spatial 0 0")      # no locations: no array needed
    assert _spatial_line(driver, [(0, 0, 0), (3e38, 0, 0)], 5, "1e300").startswith("spatial 2 4")      # a distance may overflow to +inf: still ordered


@pytest.mark.parametrize("args,why", [
    (dict(n=-1, matched=[], tried=[]), "negative number of images"),
    (dict(n=3, matched=[], tried=[], num_matched=-1), "negative number of pairs"),
    (dict(n=3, matched=[], tried=[], num_tried=-1), "negative number of pairs"),
    (dict(n=3, matched=[(0, 1)], tried=[], null_matched=1), "null pairs"),
    (dict(n=3, matched=[(0, 1)], tried=[(1, 2)], null_tried=1), "null pairs"),
    (dict(n=3, matched=[(0, 1), (1, 3)], tried=[]), "matched pair 1"),
    (dict(n=3, matched=[(0, 1)], tried=[(-1, 2)]), "tried pair 0"),
    (dict(n=0, matched=[(0, 0)], tried=[]), "matched pair 0"),
])
def test_the_transitive_refusals(driver, args, why):
    line = _transitive_line(driver, **args)
    assert line.startswith("refused") and why in line


def test_the_key_orders_as_distance_index_tuples(driver):
    rng = np.random.default_rng(3)
    dist = np.concatenate([rng.uniform(0, 1e4, 40), [0.0, 0.0, 0.0, 1e-45, 1e-45, 1.17e-38, np.inf, np.inf, 3.4e38, 0.5, 0.5, 0.5]]).astype(np.float32)
    dist = np.concatenate([dist, dist[:20]])      # equal distances under different indices
    index = rng.permutation(len(dist)).astype(np.uint32)
    index[:6] = [0, 1, 255, 256, 65536, 2 ** 31 - 2]      # every byte of the index takes part in the order
    tokens = " ".join("%d %d" % (b, i) for b, i in zip(dist.view(np.uint32), index))
    order = [int(v) for v in _run(driver, ["keys %d %s" % (len(dist), tokens)])[0].split()[1:]]
    assert order == sorted(range(len(dist)), key=lambda k: (float(dist[k]), int(index[k])))


def _assert_host_rule_is_flann(driver, xyz, knn, max_distance):
    pairs, sqdist = _spatial(driver, xyz, knn, max_distance)
    ref_pairs, ref_dist = cases.flann_pairs(np.asarray(xyz, dtype=np.float32), knn, max_distance)
    assert np.array_equal(pairs, ref_pairs) and np.array_equal(sqdist.view(np.uint32), ref_dist.view(np.uint32))
    return pairs


def test_the_spatial_host_rule_on_the_fixtures(driver):
    _, xyz, options = cases.gps_fixture()
    _assert_host_rule_is_flann(driver, xyz, options.max_num_neighbors, options.max_distance)
    _, xyz, options = cases.cartesian_fixture()      # bit for bit: the host's distance is the unfused chain
    _assert_host_rule_is_flann(driver, xyz, options.max_num_neighbors, options.max_distance)


def test_the_spatial_host_rule_on_the_edge_cases(driver):
    same = np.tile(np.array([[3.0, 4.0, 5.0]], dtype=np.float32), (70, 1))
    pairs = _assert_host_rule_is_flann(driver, same, 50, 1.0)
    assert [b for a, b in pairs.tolist() if a == 60] == list(range(50))      # the query falls out of its own list
    _assert_host_rule_is_flann(driver, cases.lattice_locations(), 30, 1.5)
    rng = np.random.default_rng(5)
    for m, knn in ((5, 9), (1, 1), (1, 4), (0, 3)):
        _assert_host_rule_is_flann(driver, rng.uniform(0, 10, (m, 3)).astype(np.float32), knn, 100.0)


@pytest.mark.parametrize("name", sorted(cases.transitive_graphs()))
def test_the_transitive_host_rule(driver, name):
    n, matches = cases.transitive_graphs()[name]
    _, matched, tried = fm.transitive_pair_lists(n, matches)
    want = sorted(tuple(sorted(p)) for p in cases.transitive_literal(matches))
    for listed in (tried, tried[: len(tried) // 2]):      # the matched pairs count as tried whether they are listed there or not
        if len(listed) < len(tried) and any(len(m) == 0 for m in matches.values()):
            continue      # (halving the list would drop a tried-but-empty pair)
        head, body = _transitive_line(driver, n, matched, listed).split("|")
        pairs = np.array(body.split(), dtype=np.int64).reshape(-1, 2)
        assert head.split()[0] == "transitive" and int(head.split()[1]) == len(pairs)
        assert [tuple(p) for p in pairs.tolist()] == want
