"""csrc/sift_match_replay.hpp - the host half of the SIFT matcher (K17) - without a device and under the sanitizers: the header is std only,
tests/sift_match_replay_host_driver.cpp compiles with g++ -fsanitize=address,undefined.  The integer thresholds must agree with the reference's two float
rules evaluated directly - for every best of the table against every second within 64 of its boundary and on 200 000 random pairs - and with the integers
tests/sift_match_reference.py derives from the definitions; the host one-way scan, decision and cross-check must agree with the Python reference on
generated descriptor pairs.  A sanitizer report ends the driver with a non-zero status."""
import os
import subprocess

import numpy as np
import pytest

import sift_match_reference as ref
from privacy_preserving_sfm_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_SETS = [(0.8, 0.7), (1.5, 0.7), (0.8, 3.0), (0.8, 1e-3), (1e-3, 0.7)]      # (max_ratio, max_distance)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sift_match_replay") / "sift_match_replay_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "sift_match_replay_host_driver.cpp")])
    return exe


def _run(exe, script):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    return [l.split() for l in out.stdout.splitlines()]


def _rows(d):
    return [bytes(row).hex() for row in np.asarray(d, dtype=np.uint8).reshape(-1, 128)]


@pytest.mark.parametrize("ratio,distance", OPTION_SETS)
def test_the_thresholds_agree_with_the_float_rules(driver, tmp_path, ratio, distance):
    path = str(tmp_path / "table.bin")
    out = _run(driver, ["thresholds %r %r" % (ratio, distance), "dump %r %r %s" % (ratio, distance, path)])
    assert out[0][0] == "thresholds" and out[1][0] == "dump", out
    d_min, count, checked, mismatches = (int(v) for v in out[0][1:])
    assert mismatches == 0 and checked > 200000
    assert count == ref.CLAMP - d_min + 1
    r_d_min, r_table = ref.thresholds(ratio, distance)
    table = np.fromfile(path, dtype=np.int32)
    assert d_min == r_d_min == int(out[1][1]) and len(table) == count
    assert np.array_equal(table, r_table)


def test_the_default_thresholds_are_the_documented_ones(driver):
    out = _run(driver, ["thresholds 0.8 0.7"])
    assert out[0][:3] == ["thresholds", "200499", "61646"]      # cos(0.7) * 2^18 = 200499.6


def test_bad_options_are_refused(driver):
    out = _run(driver, ["thresholds 0 0.7", "thresholds 0.8 -1", "thresholds nan 0.7"])
    assert [l[0] for l in out] == ["refused"] * 3 and all(l[1] == "invalid:" for l in out)


CASES = [dict(n1=60, n2=47, shared=30, noise=0.35, seed=1, duplicates=3, zero_rows=2), dict(n1=33, n2=70, shared=33, noise=0.8, seed=2, duplicates=4),
         dict(n1=1, n2=5, shared=1, noise=0.1, seed=3), dict(n1=5, n2=1, shared=1, noise=0.1, seed=4), dict(n1=0, n2=4, shared=0, noise=0.1, seed=5),
         dict(n1=4, n2=0, shared=0, noise=0.1, seed=6)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d" % (c["n1"], c["n2"]))
@pytest.mark.parametrize("cross,ratio,distance", [(1, 0.8, 0.7), (0, 0.8, 0.7), (1, 1.5, 0.7), (1, 0.8, 3.0)])
def test_the_host_restatement_agrees_with_the_python_reference(driver, case, cross, ratio, distance):
    pair = synthetic.make_descriptor_pair(**case)
    d1, d2 = pair["d1"], pair["d2"]
    out = _run(driver, ["match %d %d %d %r %r" % (len(d1), len(d2), cross, ratio, distance)] + _rows(d1) + _rows(d2))
    assert out[0][0] == "top2" and out[1][0] == "matches"
    got = np.array(out[0][2:], dtype=np.int64).reshape(-1, 3)
    dists = ref.dist_matrix(d1, d2)
    for k, want in enumerate(ref.top2(dists)):
        assert np.array_equal(got[:, k], want)
    for k, want in enumerate(ref.top2_sequential(dists)):      # (the order-free statement equals the scan as the reference writes it)
        assert np.array_equal(got[:, k], want)
    matches = np.array(out[1][2:], dtype=np.int32).reshape(-1, 2)
    assert int(out[1][1]) == len(matches)
    assert np.array_equal(matches, ref.match(d1, d2, ratio, distance, bool(cross)))
