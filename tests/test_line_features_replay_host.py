"""csrc/line_features_replay.hpp - the host half of the line-feature generator (K19) - without a device and under the sanitizers: the header is std only,
tests/line_features_replay_host_driver.cpp compiles with g++ -fsanitize=address,undefined and runs as its own program.  Its draws, alignment keys,
aligned counts, threshold keys and refusals must equal the Python mirror of feature_extraction.py with no tolerance: the draws are compared by the bits
of their doubles.  A sanitizer report ends the driver with a non-zero status."""
import os
import struct
import subprocess

import numpy as np
import pytest

from privacy_preserving_sfm_amd import feature_extraction as fe
from privacy_preserving_sfm_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("line_features_replay") / "line_features_replay_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "line_features_replay_host_driver.cpp")])
    return exe


def _run(exe, script):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    return out.stdout.splitlines()


CASES = [(0, 0), (0, 1), (1, 0), (7, 12345), (2**64 - 1, 2**31 - 1), (0x9E3779B97F4A7C15, -1), (42, -2**31)]


def test_draws_bit_for_bit(driver):
    lines = _run(driver, ["draws %d %d %d %d" % (seed, image, first, 300) for seed, image in CASES for first in (0, 2**31 - 300)])
    k = 0
    for seed, image in CASES:
        for first in (0, 2**31 - 300):
            got = lines[k].split()
            k += 1
            assert got[0] == "draws" and len(got) == 1 + 900
            want = fe.draws(seed, image, np.arange(first, first + 300)).reshape(-1)
            assert [int(v, 16) for v in got[1:]] == [struct.unpack("<Q", struct.pack("<d", float(v)))[0] for v in want]
            assert want.min() >= -1.0 and want.max() < 1.0


def test_keys(driver):
    lines = _run(driver, ["keys %d %d 0 500" % c for c in CASES])
    for line, (seed, image) in zip(lines, CASES):
        got = np.array([int(v, 16) for v in line.split()[1:]], dtype=np.uint64)
        assert np.array_equal(got, fe.align_keys(seed, image, np.arange(500)))
        assert np.array_equal(got & np.uint64(0xFFFFFFFF), np.arange(500, dtype=np.uint64))      # the index in the low half: no ties


RATIOS = (0.0, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.999, 1.0)


def test_counts(driver):
    sizes = list(range(41)) + [4096, 4097, 99999]
    lines = _run(driver, ["count %d %s" % (N, float(r).hex()) for N in sizes for r in RATIOS])
    k = 0
    for N in sizes:
        for r in RATIOS:
            assert lines[k] == "count %d" % fe.aligned_count(N, r), (N, r)
            k += 1


def test_thresholds(driver):
    script, want = [], []
    for seed, image in CASES[:4]:
        for N, r in ((1, 1.0), (63, 0.3), (64, 0.5), (257, 0.999), (4097, 0.3), (300, 1.0)):
            n = fe.aligned_count(N, r)
            script.append("threshold %d %d %d %d" % (seed, image, N, n))
            keys = fe.align_keys(seed, image, np.arange(N))
            want.append(int(np.sort(keys)[n - 1]))
            assert int((keys <= np.uint64(want[-1])).sum()) == n == int(fe.aligned_flags(seed, image, N, r).sum())
    assert [int(l.split()[1], 16) for l in _run(driver, script)] == want


def _validate(exe, ratio, cameras, starts, images):
    """cameras: (model, params); images: (camera, has_gravity, gravity)"""
    text = "validate %r %d %d |" % (float(ratio), len(cameras), len(images))
    for model, p in cameras:
        text += " %d %d %s" % (model, synthetic.NUM_PARAMS[model] if 0 <= model < 11 else -1, " ".join("%r" % float(v) for v in p))
    text += " | " + " ".join(str(s) for s in starts) + " |"
    for cam, hg, g in images:
        text += " %d %d %s" % (cam, hg, " ".join("%r" % float(v) for v in g))
    return _run(exe, [text])[0]


def test_validation(driver):
    cams = [(2, synthetic.default_intrinsics(2)[:4]), (10, synthetic.default_intrinsics(10))]
    imgs = [(0, 1, (0, 1, 0)), (1, 0, (0, 0, 0)), (1, 1, (0.6, 0.8, 0))]
    assert _validate(driver, 0.5, cams, [0, 5, 5, 9], imgs) == "ok"
    assert _validate(driver, 0.0, cams, [0, 0, 0, 0], imgs) == "ok" and _validate(driver, 1.0, [], [0], []) == "ok"
    assert _validate(driver, 0.5, cams, [0, 5, 5, 9], [(0, 0, (float("nan"),) * 3)] + imgs[1:]) == "ok"      # gravity is read only where the flag is set
    for ratio in (-0.1, 1.1, float("nan")):
        line = _validate(driver, ratio, cams, [0, 5, 5, 9], imgs)
        assert line.startswith("refused") and "aligned_line_ratio" in line
    for why, args in (("decreases", (0.5, cams, [0, 5, 4, 9], imgs)), ("kp_start[0]", (0.5, cams, [1, 5, 5, 9], imgs)),
                      ("out of range", (0.5, cams, [0, 5, 5, 9], [(2, 1, (0, 1, 0))] + imgs[1:])),
                      ("out of range", (0.5, cams, [0, 5, 5, 9], [(-1, 1, (0, 1, 0))] + imgs[1:])),
                      ("non-finite parameter", (0.5, [(2, [1000.0, 640.0, float("inf"), 0.01]), cams[1]], [0, 5, 5, 9], imgs)),
                      ("non-finite parameter", (0.5, [cams[0], (10, list(cams[1][1][:11]) + [float("nan")])], [0, 5, 5, 9], imgs)),
                      ("unknown model", (0.5, [(11, []), cams[1]], [0, 5, 5, 9], imgs)),
                      ("non-finite gravity", (0.5, cams, [0, 5, 5, 9], [(0, 1, (0, float("nan"), 0))] + imgs[1:])),
                      ("too many keypoints", (0.5, cams, [0, 5, 5, 2**31], imgs))):
        line = _validate(driver, *args)
        assert line.startswith("refused") and why in line, (why, line)
    for ratio in (-0.1, 1.1, float("nan")):
        assert _run(driver, ["count 10 %r" % ratio])[0].startswith("refused")
