"""csrc/lomsac_host.hpp - the host replay every accept, local optimisation and termination of pp_planar_lomsac, pp_pose2d_lomsac and pp_fourview2d_lomsac
comes from - without a device: the header compiles with plain g++ and, over a toy line-fitting backend (tests/lomsac_host_driver.cpp), reproduces the trace
the reference's own RansacLib headers print on the same data (tests/golden/ransaclib_trace_n200.txt, which so far pinned only the oracle's restatement) and
agrees with oracle::LocallyOptimizedMSAC over a grid of sizes, outlier patterns and options.  The same program runs under ASan + UBSan as a plain executable."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ransaclib_trace_n200.txt")
SOURCE = os.path.join(ROOT, "tests", "lomsac_host_driver.cpp")
PP_OK, PP_ERR_HIP, PP_ERR_NUMERIC = 0, -2, -3


def _compile(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / "lomsac_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, SOURCE])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _compile(tmp_path_factory, "lomsac_host", ["-O1"])


@pytest.fixture(scope="module")
def sanitized_driver(tmp_path_factory):
    return _compile(tmp_path_factory, "lomsac_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def _fields(line):
    return dict(t.split("=") for t in line.split())


def test_header_compiles_alone_without_warnings(tmp_path):
    """std + include/ppsfm_hip.h only: no common.hpp, no HIP"""
    src = tmp_path / "only_the_header.cpp"
    src.write_text('#include "%s"\nint main() { return 0; }\n' % os.path.join(ROOT, "privacy_preserving_sfm_amd", "csrc", "lomsac_host.hpp"))
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr


@pytest.mark.parametrize("backend", ["immediate", "deferred"])
@pytest.mark.parametrize("chunk", [0, 1, 7, 64])
def test_replay_reproduces_the_reference_driver_trace(driver, chunk, backend):
    """what test_lomsac_restatement_equals_reference_driver_trace asserts of the oracle's restatement, of the product's loop - byte for byte, and
    whatever the speculation width and whether the scores of a local optimisation are deferred"""
    assert _run(driver, "trace", chunk, backend) == open(GOLDEN).read()


def test_replay_equals_the_oracle_driver_over_the_grid(driver):
    """n in {1, 2, 5, 6, 12, 40, 200} x outliers {none, every 2nd, every 3rd} x 3 seeds x lo_starting_iterations {0, 10, 50, 5000} x num_lo_steps
    {0, 3, 10} x final_least_squares {0, 1} x chunk {0, 1, 7} x {immediate, deferred}: iterations, LO count, inlier count and indices, score, ratio
    and model equal with == on doubles"""
    assert _run(driver, "sweep").strip() == "cases=9072 mismatches=0"


def test_fewer_data_than_a_minimal_sample(driver):
    r = _fields(_run(driver, "small"))
    assert r == dict(rc=str(PP_OK), iterations="0", lo="0", inliers="0", indices="0", hypotheses="0", score_is_max="1", ratio="0", model="0,0,0")


@pytest.mark.parametrize("final_least_squares", [0, 1])
def test_every_minimal_sample_degenerate(driver, final_least_squares):
    """all points equal: no model, the score stays DBL_MAX, the loop runs max(min, max) = 1000 iterations and returns the zero model it started from;
    the final least squares (a fit to no inliers) changes nothing, as in the oracle's driver"""
    result, same = _run(driver, "degenerate", final_least_squares).splitlines()
    assert _fields(result) == dict(rc=str(PP_OK), iterations="1000", lo="0", inliers="0", indices="0", hypotheses="1000", score_is_max="1", ratio="0",
                                   model="0,0,0")
    assert same == "same_as_oracle=1"


def test_a_failing_backend_ends_the_run_with_its_code(driver):
    """rc becomes non-zero in the third GetInliers: LoMsacRun returns that code (immediate backend, deferred backend)"""
    assert _run(driver, "fail").split() == ["rc=%d" % PP_ERR_HIP, "rc=%d" % PP_ERR_NUMERIC]


def test_trace_and_sweep_clean_under_asan_and_ubsan(sanitized_driver):
    for chunk, backend in ((0, "immediate"), (7, "deferred")):
        assert _run(sanitized_driver, "trace", chunk, backend) == open(GOLDEN).read()
    assert _run(sanitized_driver, "sweep").strip() == "cases=9072 mismatches=0"
