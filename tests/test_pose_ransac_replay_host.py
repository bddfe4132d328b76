"""csrc/ransac_host.hpp's PoseRansacReplay - every sequential rule of pp_pose_ransac: a-priori trial cap, sampler, speculation width, which models need an
exact sequential sum, accept and tie-break in trial order, adaptive termination, num_trials - without a device: the header compiles with plain g++ and,
over the oracle's own solver and scoring as its backend (tests/pose_ransac_replay_host_driver.cpp), reports what oracle::P6LRansac reports on the same data
and seed, with == on every field and memcmp on the model, whatever the chunk width.  The same program runs under ASan + UBSan as a plain executable."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "pose_ransac_replay_host_driver.cpp")
# every rule of the replay the grid has to exercise: a count of 0 would let the comparison pass without it
CONDITIONS = ["small", "success", "early", "capped", "no_model", "ties", "ties_won"]


def _compile(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / "pose_ransac_replay_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"] + flags + ["-o", exe, SOURCE])      # (the OpenMP pragmas of oracle/linalg.h)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _compile(tmp_path_factory, "pose_ransac_replay_host", ["-O1"])


@pytest.fixture(scope="module")
def sanitized_driver(tmp_path_factory):
    return _compile(tmp_path_factory, "pose_ransac_replay_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def _counters(exe, mode):
    out = _run(exe, mode)
    print(out)
    return {k: int(v) for k, v in (t.split("=") for t in out.split())}


def test_header_compiles_alone_without_warnings(tmp_path):
    """std + include/ppsfm_hip.h only: no common.hpp, no HIP"""
    src = tmp_path / "only_the_header.cpp"
    src.write_text('#include "%s"\nint main() { return 0; }\n' % os.path.join(ROOT, "privacy_preserving_sfm_amd", "csrc", "ransac_host.hpp"))
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr


def test_sampler_equals_the_oracle_sampler(driver):
    """1000 six-tuples for each of n in {6, 7, 40, 2000} x seeds {0, 1, 7}: this toolchain's <random> against the oracle's restated MT19937 + integer rule"""
    assert _run(driver, "sampler").strip() == "draws=12000 mismatches=0"


def test_replay_equals_the_oracle_loop_over_the_grid(driver):
    """n in {5, 6, 7, 12, 40, 150} x outlier ratio {0, 0.3, 0.6} x aligned ratio {0, 0.2, 1.1} x seeds {0, 1, 7} x chunk_trials {1, 2, 7, 64, 0} x six option
    sets (the mapper's; the defaults; max_num_trials = 1; confidence = 1 under a cap of 300; min_inlier_ratio = 1; min_inlier_ratio = 0 with min = max = 150):
    success, num_trials, best_trial, best_model_index, num_inliers, residual_sum and the 12 doubles of the model equal the oracle's, no tolerance.
    The grid contains runs with n < 6, successful runs, runs the adaptive bound ended early, runs that reached the cap, runs that never saw a model, ties on
    the inlier count and ties the sequential sum decided for the newcomer."""
    c = _counters(driver, "sweep")
    assert c["cases"] == 4860 and c["mismatches"] == 0 and c["oracle_trials"] > 0
    for name in CONDITIONS:
        assert c[name] > 0, name


def test_sub_grid_clean_under_asan_and_ubsan(sanitized_driver):
    """seed 1 and chunk_trials {1, 7, 0} of the grid above (a fifth of it, every condition still met), and the sampler comparison"""
    assert _run(sanitized_driver, "sampler").strip() == "draws=12000 mismatches=0"
    c = _counters(sanitized_driver, "subsweep")
    assert c["cases"] == 972 and c["mismatches"] == 0
    for name in CONDITIONS:
        assert c[name] > 0, name
