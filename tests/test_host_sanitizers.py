"""The sanitizer configuration SURVEY.md section 5 asks for: the HOST halves of the library (image ordering, Cholesky task planner + replay, host
pair-list builder, co-visibility, sampler, exception containment) compiled with -fsanitize=address,undefined
(privacy_preserving_sfm_amd/build.py --host-asan) and driven through the C ABI by tests/host_sanitizer_driver.cpp, without a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_code_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    from privacy_preserving_sfm_amd import build
    lib = build.build_host_sanitized()
    rt = build.sanitizer_runtime_dir()
    exe = str(tmp_path / "host_sanitizer_driver")
    subprocess.check_call([build.hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined", "-shared-libsan",
                           os.path.join(ROOT, "tests", "host_sanitizer_driver.cpp"), "-x", "none", "-o", exe, lib,
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + rt, "-Wl,-rpath,/opt/rocm/lib"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1:protect_shadow_gap=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               LSAN_OPTIONS="suppressions=" + os.path.join(ROOT, "tests", "lsan_suppressions.txt"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    report = out.stdout[-3000:] + "\n" + out.stderr[-6000:]
    assert out.returncode == 0, report
    assert "host sanitizer driver: ok" in out.stdout
    assert "AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr and "LeakSanitizer" not in out.stderr, report


def test_oracle_is_clean_under_address_and_undefined_behaviour_sanitizers():
    """The CPU restatement itself (oracle/, the checker of every parity test) under the same sanitizers: `make -C oracle asan`, then the oracle's own
    CPU tests in a subprocess whose interpreter has libasan preloaded and PPSFM_ORACLE_ASAN=1 (tests/oracle_lib.py loads the sanitizer build)."""
    import sys
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "asan"])
    libasan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"]).decode().strip()
    if not os.path.isabs(libasan):
        pytest.skip("gcc has no libasan.so here")
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", PPSFM_ORACLE_ASAN="1")
    files = ["test_oracle_line_cost.py", "test_oracle_init_solvers.py", "test_oracle_bundle_adjustment.py", "test_oracle_absolute_pose.py"]
    out = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider"] + [os.path.join(ROOT, "tests", f) for f in files],
                         capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    report = out.stdout[-3000:] + "\n" + out.stderr[-6000:]
    assert out.returncode == 0 and " passed" in out.stdout, report
    assert "AddressSanitizer" not in report and "runtime error:" not in report, report
