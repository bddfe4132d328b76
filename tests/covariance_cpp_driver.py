"""Builds tests/cpp_covariance_compile_test.cpp against libppsfm_hip.so (shared by the host compile test and the device test of the C++ mirror)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(tmp_path):
    from privacy_preserving_sfm_amd import build
    build.build_library()
    exe = os.path.join(str(tmp_path), "cpp_covariance_compile_test")
    libdir = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "cpp_covariance_compile_test.cpp"), "-L" + libdir,
                           "-lppsfm_hip", "-Wl,-rpath," + libdir])
    return exe
