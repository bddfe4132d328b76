"""ppsfm/ppsfm.hpp's global refinement part (Normalize, GlobalBundleAdjustmentOptions, AdjustGlobalBundle, IterativeGlobalRefinement) compiles with
g++ -std=c++14 against the C ABI; its host-only Normalize gives what the Python mirror gives (reference src/base/reconstruction.cc:302-397)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_global_refinement_compiles_links_and_normalizes(tmp_path):
    from privacy_preserving_sfm_amd import build
    from privacy_preserving_sfm_amd.bundle_adjustment import Camera, Image, Point3D, Reconstruction
    exe = str(tmp_path / "refinement_test")
    libdir = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "cpp_global_refinement_compile_test.cpp"),
                           "-L" + libdir, "-lppsfm_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines() if line.strip()}
    assert rows["options"] == ["100", "50", "0.1", "1", "200", "100"]
    assert out.stdout.count("caught:") + out.stdout.count("returned") + out.stdout.count("rounds") == 2     # both device functions were called
    # the same scene through the Python mirror
    rec = Reconstruction()
    rec.cameras[0] = Camera(0, 2, [1000.0, 640.0, 480.0, 0.01])
    for c in range(5):
        a, h = 0.3 * c, np.sqrt(1.0 - 0.04 - 0.01)
        rec.images[c] = Image(c, 0, [h * np.cos(a), 0.2, h * np.sin(a), 0.1], [0.5 * c - 1.0, 0.25 * c * c, 4.0 - 0.7 * c])
    for p in range(6):
        rec.points3D[p] = Point3D([0.1 * p, -0.2 * p, 0.05 * p * p])
    before = np.array([rec.images[c].tvec for c in range(5)])
    rec.Normalize()
    want_poses = np.array([np.concatenate([rec.images[c].qvec, rec.images[c].tvec]) for c in range(5)])
    want_points = np.array([rec.points3D[p].xyz for p in range(6)])
    got_poses = np.array(rows["poses"], dtype=np.float64).reshape(5, 7)
    got_points = np.array(rows["points"], dtype=np.float64).reshape(6, 3)
    assert np.abs(want_poses[:, 4:] - before).max() > 0.1
    assert np.allclose(got_poses, want_poses, rtol=1e-13, atol=1e-13) and np.allclose(got_points, want_points, rtol=1e-13, atol=1e-13)
