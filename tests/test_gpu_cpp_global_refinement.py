"""ppsfm::IterativeGlobalRefinement (ppsfm/ppsfm.hpp) EXECUTED on the device, in the manner of tests/test_gpu_cpp_mirror.py: tests/cpp_global_refinement_gpu_test.cpp
is built with g++ against libppsfm_hip.so and run as a child process on the noisy cfg-1 scene of tests/test_gpu_global_refinement.py (seed 0x260, on which
the oracle's loop is reproducible); its report is compared with the Python mirror's run on the same device (reference
src/controllers/incremental_mapper.cc:102-124): the same rounds, counts, `changed` and deleted observations, parameters within 1e-5 of the array's
largest entry."""
import os
import subprocess

import numpy as np
import pytest

import refinement_oracle
from privacy_preserving_sfm_amd import synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_iterative_global_refinement_equals_the_python_mirror(tmp_path):
    from privacy_preserving_sfm_amd import build
    from privacy_preserving_sfm_amd.bundle_adjustment import IncrementalMapperOptions, IterativeGlobalRefinement, Reconstruction
    exe = str(tmp_path / "cpp_global_refinement_gpu_test")
    libdir = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "cpp_global_refinement_gpu_test.cpp"),
                           "-L" + libdir, "-lppsfm_hip", "-Wl,-rpath," + libdir])
    sc = synthetic.make_ba_scene(20, 500, 4, seed=0x260, model=2, **refinement_oracle.NOISY)
    C, P, K, M = 20, 500, 1, len(sc["obs_pose"])
    path = str(tmp_path / "scene.txt")
    with open(path, "w") as f:
        f.write("\n".join(str(v) for v in (C, P, K, M)) + "\n")
        for a in (sc["lines"], sc["obs_pose"], sc["obs_point"], sc["pose_camera"], sc["camera_model"], sc["poses"], sc["points"], sc["intr"]):
            a = np.asarray(a)
            f.write("\n".join(repr(float(x)) if a.dtype.kind == "f" else str(int(x)) for x in a.ravel()) + "\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        key, _, rest = line.partition(" ")
        rows.setdefault(key, []).append(rest.split())
    options = IncrementalMapperOptions()
    options.print_summary = False
    rec = Reconstruction.from_scene(sc)
    rep = IterativeGlobalRefinement(rec, options)
    # observation o of the flat scene is (image, line index) in the Python data model
    count, ref_of = {}, []
    for c in sc["obs_pose"]:
        k = count.get(int(c), 0)
        count[int(c)] = k + 1
        ref_of.append((int(c), k))
    assert int(rows["rounds"][0][0]) == rep.num_rounds
    for r in range(rep.num_rounds):
        nf, changed, its, term, npd = rows["round"][r]
        assert int(nf) == rep.num_filtered[r] and float(changed) == rep.changed[r] and int(npd) == len(rep.point_deleted[r])
        assert (int(its), int(term)) == (rep.summaries[r].num_iterations, rep.summaries[r].termination)
        assert sorted(ref_of[int(o)] for o in rows["obs_deleted"][r]) == rep.obs_deleted[r]
    poses, points, ids = refinement_oracle.parameters(rec)
    cposes = np.array(rows["poses"][0], dtype=np.float64).reshape(C, 7)
    alive = np.array(rows["alive"][0], dtype=np.int64).astype(bool)
    cpoints = np.array(rows["points"][0], dtype=np.float64).reshape(P, 3)
    assert list(np.flatnonzero(alive)) == ids and int(rows["left"][0][0]) == rec.ComputeNumObservations()
    assert np.abs(cposes - poses).max() <= 1e-5 * np.abs(poses).max() and np.abs(cpoints[alive] - points).max() <= 1e-5 * np.abs(points).max()
