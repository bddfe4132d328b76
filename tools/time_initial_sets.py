"""pp_tracks_find_initial_sets (K15) at one synthetic size, beside a std::map / std::set restatement of the reference's search on one host core
(tests/initial_sets_replay_host_driver.cpp --time, built here with g++ -O2 and no sanitizer into tools/_bin/).  The two alternate in one process; after
three warm-up rounds, ten timed ones.  Both must give the same totals and the same ranked sets in every round.  Prints the rounds and one JSON line.
    PYTHONPATH=. python tools/time_initial_sets.py"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import initial_sets_scenes as scenes      # noqa: E402
from test_initial_sets_replay_host import graph_script      # noqa: E402
from privacy_preserving_sfm_amd.device import TracksProblem, init_sets_options      # noqa: E402

WARMUP, REPEATS = 3, 10


def driver():
    exe = os.path.join(ROOT, "tools", "_bin", "initial_sets_driver")
    src = os.path.join(ROOT, "tests", "initial_sets_replay_host_driver.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, src])
    return exe


def main():
    exe = driver()
    scene = scenes.timing_scene()
    script = "\n".join(graph_script(scene)) + "\n"
    degree = [len(c) for l, c in enumerate(scene["corr"]) if scene["line_image"][l] in scene["check_images"] and c]
    pb = TracksProblem(scenes.to_flat(scene))
    options = init_sets_options()
    device, host = [], []
    for it in range(WARMUP + REPEATS):
        t0 = time.perf_counter()
        rep, sets = pb.find_initial_sets(scene["line_aligned"], scene["check_images"], None, options, capacity=1 << 16)
        wall = (time.perf_counter() - t0) * 1e3
        out = subprocess.run([exe, "--time"], input=script, capture_output=True, text=True, timeout=600, check=True).stdout.splitlines()
        ms = float([l for l in out if l.startswith("time_ms")][0].split()[1])
        totals = [int(x) for x in [l for l in out if l.startswith("totals")][0].split()[1:]]
        assert totals == [rep.num_candidates, rep.num_aligned_tracks, rep.num_random_tracks, rep.num_aligned_sets, rep.num_random_sets, rep.num_qualified]
        assert [[int(x) for x in l.split()[1:7]] for l in out if l.startswith("set")] == [list(s["images"]) + [s["num_aligned"], s["num_random"]] for s in sets]
        print("%2d%s device_ms %.3f replay_ms %.3f total_ms %.3f caller_ms %.3f | driver %.3f ms" %
              (it, " (warm-up)" if it < WARMUP else "", rep.device_ms, rep.replay_ms, rep.total_ms, wall, ms), flush=True)
        if it >= WARMUP:
            device.append((rep.device_ms, rep.total_ms, wall))
            host.append(ms)
    pb.close()
    device, host = np.array(device), np.array(host)
    stat = lambda a: dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()))      # noqa: E731
    print(json.dumps(dict(check_images=len(scene["check_images"]), images=scene["num_images"], lines=len(scene["line_image"]), work_lines=int(rep.num_work_lines),
                          neighbours=[min(degree), max(degree)], candidates=int(rep.num_candidates), unique_aligned=int(rep.num_aligned_tracks),
                          unique_random=int(rep.num_random_tracks), sets=int(rep.num_aligned_sets), qualified=int(rep.num_qualified), repeats=REPEATS,
                          device_ms=stat(device[:, 0]), total_ms=stat(device[:, 1]), caller_ms=stat(device[:, 2]), driver_ms=stat(host))))


if __name__ == "__main__":
    main()
