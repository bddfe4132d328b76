"""BundleAdjuster.flatten() (the host loop over the model) beside BundleAdjuster.flatten_on(session) (pp_tracks_bundle_setup, K16) at the headline scene's
shape: Reconstruction.from_scene(make_ba_scene(500, 25000, 8)) - 500 images, 200k observations - the cameras sized, an empty correspondence graph, ONE
handle open.  Two configs: the global one (every image), and a local one (7 images, 500 variable points).  The two routes alternate in one process; after one
warm-up round, five timed ones; the warm-up round also checks that both routes return the same arrays.  Host clocks around calls that end synchronised
(flatten_on returns host arrays); device_ms / replay_ms are the call's own report.  Prints the rounds and one JSON line per config.
    PYTHONPATH=. python tools/bundle_setup_timing.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bundle_setup_worlds as bsw      # noqa: E402
from privacy_preserving_sfm_amd.bundle_adjustment import BundleAdjuster      # noqa: E402
from privacy_preserving_sfm_amd.incremental_triangulator import CorrespondenceGraph, IncrementalTriangulator      # noqa: E402

WARMUP, REPEATS = 1, 5
SHAPE = (500, 25000, 8)


def main():
    t0 = time.perf_counter()
    rec = bsw.world(*SHAPE)
    t1 = time.perf_counter()
    tri = IncrementalTriangulator(CorrespondenceGraph(), rec)
    ses = tri._open(tri.Options())
    print("world %.1f s, session open (IncrementalTriangulator.flatten + pp_tracks_create) %.1f s" % (t1 - t0, time.perf_counter() - t1), flush=True)
    options = bsw.options(False)
    configs = (("global", bsw.global_config(rec)), ("local", bsw.local_config(rec, images=tuple(range(7)), num_variable=500)))
    try:
        for name, cfg in configs:
            rows = []
            for it in range(WARMUP + REPEATS):
                t0 = time.perf_counter()
                want = bsw.flatten_and_restore(BundleAdjuster(options, cfg), rec)
                host_ms = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                got = BundleAdjuster(options, cfg).flatten_on(ses)
                on_ms = (time.perf_counter() - t0) * 1e3
                rep = ses.last_bundle_setup_report
                if it < WARMUP:
                    bsw.assert_same_flatten(got, want)
                print("%s %d%s flatten %.2f ms | flatten_on %.2f ms (call total_ms %.3f device_ms %.3f replay_ms %.3f)" %
                      (name, it, " (warm-up)" if it < WARMUP else "", host_ms, on_ms, rep.total_ms, rep.device_ms, rep.replay_ms), flush=True)
                if it >= WARMUP:
                    rows.append((host_ms, on_ms, rep.total_ms, rep.device_ms, rep.replay_ms))
            a = np.array(rows)
            stat = lambda c: dict(median=float(np.median(a[:, c])), min=float(a[:, c].min()), max=float(a[:, c].max()))      # noqa: E731
            print(json.dumps(dict(config=name, shape=list(SHAPE), config_images=cfg.NumImages(), listed_points=cfg.NumPoints(), observations=int(rep.num_obs),
                                  poses=int(rep.num_poses), points=int(rep.num_points), repeats=REPEATS, flatten_ms=stat(0), flatten_on_ms=stat(1),
                                  call_total_ms=stat(2), device_ms=stat(3), replay_ms=stat(4))), flush=True)
    finally:
        ses.close()


if __name__ == "__main__":
    main()
