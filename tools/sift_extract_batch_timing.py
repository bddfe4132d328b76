"""SIFT extraction of an image batch (pp_sift_extract_batch, K23) against the single call (pp_sift_extract, K21) on the dense texture of
tools/sift_extract_timing.py, the reference's default options.  Both routes alternate in one process on handles of their own; one warm-up round, then
the median of five.  Three legs, one JSON line each:
  one image    1600 x 1200 and 3200 x 2400: the single call against a batch of one, with phase_timings - phase_ms[4] of the two is the lane-per-feature
               descriptor kernel against the wavefront-per-feature one on the same features (total_ms from runs without phase_timings)
  sixteen      1600 x 1200 images (the texture under sixteen seeds): a loop of single calls against one batch call, by the host clock
  sixty-four   160 x 120 images: the same - the case the waits bound
    PYTHONPATH=. python tools/sift_extract_batch_timing.py [--legs one,sixteen,sixtyfour]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from privacy_preserving_sfm_amd import _capi      # noqa: E402
from privacy_preserving_sfm_amd.device import SiftExtractor, sift_extract_options      # noqa: E402
from sift_extract_timing import dense_texture      # noqa: E402

WARMUP, REPEATS = 1, 5
CAPACITY = 1 << 20      # rows of room for one image, as in sift_extract_timing.py; the legs of many images state theirs per image


def _phases(values):
    return dict(zip(_capi.SIFT_PHASES, [float(v) for v in values]))


def one_image(single, batcher, w, h):
    im = dense_texture(w, h)
    plain, timed = sift_extract_options(), sift_extract_options(phase_timings=1)
    rows = {"single": [], "batch": []}
    for it in range(WARMUP + REPEATS):
        _, _, rep = single.extract(im, plain, capacity=CAPACITY)
        _, _, prep = single.extract(im, timed, capacity=CAPACITY)
        out = batcher.extract_batch([im], plain, capacity=CAPACITY)
        brep = batcher.last_batch_report
        batcher.extract_batch([im], timed, capacity=CAPACITY)
        bprep = batcher.last_batch_report
        if it >= WARMUP:
            rows["single"].append([rep.total_ms, rep.device_ms] + list(prep.phase_ms))
            rows["batch"].append([brep.total_ms, brep.device_ms] + list(bprep.phase_ms))
    s, b = np.median(np.array(rows["single"]), axis=0), np.median(np.array(rows["batch"]), axis=0)
    print(json.dumps(dict(leg="one image", width=w, height=h, features_found=int(rep.num_features_found), features=int(out[0][2].num_features), repeats=REPEATS,
                          single=dict(total_ms=s[0], device_ms=s[1], phase_ms=_phases(s[2:])), batch_of_one=dict(total_ms=b[0], device_ms=b[1], phase_ms=_phases(b[2:])),
                          descriptor_ratio=s[6] / b[6])), flush=True)


def many_images(single, batcher, count, w, h, leg, rows_per_image):
    ims = [dense_texture(w, h, seed=k) for k in range(count)]
    o = sift_extract_options()
    loop, batch, device = [], [], []
    for it in range(WARMUP + REPEATS):
        t0 = time.perf_counter()
        found = 0
        for im in ims:
            found += len(single.extract(im, o, capacity=rows_per_image)[0])
        t1 = time.perf_counter()
        out = batcher.extract_batch(ims, o, capacity=count * rows_per_image)
        t2 = time.perf_counter()
        assert found == sum(len(kp) for kp, _, _ in out)
        if it >= WARMUP:
            loop.append((t1 - t0) * 1e3)
            batch.append((t2 - t1) * 1e3)
            device.append(batcher.last_batch_report.device_ms)
    rep = batcher.last_batch_report
    print(json.dumps(dict(leg=leg, images=count, width=w, height=h, features=int(rep.num_features), sub_batches=int(rep.num_sub_batches),
                          workspace_gb=rep.workspace_bytes / 1e9, repeats=REPEATS, loop_ms=float(np.median(loop)), batch_ms=float(np.median(batch)),
                          batch_device_ms=float(np.median(device)), ratio=float(np.median(loop) / np.median(batch)))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="one,sixteen,sixtyfour")
    legs = ap.parse_args().legs.split(",")
    single, batcher = SiftExtractor(), SiftExtractor()
    if "one" in legs:
        for w, h in ((1600, 1200), (3200, 2400)):
            one_image(single, batcher, w, h)
    if "sixteen" in legs:
        many_images(single, batcher, 16, 1600, 1200, "sixteen images", 1 << 17)
    if "sixtyfour" in legs:
        many_images(single, batcher, 64, 160, 120, "sixty-four images", 1 << 12)
    single.close()
    batcher.close()


if __name__ == "__main__":
    main()
