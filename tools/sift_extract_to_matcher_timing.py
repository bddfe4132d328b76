"""From images to a matcher handle by two routes (K24), on the dense texture of tools/sift_extract_timing.py under the reference's default options:
  A  pp_sift_extract_batch, then pp_sift_create on the descriptors it returned (SiftExtractor.extract_batch + SiftMatcher) - every feature found gets
     an orientation and a descriptor, 640 bytes per feature found come to the host, the kept descriptors go back up
  B  pp_sift_extract_to_matcher (SiftExtractor.extract_to_matcher) - the cut first, the kept features described into the matcher's store
The two alternate in one process on extractors of their own; one warm-up round, then the median of five.  call_ms is the host clock around the whole
route (A: both calls and the arrays between them), device_ms the extractor's events (A's upload and k_sift_prepare are not in it), phase_ms from
separate runs with phase_timings.  Three legs, one JSON line each: a 1600 x 1200 and a 3200 x 2400 image alone, and sixteen 1600 x 1200 images (the
texture under sixteen seeds).
    PYTHONPATH=. python tools/sift_extract_to_matcher_timing.py [--legs small,large,sixteen]"""
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
from privacy_preserving_sfm_amd.device import SiftExtractor, SiftMatcher, sift_extract_options      # noqa: E402
from sift_extract_timing import dense_texture      # noqa: E402

WARMUP, REPEATS = 1, 5
ROWS_PER_IMAGE = 1 << 15      # kept features: max_num_features is 8192 keypoints, the level that crosses it is kept whole


def _phases(values):
    return dict(zip(_capi.SIFT_PHASES, [float(v) for v in values]))


def route_a(ex, ims, options, capacity):
    t0 = time.perf_counter()
    out = ex.extract_batch(ims, options, capacity=capacity)
    matcher = SiftMatcher([desc for _, desc, _ in out])
    ms = (time.perf_counter() - t0) * 1e3
    return ms, ex.last_batch_report, out[0][2], matcher


def route_b(ex, ims, options, capacity):
    t0 = time.perf_counter()
    _, reports, brep, matcher = ex.extract_to_matcher(ims, options, capacity=capacity)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, brep, reports[0], matcher


def leg(name, a, b, ims):
    plain, timed = sift_extract_options(), sift_extract_options(phase_timings=1)
    capacity = len(ims) * ROWS_PER_IMAGE
    rows = {"A": [], "B": []}
    for it in range(WARMUP + REPEATS):
        for key, route, ex in (("A", route_a, a), ("B", route_b, b)):
            ms, brep, first, matcher = route(ex, ims, plain, capacity)
            sizes = matcher.num_features
            matcher.close()
            _, prep, _, matcher = route(ex, ims, timed, capacity)
            matcher.close()
            if it >= WARMUP:
                rows[key].append([ms, brep.device_ms] + list(prep.phase_ms))
            if key == "A":
                found, sizes_a = int(first.num_features_found), sizes
        assert sizes == sizes_a      # both routes keep the same features
    ma, mb = np.median(np.array(rows["A"]), axis=0), np.median(np.array(rows["B"]), axis=0)
    print(json.dumps(dict(leg=name, images=len(ims), width=int(ims[0].shape[1]), height=int(ims[0].shape[0]), features_found_first_image=found,
                          features=int(sum(sizes)), sub_batches=int(brep.num_sub_batches), repeats=REPEATS,
                          batch_then_create=dict(call_ms=ma[0], device_ms=ma[1], phase_ms=_phases(ma[2:])),
                          to_matcher=dict(call_ms=mb[0], device_ms=mb[1], phase_ms=_phases(mb[2:])),
                          call_ratio=ma[0] / mb[0], device_ratio=ma[1] / mb[1])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="small,large,sixteen")
    legs = ap.parse_args().legs.split(",")
    a, b = SiftExtractor(), SiftExtractor()
    if "small" in legs:
        leg("one image", a, b, [dense_texture(1600, 1200)])
    if "large" in legs:
        leg("one image", a, b, [dense_texture(3200, 2400)])
    if "sixteen" in legs:
        leg("sixteen images", a, b, [dense_texture(1600, 1200, seed=k) for k in range(16)])
    a.close()
    b.close()


if __name__ == "__main__":
    main()
