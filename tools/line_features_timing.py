"""From keypoints to line features, both routes in one process, alternating: the numpy host mirror (feature_extraction.generate_line_features) against
the device route (generate_line_features_on_device = pp_line_features_from_keypoints, K19).  128 images of 4096 keypoints uniform over 1280 x 960, every
image with a gravity direction and aligned_line_ratio 0.5, once with SIMPLE_RADIAL cameras (two Newton iterations per keypoint) and once with
THIN_PRISM_FISHEYE; one camera per image.  One warm-up round, then the median of five.  Both routes are timed to their arrays (fill=False: the Python
list of FeatureLine objects either route can build on top is the same loop over the same arrays); the device call's own report (HIP events over the two
kernels) is printed beside the wrapper's wall time, which also holds the uploads, the download of the lines and the flag count.  The two routes must
agree: flags and directions exactly, lines to 1e-6.  Prints one JSON line per camera model.
    PYTHONPATH=. python tools/line_features_timing.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from privacy_preserving_sfm_amd import feature_extraction as fe, synthetic      # noqa: E402
from privacy_preserving_sfm_amd.bundle_adjustment import Camera, Image      # noqa: E402

WARMUP, REPEATS = 1, 5
NUM_IMAGES, NUM_KEYPOINTS = 128, 4096
MODELS = ((2, "SIMPLE_RADIAL"), (10, "THIN_PRISM_FISHEYE"))


def make_input(model, seed=0):
    rng = np.random.default_rng(seed)
    images, cameras, kps = [], {}, {}
    for k in range(NUM_IMAGES):
        cameras[k] = Camera(k, model, synthetic.default_intrinsics(model)[:synthetic.NUM_PARAMS[model]], 1280, 960)
        g = rng.normal(size=3)
        images.append(Image(k + 1, k, [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0], gravity=g / np.linalg.norm(g)))
        kps[k + 1] = np.stack([rng.uniform(0, 1280, NUM_KEYPOINTS), rng.uniform(0, 960, NUM_KEYPOINTS)], axis=1).astype(np.float32)
    return images, cameras, kps


def ms_since(t0):
    return (time.perf_counter() - t0) * 1e3


def main():
    for model, name in MODELS:
        images, cameras, kps = make_input(model)
        rows, last = [], None
        for it in range(WARMUP + REPEATS):
            t0 = time.perf_counter()
            host = fe.generate_line_features(images, cameras, kps, 0.5, seed=1, fill=False)
            host_ms = ms_since(t0)
            t0 = time.perf_counter()
            dev = fe.generate_line_features_on_device(images, cameras, kps, 0.5, seed=1, fill=False)
            device_ms = ms_since(t0)
            if it >= WARMUP:
                rows.append((host_ms, device_ms, dev["device_ms"]))
            last = (host, dev)
        host, dev = last
        worst = 0.0
        for im in images:
            k = im.image_id
            assert np.array_equal(host["aligned"][k], dev["aligned"][k]) and np.array_equal(host["dirs"][k], dev["dirs"][k]), "the two routes differ"
            use = host["head"][k] >= 0.05
            worst = max(worst, float(np.abs(host["lines"][k][use] - dev["lines"][k][use]).max()))
        assert worst <= 1e-6, "the two routes differ by %g" % worst
        med = np.median(np.array(rows), axis=0)
        print(json.dumps(dict(model=name, images=NUM_IMAGES, keypoints_per_image=NUM_KEYPOINTS, lines=int(dev["num_lines"]), aligned=int(dev["num_aligned"]),
                              repeats=REPEATS, host_mirror_ms=med[0], device_route_ms=med[1], device_kernels_ms=med[2], ratio=med[0] / med[1],
                              largest_line_difference=worst)), flush=True)


if __name__ == "__main__":
    main()
