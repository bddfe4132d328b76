"""SIFT extraction on the device (pp_sift_extract, K21) at the sizes a user runs: 1600 x 1200 and 3200 x 2400 (the reference's max_image_size) on a
dense synthetic texture (band-passed noise: blobs of every size), the reference's default options (first_octave -1: the first octave is 6400 x 4800 for
the larger image).  One warm-up run, then the median of five, per size:
  total_ms      the call by the host clock: uploads, kernels, the waits for the counts, the host's share (pow, sin, cos, the level containers), downloads
  device_ms     HIP events over everything on the stream
  phase_ms      pyramid, detection, gradient, orientation, descriptor, from a second set of runs with phase_timings (the stream is drained between the
                phases there, so their sum exceeds device_ms of the untimed runs a little)
  pyramid_bytes the bytes the pyramid needs, from the shapes: the float32 read and the float32 write of each of the two passes of every smoothing, the
                doubling or halving in front of an octave, and the DoG (two reads, one write); pyramid_gb_s = those over the pyramid's phase time,
                share_of_hbm = that over 6.29 TB/s (the measured copy rate of an MI355X; the specification says 8 TB/s)
Prints one JSON line per size.
    PYTHONPATH=. python tools/sift_extract_timing.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from privacy_preserving_sfm_amd import _capi      # noqa: E402
from privacy_preserving_sfm_amd.device import SiftExtractor, sift_extract_options      # noqa: E402

WARMUP, REPEATS = 1, 5
SIZES = ((1600, 1200), (3200, 2400))
HBM_MEASURED_TB_S = 6.29
CAPACITY = 1 << 20      # rows of room: the level that crosses max_num_features is kept whole, and on this texture it is a fine one


def _box(a, r):
    """the mean over (2 r + 1)^2 windows, the ends clamped"""
    for axis in (0, 1):
        p = np.concatenate([np.repeat(a.take([0], axis), r + 1, axis), a, np.repeat(a.take([-1], axis), r, axis)], axis)
        c = np.cumsum(p, axis=axis)
        a = (c.take(range(2 * r + 1, c.shape[axis]), axis) - c.take(range(0, c.shape[axis] - 2 * r - 1), axis)) / (2 * r + 1)
    return a


def dense_texture(w, h, seed=0):
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(h, w))
    im = sum(scale * (_box(_box(n, r), r) - _box(_box(n, 2 * r), 2 * r)) * r for r, scale in ((1, 1.0), (2, 1.0), (4, 1.2), (8, 1.5)))
    im = (im - im.mean()) / im.std()
    return np.clip(np.rint(128 + 48 * im), 0, 255).astype(np.uint8)


def pyramid_bytes(w, h, o):
    """float32 bytes the pyramid kernels read and write, from the shapes"""
    S, total = int(o.octave_resolution), 4 * w * h + w * h      # the bytes in, the floats out
    ow, oh = (w << -o.first_octave, h << -o.first_octave) if o.first_octave < 0 else (w >> o.first_octave, h >> o.first_octave)
    total += 4 * (w * h + 2 * w * h) + 4 * (2 * w * h + 4 * w * h) if o.first_octave == -1 else 8 * ow * oh
    for q in range(int(o.num_octaves)):
        lev = ow * oh
        smooths = (S + 2) + (1 if q == 0 else 0)
        total += smooths * 2 * 8 * lev + (S + 2) * 12 * lev
        if q:
            total += 8 * lev
        ow, oh = ow >> 1, oh >> 1
    return total


def main():
    ex = SiftExtractor()
    for w, h in SIZES:
        im = dense_texture(w, h)
        plain, timed = sift_extract_options(), sift_extract_options(phase_timings=1)
        rows, phases, rep = [], [], None
        for it in range(WARMUP + REPEATS):
            t0 = time.perf_counter()
            kp, desc, rep = ex.extract(im, plain, capacity=CAPACITY)
            wall = (time.perf_counter() - t0) * 1e3
            _, _, prep = ex.extract(im, timed, capacity=CAPACITY)
            if it >= WARMUP:
                rows.append((wall, rep.total_ms, rep.device_ms))
                phases.append(list(prep.phase_ms))
        med, ph = np.median(np.array(rows), axis=0), np.median(np.array(phases), axis=0)
        nbytes = pyramid_bytes(w, h, plain)
        gb_s = nbytes / (ph[0] * 1e-3) / 1e9
        print(json.dumps(dict(width=w, height=h, features=int(rep.num_features), keypoints=int(rep.num_keypoints), features_found=int(rep.num_features_found),
                              candidates=[int(rep.octave_candidates[q]) for q in range(rep.num_octaves)], repeats=REPEATS,
                              wrapper_ms=med[0], total_ms=med[1], device_ms=med[2], phase_ms=dict(zip(_capi.SIFT_PHASES, [float(v) for v in ph])),
                              pyramid_bytes=int(nbytes), pyramid_gb_s=gb_s, share_of_hbm=gb_s / (HBM_MEASURED_TB_S * 1e3))), flush=True)
    ex.close()


if __name__ == "__main__":
    main()
