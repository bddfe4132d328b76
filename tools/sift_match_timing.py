"""pp_sift_match_pairs (K17) at three shapes: 8192 x 8192 in a batch of 16 pairs, 8192 x 8192 as a single pair, 2048 x 2048 in a batch of 64 pairs - default
options (cross-check on: both directions).  device_ms is the call's own report (HIP events around the kernels of every internal batch); one warm-up call, then
the median of five.  Beside each: the host's numpy brute force of ONE pair of that shape (the product as a float32 GEMM - exact, every partial sum is an
integer below 2^24 - then the top-2 of both directions by partition; the decision is left out, it is a table look-up per feature; pp_sift_top2 of that
pair must equal it in both directions), and the achieved i8
rate - 2 x 128 x N1 x N2 operations per direction - as a share of the MI355X's dense i8 MFMA peak, taken as twice the ~2.5 PFLOP/s of BF16.
Prints one JSON line per shape.
    PYTHONPATH=. python tools/sift_match_timing.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from privacy_preserving_sfm_amd import synthetic      # noqa: E402
from privacy_preserving_sfm_amd.device import SiftMatcher, sift_match_options      # noqa: E402

WARMUP, REPEATS = 1, 5
I8_PEAK_OPS = 5.0e15
SHAPES = (("8192x8192 batch of 16", 8192, 16), ("8192x8192 single pair", 8192, 1), ("2048x2048 batch of 64", 2048, 64))


def host_brute_force(d1, d2):
    """-> (ms, [(best_j, best, second) of 1 -> 2, the same of 2 -> 1])"""
    t0 = time.perf_counter()
    dists = d1.astype(np.float32) @ d2.astype(np.float32).T
    out = []
    for m in (dists, dists.T):
        top = np.partition(m, m.shape[1] - 2, axis=1)[:, -2:]
        out.append((m.argmax(axis=1), top[:, 1], top[:, 0]))
    return (time.perf_counter() - t0) * 1e3, out


def main():
    rng = np.random.default_rng(0)
    for name, n, num_pairs in SHAPES:
        images = [synthetic.sift_like_descriptors(rng, n) for _ in range(2 * min(num_pairs, 16))]
        pairs = [(a, b) for a in range(0, len(images), 2) for b in range(1, len(images), 2)][:num_pairs]      # distinct pairs, an image in several of them
        m = SiftMatcher(images)
        try:
            rows = []
            for it in range(WARMUP + REPEATS):
                rep, out = m.match_pairs(pairs, sift_match_options())
                if it >= WARMUP:
                    rows.append((rep.device_ms, rep.total_ms))
            a = np.array(rows)
            host_ms, host = host_brute_force(images[0], images[1])
            for (x, y), want in zip(((0, 1), (1, 0)), host):      # the timed kernel computes what the host computes, at this size too
                got = m.top2(x, y)
                assert all(np.array_equal(g, w.astype(np.int32)) for g, w in zip(got, want)), "top-2 differs from the host's at %s" % name
            device_ms = float(np.median(a[:, 0]))
            ops = 2.0 * 128 * n * n * 2 * num_pairs
            print(json.dumps(dict(shape=name, features=n, pairs=num_pairs, batches=int(rep.num_batches), matches=int(rep.num_matches), repeats=REPEATS,
                                  device_ms=dict(median=device_ms, min=float(a[:, 0].min()), max=float(a[:, 0].max())),
                                  device_ms_per_pair=device_ms / num_pairs, total_ms_median=float(np.median(a[:, 1])),
                                  host_numpy_ms_one_pair=host_ms, i8_tops=ops / (device_ms * 1e-3) / 1e12,
                                  share_of_i8_peak=ops / (device_ms * 1e-3) / I8_PEAK_OPS)), flush=True)
        finally:
            m.close()


if __name__ == "__main__":
    main()
