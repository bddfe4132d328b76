"""Image-pair selection (K20), both routes in one process, alternating: the numpy mirrors of feature_matching.py (spatial_pair_positions,
transitive_pair_positions) against the device route (device.PairSelector = pp_pairs_spatial / pp_pairs_transitive) over location indices / image
positions, so that neither side pays for Python tuples.  Spatial: 20 000 locations scattered over a square kilometre, max_num_neighbors = 50,
max_distance = 100.  Transitive: one iteration over 20 000 images of mean degree 50, the edges between images that are close in a shuffled ring, as a
first round of spatial matches would leave them.  One warm-up round, then the median of five.  The device's own report (the kernels by HIP events / the
whole call with checks, uploads and the two waits for a count) is printed beside the wrapper's wall time, which also holds the download of the result and
the numpy around the call.  The two results must be equal, the distances bit for bit.  Prints one JSON line per selection.
    PYTHONPATH=. python tools/pair_selection_timing.py [--locations 20000] [--images 20000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from privacy_preserving_sfm_amd import feature_matching as fm      # noqa: E402
from privacy_preserving_sfm_amd.device import PairSelector          # noqa: E402

WARMUP, REPEATS = 1, 5


def ms_since(t0):
    return (time.perf_counter() - t0) * 1e3


def spatial_input(m, seed=0):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.concatenate([rng.uniform(0, 1000, (m, 2)), rng.uniform(0, 30, (m, 1))], axis=1), dtype=np.float32)


def transitive_input(n, mean_degree, seed=0):
    rng = np.random.default_rng(seed)
    ring = rng.permutation(n)
    a = rng.integers(0, n, n * mean_degree // 2)
    b = (a + rng.integers(1, 2 * mean_degree, a.shape[0])) % n
    pairs = np.unique(np.sort(np.stack([ring[a], ring[b]], axis=1), axis=1), axis=0)
    return np.ascontiguousarray(pairs, dtype=np.int32)


def time_spatial(selector, m, knn, max_distance):
    xyz = spatial_input(m)
    rows, last = [], None
    for it in range(WARMUP + REPEATS):
        t0 = time.perf_counter()
        host_pairs, host_dist = fm.spatial_pair_positions(xyz, knn, max_distance)
        host = ms_since(t0)
        t0 = time.perf_counter()
        rep, pairs, dist = selector.spatial(xyz, knn, max_distance)
        device = ms_since(t0)
        if it >= WARMUP:
            rows.append((host, device, rep.device_ms, rep.total_ms))
        last = (host_pairs, host_dist, pairs, dist, rep)
    host_pairs, host_dist, pairs, dist, rep = last
    assert np.array_equal(host_pairs, pairs) and np.array_equal(host_dist.view(np.uint32), dist.view(np.uint32)), "the two routes differ"
    med = np.median(np.array(rows), axis=0)
    return dict(selection="spatial", locations=m, max_num_neighbors=knn, max_distance=max_distance, pairs=int(rep.num_pairs), repeats=REPEATS,
                host_mirror_ms=med[0], device_route_ms=med[1], pp_pairs_spatial_total_ms=med[3], pp_pairs_spatial_device_ms=med[2],
                host_share_of_device_route_ms=med[1] - med[2], ratio=med[0] / med[1])


def time_transitive(selector, n, mean_degree):
    matched = transitive_input(n, mean_degree)
    tried = np.zeros((0, 2), dtype=np.int32)
    rows, last = [], None
    for it in range(WARMUP + REPEATS):
        t0 = time.perf_counter()
        host_pairs = fm.transitive_pair_positions(n, matched, tried)
        host = ms_since(t0)
        t0 = time.perf_counter()
        rep, pairs = selector.transitive(n, matched, tried)
        device = ms_since(t0)
        if it >= WARMUP:
            rows.append((host, device, rep.device_ms, rep.total_ms))
        last = (host_pairs, pairs, rep)
    host_pairs, pairs, rep = last
    assert np.array_equal(host_pairs, pairs), "the two routes differ"
    med = np.median(np.array(rows), axis=0)
    return dict(selection="transitive", images=n, matched_pairs=len(matched), mean_degree=2.0 * len(matched) / n, candidates_visited=int(rep.num_candidates),
                pairs=int(rep.num_pairs), repeats=REPEATS, host_mirror_ms=med[0], device_route_ms=med[1], pp_pairs_transitive_total_ms=med[3],
                pp_pairs_transitive_device_ms=med[2], host_share_of_device_route_ms=med[1] - med[2], ratio=med[0] / med[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--locations", type=int, default=20000)
    ap.add_argument("--images", type=int, default=20000)
    ap.add_argument("--max-num-neighbors", type=int, default=50)
    ap.add_argument("--mean-degree", type=int, default=50)
    args = ap.parse_args()
    selector = PairSelector()
    try:
        print(json.dumps(time_spatial(selector, args.locations, args.max_num_neighbors, 100.0)), flush=True)
        print(json.dumps(time_transitive(selector, args.images, args.mean_degree)), flush=True)
    finally:
        selector.close()


if __name__ == "__main__":
    main()
