"""From the match lists to the corr_start / corr_line of pp_tracks_desc, both routes in one process, alternating: the host mirror
(feature_matching.build_correspondence_graph, then IncrementalTriangulator.flatten over the dict graph) against the device route
(build_correspondence_graph_on_device = pp_corr_graph_build (K18), then flatten's array path over the FlatCorrespondenceGraph).  Inputs shaped like the
matcher's output - per pair ascending distinct first indices, distinct second indices - over all pairs of the images: 64 images of 2048 lines with 128
matches per pair, and 128 images of 4096 lines with 64 per pair.  One warm-up round, then the median of five; each route's two stages are timed apart, and
the device stage's own report (HIP events / the whole call) is printed beside the wrapper's wall time, which also holds the handle's creation, the
uploads and the download.  Both routes' flatten share the loop over the reconstruction's lines (their coefficients, not the graph).  The two flattened
dicts must be equal.  Prints one JSON line per input.
    PYTHONPATH=. python tools/corr_graph_timing.py"""
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from privacy_preserving_sfm_amd import _capi, feature_matching as fm      # noqa: E402
from privacy_preserving_sfm_amd.bundle_adjustment import Camera, FeatureLine, Image, Reconstruction      # noqa: E402
from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator      # noqa: E402

WARMUP, REPEATS = 1, 5
INPUTS = ((64, 2048, 128), (128, 4096, 64))      # images, lines per image, matches per pair
MIN_NUM_MATCHES = 15


def make_input(num_images, num_lines, per_pair, seed=0):
    rng = np.random.default_rng(seed)
    ids = list(range(1, num_images + 1))
    matches = {}
    for a, b in itertools.combinations(ids, 2):
        first = np.sort(rng.choice(num_lines, per_pair, replace=False))
        matches[(a, b)] = np.stack([first, rng.choice(num_lines, per_pair, replace=False)], axis=1).astype(np.int32)
    rec = Reconstruction()
    rec.cameras[0] = Camera(0, 0, np.ones(_capi.lib().pp_camera_num_params(0)), width=1280, height=960)
    for i in ids:
        rec.images[i] = Image(i, 0, [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0], lines=[FeatureLine([1.0, 0.0, 0.0]) for _ in range(num_lines)])
    return matches, {i: num_lines for i in ids}, rec


def ms_since(t0):
    return (time.perf_counter() - t0) * 1e3


def main():
    for num_images, num_lines, per_pair in INPUTS:
        matches, lines_by_image, rec = make_input(num_images, num_lines, per_pair)
        rows, flats = [], None
        for it in range(WARMUP + REPEATS):
            t0 = time.perf_counter()
            graph, connected = fm.build_correspondence_graph(matches, lines_by_image, MIN_NUM_MATCHES)
            host_build = ms_since(t0)
            t0 = time.perf_counter()
            host_flat, _, _ = IncrementalTriangulator(graph, rec).flatten()
            host_flatten = ms_since(t0)
            reports = []
            t0 = time.perf_counter()
            flat_graph, flat_connected = fm.build_correspondence_graph_on_device(matches, lines_by_image, MIN_NUM_MATCHES, report=reports)
            device_build = ms_since(t0)
            t0 = time.perf_counter()
            device_flat, _, _ = IncrementalTriangulator(flat_graph, rec).flatten()
            device_flatten = ms_since(t0)
            if it >= WARMUP:
                rows.append((host_build, host_flatten, device_build, device_flatten, reports[0].device_ms, reports[0].total_ms))
            flats = (host_flat, device_flat, connected, flat_connected, reports[0])
        host_flat, device_flat, connected, flat_connected, rep = flats
        assert connected == flat_connected and all(np.array_equal(host_flat[k], device_flat[k]) for k in host_flat), "the two routes differ"
        assert rep.num_pairs_replayed == 0
        med = np.median(np.array(rows), axis=0)
        print(json.dumps(dict(images=num_images, lines_per_image=num_lines, pairs=len(matches), matches=int(rep.num_matches_in),
                              accepted=int(rep.num_matches_accepted), repeats=REPEATS,
                              host_ms=dict(build_correspondence_graph=med[0], flatten=med[1], total=med[0] + med[1]),
                              device_route_ms=dict(build_correspondence_graph_on_device=med[2], flatten=med[3], total=med[2] + med[3],
                                                   pp_corr_graph_build_total_ms=med[5], pp_corr_graph_build_device_ms=med[4]),
                              ratio_total=(med[0] + med[1]) / (med[2] + med[3]), ratio_graph_stage=med[0] / med[2])), flush=True)


if __name__ == "__main__":
    main()
