"""Track completion and merging on the 500-image completion scene: device time per complete / merge (HIP events), host replay and wall time, the
conflict replays and fresh-pair launches, candidates evaluated per second - the median of --runs runs after a warm-up, one JSON line.
The comparison figure is the single-thread time of the CPU oracle's inner loop (tests/tracks_reference.py: Python floats around the oracle's C++
WorldToImage) for the same calls on the same scene and machine; it is not the code under test.  Needs a GPU (there is no CPU path)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--track", type=int, default=8)
    ap.add_argument("--seed", type=int, default=11)
    args = ap.parse_args()
    from privacy_preserving_sfm_amd import synthetic
    from privacy_preserving_sfm_amd.device import TracksProblem, tracks_options
    from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator, reconstruction_from_completion_scene
    sc = synthetic.make_completion_scene(args.images, args.points, args.track, seed=args.seed, window=40, split=0.1, noise_point=1e-4, noise_t=1e-5, noise_q=1e-5)
    rec, graph = reconstruction_from_completion_scene(sc)
    flat, _, _ = IncrementalTriangulator(graph, rec).flatten()
    o = tracks_options()
    rows = []
    for run in range(args.runs + 1):      # run 0 warms up (code objects, the pool)
        pb = TracksProblem(flat)
        t0 = time.perf_counter()
        crep, pairs = pb.complete(o)
        t1 = time.perf_counter()
        mrep, merges = pb.merge(o)
        t2 = time.perf_counter()
        pb.close()
        if run:
            rows.append(dict(complete_device_ms=crep.device_ms, complete_replay_ms=crep.replay_ms, complete_wall_ms=(t1 - t0) * 1e3, merge_device_ms=mrep.device_ms,
                             merge_replay_ms=mrep.replay_ms, merge_wall_ms=(t2 - t1) * 1e3))
    med = {k: statistics.median(r[k] for r in rows) for k in rows[0]}
    import oracle_lib
    import tracks_reference as tr
    oracle_lib.build()
    orc = tr.TracksOracle(graph, rec)
    t0 = time.perf_counter()
    nc = orc.CompleteAllTracks(tr.Options())
    t1 = time.perf_counter()
    nm = orc.MergeAllTracks(tr.Options())
    t2 = time.perf_counter()
    assert nc == crep.num_changed and nm == mrep.num_changed and len(orc.merged) == len(merges)
    out = dict(scene="make_completion_scene(%d, %d, %d, seed=%d, window=40, split=0.1)" % (args.images, args.points, args.track, args.seed),
               lines=int(len(flat["line_image"])), correspondences=int(len(flat["corr_line"])), runs=args.runs, completed=int(crep.num_changed),
               merged_observations=int(mrep.num_changed), merges=int(len(merges)), conflict_replays=int(crep.conflict_replays), overflow_points=int(crep.overflow_points),
               fresh_pair_launches=int(mrep.fresh_pair_launches), complete_candidates=int(crep.candidates_evaluated), merge_candidates=int(mrep.candidates_evaluated),
               complete_candidates_per_s=crep.candidates_evaluated / (med["complete_device_ms"] * 1e-3), merge_candidates_per_s=mrep.candidates_evaluated / (med["merge_device_ms"] * 1e-3),
               oracle_complete_ms=(t1 - t0) * 1e3, oracle_merge_ms=(t2 - t1) * 1e3, oracle_tested=len(orc.tested), **med)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
