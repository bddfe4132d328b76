"""Records tests/golden/image_orders.json: for every case of corpus() the info[8] of pp_ba_plan_ordering and the length and FNV-1a digest of old_of_new, as
the library at hand computes them (privacy_preserving_sfm_amd.device.plan_ordering).  The fixture was recorded BEFORE the ordering moved out of
csrc/image_ordering.hip into csrc/image_ordering.hpp; tests/test_image_orders_golden.py re-runs the corpus and asserts equality, so the orders, the
tile counts and the chain plans are what they were.  Run from the repository root:  python tests/golden/gen_image_orders.py"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "image_orders.json")
SWITCHES = ("PPSFM_BA_ORDERING", "PPSFM_BA_GRAPH_ND", "PPSFM_BA_INTR_LAYOUT", "PPSFM_BA_LINEAR_SOLVER", "PPSFM_BA_SPARSE")


def _scenes():
    """name -> a function that builds the scene (built once per name, shared by the cases that differ in their switches only)"""
    from privacy_preserving_sfm_amd import synthetic
    from privacy_preserving_sfm_amd.device import covisibility

    def seq(images, window, loop=False, track=6, **kw):      # tests/test_image_ordering.py _scene
        return synthetic.make_ba_scene(images, 20 * images, track, seed=0xC0FFEE + images, model=2, window=window, loop=loop, **kw)

    def shuffled(sc, seed):
        return synthetic.shuffle_image_ids(sc, seed=seed)[0]

    def some_constant(sc, every=10, first=3):      # about a tenth of the poses constant, beside the gauge image
        pc = np.array(sc["pose_const"], dtype=np.uint8)
        pc[first::every] = 1
        return dict(sc, pose_const=pc)

    def private(sc, mask):
        return dict(sc, camera_const_mask=np.full(len(sc["camera_model"]), mask, dtype=np.uint16))

    def clustered(topology, clusters):
        sc = synthetic.make_ba_scene(500, 10000, 6, seed=0xC0FFEE + 11 * clusters, model=2, clusters=clusters, bridge=4, topology=topology)
        return shuffled(sc, 5)

    def half_with_matrix(sc):      # half of the observations + the full matrix: a shard of a point-sharded group
        keep = sc["obs_point"] % 2 == 0
        half = dict(sc, covisibility=covisibility(sc))
        for k in ("lines", "obs_pose", "obs_point"):
            half[k] = np.ascontiguousarray(sc[k][keep])
        return half

    def unsorted(sc, seed):      # observations in random order: the by-point grouping is a counting sort, not the caller's arrays
        perm = np.random.default_rng(seed).permutation(len(sc["obs_pose"]))
        return dict(sc, **{k: np.ascontiguousarray(np.asarray(sc[k])[perm]) for k in ("lines", "obs_pose", "obs_point")})

    def twice(sc):      # image 7 sees point 0 a second time: a bit on the diagonal of the graph
        return dict(sc, lines=np.concatenate([sc["lines"], sc["lines"][:1]]), obs_pose=np.append(sc["obs_pose"], sc["obs_pose"][0]).astype(np.int32),
                    obs_point=np.append(sc["obs_point"], 0).astype(np.int32))

    s = {}
    s["seq300"] = lambda: seq(300, 20)
    s["seq300_shuffled"] = lambda: shuffled(seq(300, 20), 4)
    s["seq500_shuffled"] = lambda: shuffled(seq(500, 40), 7)
    s["ring500"] = lambda: seq(500, 40, True)
    s["seq1000_shuffled"] = lambda: shuffled(seq(1000, 10), 7)
    s["dense120"] = lambda: synthetic.make_ba_scene(120, 3000, 8, seed=5, model=2)
    s["seq300_shared_intrinsics"] = lambda: dict(seq(300, 20, num_intrinsics=1), camera_const_mask=np.array([0b0110], dtype=np.uint16))
    s["seq1100"] = lambda: seq(1100, 20, track=4)
    s["seq1400"] = lambda: seq(1400, 10, track=4)
    for topology, clusters in (("star", 5), ("chain", 4), ("star", 8)):
        s["%s%d" % (topology, clusters)] = lambda t=topology, c=clusters: clustered(t, c)
    s["seq500_private8"] = lambda: private(seq(500, 40, num_intrinsics=500), 0b0110)
    s["seq500_private_odd"] = lambda: private(seq(500, 40, num_intrinsics=500), 0b1110)
    s["seq300_matrix"] = lambda: half_with_matrix(shuffled(seq(300, 20), 4))
    s["seq300_constant"] = lambda: some_constant(seq(300, 20))
    s["seq300_constant_shuffled"] = lambda: shuffled(some_constant(seq(300, 20)), 9)
    s["seq300_constant_private8"] = lambda: private(some_constant(seq(300, 20, num_intrinsics=300)), 0b0110)
    s["seq300_constant_matrix"] = lambda: half_with_matrix(some_constant(seq(300, 20)))
    s["seq300_unsorted"] = lambda: unsorted(seq(300, 20), 3)
    s["seq300_twice"] = lambda: twice(seq(300, 20))
    s["seq70"] = lambda: seq(70, 10)      # 7 block columns: below the candidate threshold
    s["seq75"] = lambda: seq(75, 10)      # 8 block columns: just above it
    return s


def corpus():
    """[(case name, scene name, environment switches, keyword arguments of plan_ordering)]"""
    out = []

    def add(scene, env=None, **kw):
        tags = ["%s=%s" % (k[len("PPSFM_BA_"):].lower(), v) for k, v in sorted((env or {}).items())] + ["%s=%s" % kv for kv in sorted(kw.items())]
        out.append(("/".join([scene] + tags), scene, env or {}, kw))

    for scene in ("seq300", "seq300_shuffled", "seq500_shuffled", "ring500", "seq1000_shuffled", "dense120", "seq300_shared_intrinsics", "star5", "chain4",
                  "star8", "seq500_private8", "seq500_private_odd", "seq300_matrix", "seq300_constant", "seq300_constant_shuffled",
                  "seq300_constant_private8", "seq300_constant_matrix", "seq300_unsorted", "seq300_twice", "seq70", "seq75"):
        add(scene)
    add("seq300", ordering=1)      # PP_ORDERING_NATURAL of the descriptor
    for order in ("natural", "rcm", "band"):
        for scene in ("seq300", "star5", "dense120", "seq300_constant"):
            add(scene, {"PPSFM_BA_ORDERING": order})
    add("seq70", {"PPSFM_BA_ORDERING": "rcm"})      # forced below the threshold
    for nd in ("0", "1"):
        for scene in ("seq300", "ring500", "star5", "chain4", "seq500_private8"):
            add(scene, {"PPSFM_BA_GRAPH_ND": nd})
    for scene in ("seq500_private8", "seq500_private_odd", "seq300_constant_private8"):
        add(scene, {"PPSFM_BA_INTR_LAYOUT": "tail"})
    add("seq300", {"PPSFM_BA_SPARSE": "0"})
    add("seq1100")      # AUTO: the iterative solver above 1000 images
    add("seq1100", linear_solver=1)
    add("seq1100", {"PPSFM_BA_LINEAR_SOLVER": "direct"})
    add("seq500_private8", {"PPSFM_BA_LINEAR_SOLVER": "iterative"})
    add("seq1400", linear_solver=1)      # 132 block columns under the direct solver: a band, no dissection
    return out


def fnv1a(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a, dtype=np.int32).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


INFO_KEYS = ("reordered", "nnz_natural", "nnz_used", "chains", "chain_steps", "block_columns", "block_sparse", "intrinsics_columns")


def run(cases=None, seconds=None):
    """name -> {"info": [8 ints], "old_of_new": [length, digest]} for the cases of corpus() (all of them, or those named); `seconds` receives the time
    plan_ordering took per case"""
    from privacy_preserving_sfm_amd.device import plan_ordering
    build, scenes, out = _scenes(), {}, {}
    for name, scene, env, kw in corpus():
        if cases is not None and name not in cases:
            continue
        if scene not in scenes:
            scenes[scene] = build[scene]()
        saved = {k: os.environ.pop(k, None) for k in SWITCHES}
        os.environ.update(env)
        try:
            t0 = time.perf_counter()
            oon, info = plan_ordering(scenes[scene], **kw)
            if seconds is not None:
                seconds[name] = time.perf_counter() - t0
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        out[name] = {"info": [int(info[k]) for k in INFO_KEYS], "old_of_new": [int(len(oon)), fnv1a(oon)]}
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    seconds = {}
    golden = run(seconds=seconds)
    with open(GOLDEN, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")
    for name, s in sorted(seconds.items(), key=lambda kv: -kv[1])[:8]:
        print("%-60s %.3f s  %s" % (name, s, golden[name]["info"]))
    print("%d cases -> %s" % (len(golden), GOLDEN))
