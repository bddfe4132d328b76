"""Mints tests/golden/init_solvers_golden.json: the four-view, pose and offset solvers of K6 at 50 digits (tests/init_solvers_reference.py), sample by
sample, with the error the CPU oracle makes on each.  Run from the repository root:  python tests/golden/gen_init_solvers_golden.py  (a few minutes; a second
run gives the same bytes).

Sets, 48 samples each unless said otherwise:
  fourview_a   exact bearings of make_scene_2d(4, 120, seed=41), m = 5, the default frames            (default_rng(5), the recipe of test_gpu_init_solvers.py)
  fourview_b   the same scene, bearings with noise 1e-4 (default_rng(2)), m = 10, the default frames  (default_rng(10))
  fourview_c   set a's bearings and samples, the frame triple that generator draws after its 300 samples
  fourview_d   make_scene_2d(4, 120, n_outliers=60, seed=43), m = 5, the default frames: samples with and without a real factorisation
  fourview_e   the 16 decided samples of largest K among 1000 draws (default_rng(50)) from set a's bearings, m = 5, the default frames
  pose2d_*     camera 1 of set a's (exact) and set b's (noise) bearings against the scene's points, m = 3, 6, 21
  planar_*     make_init_scene(120, 40, seed=7) without and with gravity noise 1e-4: the 80 unaligned tracks, poses = Rg_j P_j with t_y zeroed; m = 3, 10
  track        one decided model of set b (the candidate of its first sample that explains the tracks best) on all 120 tracks

Every bearing is a fixed point of the constructors' x / |x| (asserted), so the device and the reference see the same doubles.  The file holds the inputs, and
every double bit for bit (base64 of its bytes).  Per four-view sample: per root the cameras 2 and 3 before the flips and per root and flip1 the fourth camera
(the four candidates that share them have the same fourth camera: asserted at 1e-45); the flips are restated by init_solvers_reference.candidates."""
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import init_solvers_reference as ref  # noqa: E402
from privacy_preserving_sfm_amd import synthetic  # noqa: E402
from privacy_preserving_sfm_amd.initializer import from_two_vectors  # noqa: E402

N = 48
MAX_BYTES = 300 * 1024


def default_frames():
    """the fixed frame triple of pp_fourview2d_default_frames: a splitmix64 stream mapped to [-1, 1), a 2x2 redrawn until |det| > 0.25 (the GPU test
    asserts that the library returns these very doubles)"""
    mask, state, out = (1 << 64) - 1, 0x243F6A8885A308D3, []
    for _ in range(3):
        while True:
            A = []
            for _ in range(4):
                state = (state + 0x9E3779B97F4A7C15) & mask
                z = state
                z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
                z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
                z ^= z >> 31
                A.append(2.0 * (float(z >> 11) * (1.0 / 9007199254740992.0)) - 1.0)
            if abs(A[0] * A[3] - A[1] * A[2]) > 0.25:
                break
        out += A
    return np.array(out)


def unit(x):
    """x / |x| in double, repeated until it is its own fixed point"""
    x = np.array(x, dtype=np.float64)
    for _ in range(20):
        y = x / np.sqrt(x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1])[..., None]
        if np.array_equal(x, y):
            return x
        x = y
    raise AssertionError("a bearing has no fixed point of x / |x|")


def flt(v):
    return float("%.4g" % v)


def f(v):
    return float(v)


# ---- workers (module level: they run in a pool) -------------------------------------------------------------------------------------------------------
def work_fourview(args):
    x, sample, frames = args
    e = ref.fourview2d_minimal(x, sample, frames)
    out = dict(count=e["count"], K=[flt(k) for k in e["K"]], decided=bool(e["decided"]), residual=f(e["residual"]), margins=e["margins"],
               K_tri=e["K_tri"], K_third=e["K_third"], beta_positive=e["beta_positive"])
    if e["count"]:
        out["pre"] = [[[[f(v) for v in r] for r in P] for P in root] for root in e["pre"]]
        out["cam4"] = [[[f(v) for v in c] for c in root] for root in e["cam4"]]
    return out


def work_fourview_k(args):
    x, sample, frames = args
    e = ref.fourview2d_minimal(x, sample, frames, only_k=True)
    return max(e["K"]), bool(e["decided"])


def work_pose2d(args):
    x, X, sample = args
    e = ref.pose2d(x, X, sample)
    return dict(pose=[[f(v) for v in r] for r in e["pose"]], K=flt(e["K"]), decided=bool(e["decided"]), residual=f(e["residual"]))


def work_planar(args):
    scene, sample = args
    e = ref.planar_offsets(scene, sample)
    return dict(offsets=[f(v) for v in e["offsets"]], K=flt(e["K"]), cond=[flt(e["cond_final"]), flt(e["cond_track"])], decided=bool(e["decided"]),
                residual=f(e["residual"]))


def work_track(args):
    cams, x, i = args
    e = ref.fourview2d_track(cams, x, i)
    X = [f(v) for v in e["X"]]
    stored, scale, _ = ref.fourview2d_errors_at(cams, x, X, i)
    return dict(X=X, err=f(e["err"]), K=flt(e["K"]), decided=bool(e["decided"]), err_stored=f(stored), scale=flt(scale))


# ---- sets -----------------------------------------------------------------------------------------------------------------------------------------------
def finish(s, results, rhos, with_result):
    """the per-set figures: oracle_rho per sample, the floor, the two shares, the undecided share (asserted)"""
    dec = [r["decided"] for r in results]
    s["decided"] = "".join("1" if d else "0" for d in dec)
    s["oracle_rho"] = [ref.round_up(r) for r in rhos]
    seen = [s["oracle_rho"][i] for i in range(len(results)) if dec[i] and with_result[i]]
    s["oracle_floor"] = ref.quantile(seen, 0.9)
    s["oracle_median"], s["oracle_max"] = ref.quantile(seen, 0.5), max(seen)
    K = np.array([np.max(r["K"]) for r in results])
    s["share_K"], s["share_sqrtK"] = float(np.mean(ref.EPS * K > 1e-7)), float(np.mean(ref.EPS * np.sqrt(K) > 1e-7))
    s["undecided_share"] = float(np.mean([not d for d in dec]))
    s["max_residual"] = float("%.3g" % max(r["residual"] for r in results))
    assert s["undecided_share"] <= 0.02, (s["name"], s["undecided_share"])
    assert s["max_residual"] <= 1e-40, (s["name"], s["max_residual"])
    print("%-18s n %3d undecided %.3f  oracle rho median %.3g floor %.3g max %.3g  share(K) %.3f share(sqrt K) %.3f  K median %.3g max %.3g" % (
        s["name"], len(results), s["undecided_share"], s["oracle_median"], s["oracle_floor"], s["oracle_max"], s["share_K"], s["share_sqrtK"],
        float(np.median(K)), K.max()))
    return s


def fourview_set(pool, orc, name, xkey, x, samples, fkey, frames, none_undecided):
    results = pool.map(work_fourview, [(x, s, frames) for s in samples])
    rhos = []
    for i, (smp, r) in enumerate(zip(samples, results)):
        e = dict(count=r["count"], K=r["K"], cams=ref.candidates(r["pre"], r["cam4"]) if r["count"] else None)
        o = ref.oracle_fourview_rho(orc, name, i, x, smp, frames, e) if r["decided"] else 0.0
        assert o is not None, (name, i, "the oracle's count differs from the reference's on a decided sample")
        rhos.append(o)
    full = [r for r in results if r["count"]]
    s = dict(name=name, n=len(samples), m=int(samples.shape[1]), x=xkey, frames=fkey, samples=ref.pack(samples, np.uint8),
             full="".join("1" if r["count"] else "0" for r in results), beta_positive="".join("1" if r["beta_positive"] else "0" for r in results), K=[k for r in results for k in r["K"]],
             pre=ref.pack([r["pre"] for r in full]), cam4=ref.pack([r["cam4"] for r in full]))
    finish(s, results, rhos, [r["count"] == 16 for r in results])
    if none_undecided:
        assert s["undecided_share"] == 0.0, name
    return s


def pose2d_set(pool, orc, name, xkey, x, X, samples):
    results = pool.map(work_pose2d, [(x, X, s) for s in samples])
    rhos = [ref.oracle_pose2d_rho(orc, name, i, x, X, smp, dict(pose=r["pose"], K=r["K"])) if r["decided"] else 0.0
            for i, (smp, r) in enumerate(zip(samples, results))]
    s = dict(name=name, n=len(samples), m=int(samples.shape[1]), x=xkey, X="points", samples=ref.pack(samples, np.uint8), K=[r["K"] for r in results],
             pose=ref.pack([r["pose"] for r in results]))
    return finish(s, results, rhos, [True] * len(results))


def planar_set(pool, orc, name, key, scene, samples):
    results = pool.map(work_planar, [(scene, s) for s in samples])
    rhos = [ref.oracle_planar_rho(orc, name, i, scene, smp, dict(offsets=r["offsets"], K=r["K"])) if r["decided"] else 0.0
            for i, (smp, r) in enumerate(zip(samples, results))]
    s = dict(name=name, n=len(samples), m=int(samples.shape[1]), scene=key, samples=ref.pack(samples, np.uint8), K=[r["K"] for r in results],
             cond=[c for r in results for c in r["cond"]], offsets=ref.pack([r["offsets"] for r in results]))
    finish(s, results, rhos, [True] * len(results))
    # the normaliser holds if the oracle's normalised errors stay within three decades between their 10 % and 90 % quantiles
    seen = [rh for rh, r in zip(s["oracle_rho"], results) if r["decided"]]
    s["spread"] = float("%.3g" % (ref.quantile(seen, 0.9) / ref.quantile(seen, 0.1)))
    assert s["spread"] <= 1e3, (name, s["spread"])
    return s


def planar_scene(gravity_noise):
    sc = synthetic.make_init_scene(120, 40, seed=7, gravity_noise=gravity_noise)
    keep = ~np.asarray(sc["aligned"][0])
    Rg = np.array([from_two_vectors(sc["gravity"][j], [0.0, 1.0, 0.0]) for j in range(4)])
    poses = np.array([Rg[j] @ sc["cams"][j] for j in range(4)])
    t_gt = poses[1:, 1, 3].copy()
    poses[1:, 1, 3] = 0.0
    return dict(poses=poses, lines=np.array([np.asarray(sc["lines"][j])[keep] for j in range(4)]), Rg=Rg), t_gt


def main():
    import oracle_lib
    oracle_lib.build()
    oracle_lib.lib()
    frames = default_frames()
    sc = synthetic.make_scene_2d(4, 120, seed=41)
    xa = unit(sc["x"])
    xb = unit(sc["x"] + np.random.default_rng(2).normal(0, 1e-4, sc["x"].shape))
    scd = synthetic.make_scene_2d(4, 120, n_outliers=60, seed=43)
    xd = unit(scd["x"])
    rng5 = np.random.default_rng(5)
    s5 = np.stack([rng5.choice(120, 5, replace=False) for _ in range(300)])
    frames_c = rng5.uniform(-1, 1, 12)
    rng10 = np.random.default_rng(10)
    s10 = np.stack([rng10.choice(120, 10, replace=False) for _ in range(300)])
    rng50 = np.random.default_rng(50)
    s1000 = np.stack([rng50.choice(120, 5, replace=False) for _ in range(1000)])
    inputs = dict(frames_default=frames, frames_c=frames_c, x_a=xa, x_b=xb, x_d=xd, points=sc["X"])
    sets = []
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        sets.append(fourview_set(pool, oracle_lib, "fourview_a", "x_a", xa, s5[:N], "frames_default", frames, True))
        sets.append(fourview_set(pool, oracle_lib, "fourview_b", "x_b", xb, s10[:N], "frames_default", frames, True))
        sets.append(fourview_set(pool, oracle_lib, "fourview_c", "x_a", xa, s5[:N], "frames_c", frames_c, False))
        d = fourview_set(pool, oracle_lib, "fourview_d", "x_d", xd, s5[:N], "frames_default", frames, False)
        for ch in "01":                                # both outcomes of the discriminant, each on a twentieth of the set at least
            assert d["full"].count(ch) >= 0.05 * N, ("fourview_d", d["full"])
        sets.append(d)
        ks = pool.map(work_fourview_k, [(xa, s, frames) for s in s1000])
        hard = sorted((i for i in range(1000) if ks[i][1]), key=lambda i: (-ks[i][0], i))[:16]
        sets.append(fourview_set(pool, oracle_lib, "fourview_e", "x_a", xa, s1000[hard], "frames_default", frames, True))
        for kind, key, x in (("exact", "x_a", xa), ("noise", "x_b", xb)):
            for m in (3, 6, 21):
                rng = np.random.default_rng(100 + m)
                smp = np.stack([rng.choice(120, m, replace=False) for _ in range(N)])
                sets.append(pose2d_set(pool, oracle_lib, "pose2d_%s_m%d" % (kind, m), key, x[1], sc["X"], smp))
        for kind, noise in (("exact", 0.0), ("noise", 1e-4)):
            scene, t_gt = planar_scene(noise)
            for k, v in scene.items():
                inputs["planar_%s_%s" % (kind, k)] = v
            for m in (3, 10):
                rng = np.random.default_rng(200 + m)
                smp = np.stack([rng.choice(scene["lines"].shape[1], m, replace=False) for _ in range(N)])
                s = planar_set(pool, oracle_lib, "planar_%s_m%d" % (kind, m), "planar_%s" % kind, scene, smp)
                if noise == 0.0:                       # exact data: the reference returns the offsets the scene was made with
                    assert np.abs(ref.unpack(s["offsets"], (N, 3)) - t_gt).max() < 1e-9, s["name"]
                sets.append(s)
        # the track set: of set b's first sample the candidate with the smallest summed error over all tracks, its cameras as the file holds them
        b = ref.decode_set(sets[1], inputs)
        first = int(np.argmax(b["decided"] & (b["count"] == 16)))
        cams = min(b["cams"][first], key=lambda c: oracle_lib.fourview2d_score(c, xb, 1e-3)[0])
        results = pool.map(work_track, [(cams, xb, i) for i in range(120)])
    tracks = [dict(X=r["X"], err=r["err"], K=r["K"]) for r in results]
    rhos = ref.oracle_track_rho(oracle_lib, ref.TRACK_SET, cams, xb, tracks)
    for r in results:
        r["residual"] = 0.0
    t = dict(name=ref.TRACK_SET, n=120, x="x_b", cams=ref.pack(cams), K=[r["K"] for r in results], X=ref.pack([r["X"] for r in results]),
             err=ref.pack([r["err"] for r in results]), err_stored=ref.pack([r["err_stored"] for r in results]), scale=[r["scale"] for r in results])
    sets.append(finish(t, results, [rh if r["decided"] else 0.0 for rh, r in zip(rhos, results)], [True] * 120))
    out = os.path.join(HERE, "init_solvers_golden.json")
    doc = {"generator": "tests/golden/gen_init_solvers_golden.py", "digits": 50, "decided_rel": ref.DECIDED_REL, "decided_cond": ref.DECIDED_COND,
           "oracle_draws": ref.ORACLE_DRAWS, "inputs": {k: dict(shape=list(np.shape(v)), data=ref.pack(v)) for k, v in inputs.items()}, "sets": sets}
    with open(out, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
    size = os.path.getsize(out)
    print("%s: %d bytes" % (out, size))
    assert size <= MAX_BYTES, size


if __name__ == "__main__":
    main()
