#!/usr/bin/env python3
"""Generate tests/golden/triangulation_golden.json.

The robust track triangulation (reference estimators/triangulation.cc:55-149) on small sets of tracks, computed by tests/triangulation_reference.py in
50-digit mpmath: per track the success flag, the trial count, the inlier mask, the point rounded to double and the MARGIN - the smallest separation of
any comparison on the reference's trajectory (see that module).  The inputs are written out as arrays, not as seeds.  The oracle
(tests/test_triangulation_reference.py) and the HIP kernel (tests/test_gpu_triangulation_exact.py) are both held to these numbers: exactly on the tracks
whose margin is at least 1e-6, by invariants on the others.

Sets (see main): `grid` - 129 tracks of lengths 0..12 around the workgroup size of 64; `models` - every camera model alone and all in one call, strong
distortion, projections cut by the image size, two views inside the scene with points behind them; `options` - the RANSAC options swept over tracks
with 40 % outliers, and an image of one pixel that empties every support; `degenerate` - repeated observations, three planes along one direction,
exact fits of three inliers: these are meant to be undecided.

In `grid`, `models` and `options` at most 2 % of the tracks may be undecided; the script asserts it and prints the share.  Per set and residual type
it also runs the CPU oracle and records oracle_xyz_err, the largest |xyz_oracle - xyz_reference|_inf over the decided tracks on which the masks agree.

Run from the repo root (minutes, CPU only):  python tests/golden/gen_triangulation_golden.py
"""
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import triangulation_reference as ref  # noqa: E402

UNDECIDED_CAP = 0.02
F, CX, CY = 1000.0, 640.0, 480.0
FY = 1020.0
# distortion strong enough that every single term moves some projection by more than a pixel (asserted in check_distortion)
INTRINSICS = {
    0: [F, CX, CY], 1: [F, FY, CX, CY], 2: [F, CX, CY, 0.12], 3: [F, CX, CY, 0.12, -0.6],
    4: [F, FY, CX, CY, 0.12, -0.6, 0.012, -0.009],
    5: [F, FY, CX, CY, 0.1, -0.5, 1.5, -20.0],
    6: [F, FY, CX, CY, 0.12, -0.6, 0.012, -0.009, 2.0, 0.05, -0.3, 4.0],
    7: [F, FY, CX, CY, 0.9], 8: [F, CX, CY, 0.1], 9: [F, CX, CY, 0.1, -0.5],
    10: [F, FY, CX, CY, 0.1, -0.5, 0.012, -0.009, 1.5, -20.0, 0.05, -0.04],
}
NUM_FOCAL = (1, 2, 1, 1, 2, 2, 2, 2, 1, 1, 2)
MAX_ERROR = {0: 2e-3, 1: 2.0}
NEAR_OUTLIER_UNIT = 2e-3                               # MAX_ERROR on the normalised plane (2 px at f = 1000)


def intr_row(model, values=None):
    p = np.zeros(12)
    v = INTRINSICS[model] if values is None else values
    p[: len(v)] = v
    return p


def look_at(c, target):
    z = (target - c) / np.linalg.norm(target - c)
    x = np.cross([0, 1.0, 0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.hstack([R, (-R @ c)[:, None]])


def make_views(rng, num_circle, num_inside=0):
    """views on a circle of radius 4 looking at the origin, then `num_inside` views inside the scene, which have part of the points behind them"""
    P, centers = [], []
    for v in range(num_circle):
        ang = 2 * np.pi * v / num_circle + rng.normal(0, 0.05)
        c = np.array([4.0 * np.cos(ang), rng.normal(0, 0.3), 4.0 * np.sin(ang)])
        P.append(look_at(c, np.zeros(3)))
        centers.append(c)
    for v in range(num_inside):
        c = rng.uniform(-0.3, 0.3, 3)
        ang = rng.uniform(0, 2 * np.pi)
        P.append(look_at(c, c + np.array([np.cos(ang), 0.1 * rng.normal(), np.sin(ang)])))
        centers.append(c)
    return np.round(np.array(P), 9), np.round(np.array(centers), 9)      # nine decimals: what the JSON holds


def observe(rng, P, X, noise, outlier):
    z = P[:, :3] @ X + P[:, 3]
    xh = np.array([z[0] / z[2], z[1] / z[2], 1.0])
    xh[:2] += rng.normal(0, noise, 2)
    if outlier == "far" or (outlier and rng.random() < 0.5):      # a far outlier: anywhere in the image
        xh[:2] = rng.uniform(-0.4, 0.4, 2)
    elif outlier:                                      # a near one: up to 2.5 thresholds off, so that residuals fall on both sides of max_residual
        ang = rng.uniform(0, 2 * np.pi)
        xh[:2] += rng.uniform(0.5, 2.5) * NEAR_OUTLIER_UNIT * np.array([np.cos(ang), np.sin(ang)])
    l = np.cross(xh, rng.uniform(-1, 1, 3))
    return l / np.linalg.norm(l[:2])


def quantise(lines):
    """line coefficients as whole multiples of 1e-6, the form the JSON holds: 5e-4 px at f = 1000, a 4000th of the threshold"""
    return np.rint(np.asarray(lines) * 1e6) / 1e6


def threshold_line(rng, view, X, max_error):
    """A line whose PIXEL residual at the true point X is max_error^2 times 1 -+ (0.8 to 4 %): it is an inlier or not by what the camera model's
    distortion does to a step across the line, so a dropped term of the model flips it.  The line of a true observation, moved along its normal."""
    mpf = ref.mp.mpf
    z = [float(x) for x in view.ray([mpf(float(x)) for x in X])]
    l = np.cross([z[0] / z[2], z[1] / z[2], 1.0], rng.uniform(-1, 1, 3))
    l /= np.linalg.norm(l[:2])
    target = max_error ** 2 * (1.0 + rng.choice([-1.0, 1.0]) * rng.uniform(0.008, 0.04))
    step = rng.choice([-1.0, 1.0]) * max_error / float(view.params[0])
    for _ in range(3):                                  # the residual is close to quadratic in the step
        r = ref.residuals(X, ref.Track([view], [[mpf(l[0]), mpf(l[1]), mpf(l[2] + step)]], 1))[0]
        step *= float(ref.mp.sqrt(target / r))
    return np.array([l[0], l[1], l[2] + step])


def visible(scene, v, X):
    """the true point is in front of view v and inside its image"""
    k = int(scene["view_camera"][v])
    P = scene["P"][v]
    z = P[:, :3] @ X + P[:, 3]
    if z[2] < 1e-3:
        return False
    p = [ref.mp.mpf(float(x)) for x in scene["intr"][k]]
    ix, iy = ref.world_to_image(int(scene["camera_model"][k]), p, ref.mp.mpf(z[0] / z[2]), ref.mp.mpf(z[1] / z[2]))
    w, h = scene["cam_size"][k]
    return 2 <= ix < w - 2 and 2 <= iy < h - 2


def make_scene(rng, P, centers, view_camera, camera_model, intr, cam_size, lengths, num_outliers, noise=3e-4, min_good=4, near_axis=0, place=None, threshold_share=0.0):
    """One point per track, observed as a line in lengths[t] views (distinct while the views last), num_outliers(n) of them replaced by random lines.
    A track of four or more observations is redrawn until min_good of its true observations are visible (in front, inside the image): with fewer, the
    exact fits of three inliers tie and the winner is arbitrary - the `degenerate` set holds those on purpose.  `place`: a predicate on the track's
    outlier flags, the track is redrawn until it holds.  threshold_share: this share of the outliers in visible views are threshold_line()s.  The
    first near_axis points lie close to the origin, on every circle view's axis (the centre branches of the FOV and the fisheye models)."""
    V = len(P)
    sc = dict(P=P, centers=centers, view_camera=np.asarray(view_camera, dtype=np.int32), camera_model=np.asarray(camera_model, dtype=np.int32),
              intr=np.asarray(intr, dtype=np.float64), cam_size=np.asarray(cam_size, dtype=np.int32))
    track_start, lines, obs_view, is_out, pts, hidden, at_threshold = [0], [], [], [], [], 0, 0
    mp_views = ref.scene_views(sc)
    for t, n in enumerate(lengths):
        for attempt in range(1000):
            X = rng.uniform(-1, 1, 3) if t >= near_axis else rng.uniform(-0.004, 0.004, 3)
            views = list(rng.permutation(V)[: min(n, V)]) + list(rng.integers(0, V, max(0, n - V)))
            k = num_outliers(n)
            out = np.zeros(n, dtype=bool)
            out[rng.permutation(n)[:k]] = True
            if place is not None and not place(out):
                continue
            vis = [visible(sc, v, X) for v in views]
            good = sum(1 for i in range(n) if vis[i] and not out[i])
            if n < 4 or good >= min_good:
                break
        else:
            raise RuntimeError("no track of length %d with %d visible observations" % (n, min_good))
        hidden += sum(1 for i in range(n) if not vis[i])
        pts.append(X)
        for i, v in enumerate(views):
            if out[i] and vis[i] and rng.random() < threshold_share:
                lines.append(threshold_line(rng, mp_views[v], X, MAX_ERROR[1]))
                at_threshold += 1
            else:
                lines.append(observe(rng, P[v], X, noise, out[i]))
            obs_view.append(int(v))
            is_out.append(bool(out[i]))
        track_start.append(len(lines))
    sc.update(track_start=np.array(track_start, dtype=np.int32), lines=quantise(np.array(lines).reshape(-1, 3)), obs_view=np.array(obs_view, dtype=np.int32),
              points=np.array(pts).reshape(-1, 3), is_outlier=np.array(is_out, dtype=bool), hidden=hidden, at_threshold=at_threshold)
    return sc


def check_distortion(scene):
    """every distortion parameter of every camera, set to zero, moves some true projection by more than a pixel"""
    mpf = ref.mp.mpf
    for k, model in enumerate(scene["camera_model"]):
        model = int(model)
        p = [mpf(float(x)) for x in scene["intr"][k]]
        uv = []
        for v in np.nonzero(scene["view_camera"] == k)[0]:
            for X in scene["points"]:
                z = scene["P"][v][:, :3] @ X + scene["P"][v][:, 3]
                if z[2] > 0.5 and abs(z[0] / z[2]) < 0.5 and abs(z[1] / z[2]) < 0.5:
                    uv.append((mpf(z[0] / z[2]), mpf(z[1] / z[2])))
        for j in range(NUM_FOCAL[model] + 2, ref.NUM_PARAMS[model]):
            q = list(p)
            q[j] = mpf(0)
            if model == 7:
                q[j] = mpf(1e-3)                      # omega = 0 is the pinhole limit; the small-omega branch stands for it
            move = max(max(abs(a - b) for a, b in zip(ref.world_to_image(model, p, u, w), ref.world_to_image(model, q, u, w))) for u, w in uv)
            assert move > 1.0, ("camera %d model %d parameter %d moves projections by %.3g px only" % (k, model, j, float(move)))


SCENE_KEYS = ("track_start", "obs_view", "view_camera", "camera_model", "intr", "cam_size")


def scene_json(sc):
    """the scene as tests/triangulation_reference.load_golden reads it"""
    if "base" in sc:                                   # scene `base` of the set with another cam_size
        return dict(base=sc["base"], cam_size=np.asarray(sc["cam_size"]).tolist())
    out = {k: np.asarray(sc[k]).tolist() for k in SCENE_KEYS}
    if "views_of" in sc:                               # the views of an earlier scene of the set
        out["views_of"] = sc["views_of"]
    else:
        out["P"], out["centers"] = np.asarray(sc["P"]).reshape(-1, 12).tolist(), np.asarray(sc["centers"]).tolist()
    exact = sorted(sc.get("exact_lines", ()))          # lines that are no multiples of 1e-6, written out in full
    q = np.rint(sc["lines"] * 1e6).astype(np.int64)
    assert all(np.array_equal(q[e] / 1e6, sc["lines"][e]) for e in range(len(q)) if e not in exact)
    out["lines_1e6"] = q.reshape(-1).tolist()
    if exact:
        out["lines_exact"] = [[int(e)] + sc["lines"][e].tolist() for e in exact]
    return out


def _work(job):
    scene, options, t = job
    views = ref.scene_views(scene)
    r = ref.triangulate_track(ref.scene_track(scene, views, t, options["residual_type"]), options)
    r["xyz"] = [float(x) for x in r["xyz"]]
    r["mask"] = [int(m) for m in r["mask"]]
    r["margin"] = ref.round_margin(r["margin"])       # what the JSON holds is what classifies the track
    return r


def run(pool, oracle_lib, scene, options):
    """the reference and the oracle on one scene under one option row -> the run's JSON, (oracle disagreements on decided tracks, oracle_xyz_err)"""
    T = len(scene["track_start"]) - 1
    res = pool.map(_work, [(scene, options, t) for t in range(T)], chunksize=4)
    kw = {k: v for k, v in options.items() if k not in ("min_tri_angle", "residual_type")}
    ook, oxyz, omask, ont = oracle_lib.triangulate_tracks(scene, options["min_tri_angle"], options["residual_type"], **kw)
    ts = scene["track_start"]
    err, bad = 0.0, []
    for t, r in enumerate(res):
        if r["margin"] < ref.DECIDED_MARGIN:
            continue
        m = [int(x) for x in omask[ts[t]:ts[t + 1]]]
        if bool(ook[t]) != r["ok"] or int(ont[t]) != r["num_trials"] or m != r["mask"]:
            bad.append(t)
        elif r["ok"]:
            err = max(err, float(np.abs(oxyz[t] - np.array(r["xyz"])).max()))
    out = dict(options=options, ok="".join(str(int(r["ok"])) for r in res), num_trials=[r["num_trials"] for r in res], mask="".join(str(m) for r in res for m in r["mask"]),
               xyz=[r["xyz"] for r in res], margin=[r["margin"] for r in res], support="".join("%x" % r["support"] for r in res),
               near="".join("%x" % r["near"] for r in res))
    return out, bad, err


def finish_set(name, scenes, runs, stats, capped=True):
    """oracle_xyz_err per residual type, the undecided share (asserted where capped)"""
    err = {"0": 0.0, "1": 0.0}
    undecided = total = 0
    for r, (bad, e) in zip(runs, stats):
        rt = str(r["options"]["residual_type"])
        err[rt] = max(err[rt], e)
        undecided += sum(1 for m in r["margin"] if m < ref.DECIDED_MARGIN)
        total += len(r["margin"])
        if capped and min(r["margin"]) < ref.DECIDED_MARGIN:
            print("  %s scene %d %s: undecided tracks %s" % (name, r["scene"], r["options"], [(t, m) for t, m in enumerate(r["margin"]) if m < ref.DECIDED_MARGIN]))
        if bad:
            print("  %s scene %d %s: the ORACLE differs on decided tracks %s" % (name, r["scene"], r["options"], bad))
    share = undecided / total
    print("%-10s %4d track runs, undecided %d (%.2f %%), oracle_xyz_err angular %.3g pixel %.3g" % (name, total, undecided, 100 * share, err["0"], err["1"]), flush=True)
    if capped:
        assert share <= UNDECIDED_CAP, "%s: %.2f %% of the tracks are undecided - change the set's inputs, not the margin or the cap" % (name, 100 * share)
    points, margins = {}, {}                           # the distinct points and margins of the set; a run holds indices into them
    for r in runs:
        r["xyz"] = [points.setdefault(tuple(x), len(points)) for x in r["xyz"]]
        r["margin"] = [margins.setdefault(m, len(margins)) for m in r["margin"]]
    return dict(name=name, scenes=[scene_json(s) for s in scenes], points=[list(x) for x in points], margins=list(margins), runs=runs, oracle_xyz_err=err,
                undecided_share=share)


def base_options(rt, **kw):
    o = dict(residual_type=rt, max_error=MAX_ERROR[rt], min_tri_angle=0.0)
    o.update(kw)
    return o


def outliers_up_to(rng, frac):
    return lambda n: 0 if n < 4 else min(n - 4, int(rng.binomial(n, frac)))


def grid_set(pool, orc):
    rng = np.random.default_rng(20261020)
    P, centers = make_views(rng, 10)
    lengths = rng.integers(0, 13, 129)
    for t, n in ((0, 0), (1, 1), (2, 2), (62, 3), (63, 2), (64, 0), (65, 1), (66, 12), (127, 3), (128, 2)):
        lengths[t] = n
    sc = make_scene(rng, P, centers, np.zeros(10), [2], [intr_row(2, [800.0, CX, CY, 0.01])], [[1280, 960]], lengths, outliers_up_to(rng, 0.15))
    assert set(range(13)) <= set(int(n) for n in lengths)
    runs, stats = [], []
    for rt in (0, 1):                                  # tracks longer than the ten views see a view twice: a pair with no baseline, rejected by an angle > 0
        r, bad, e = run(pool, orc, sc, base_options(rt, min_tri_angle=0.02))
        r["scene"] = 0
        runs.append(r)
        stats.append((bad, e))
    return finish_set("grid", [sc], runs, stats)


# the true observations nearly exact, so that every hypothesis from three of them lies at the truth to a fraction of a per cent of the threshold and the
# threshold lines are judged by the camera model alone
MODELS_NOISE = dict(noise=1e-5, threshold_share=0.8)


def models_set(pool, orc):
    rng = np.random.default_rng(20261021)
    scenes, runs, stats = [], [], []
    P, centers = make_views(rng, 8, 2)
    for model in range(11):
        sc = make_scene(rng, P, centers, np.zeros(10), [model], [intr_row(model)], [[1000, 800]], rng.integers(4, 9, 24), outliers_up_to(rng, 0.5), near_axis=3, **MODELS_NOISE)
        if model:
            sc["views_of"] = 0
        scenes.append(sc)
    P, centers = make_views(rng, 10, 2)                # all models in one call, one camera per view; the twelfth is a FOV camera on its small-omega branch
    cams = list(range(11)) + [7]
    intr = [intr_row(m) for m in range(11)] + [intr_row(7, [F, FY, CX, CY, 0.005])]
    order = rng.permutation(12)                        # the two inside views get models by chance as well
    scenes.append(make_scene(rng, P, centers, order, cams, intr, [[1000 + 16 * k, 800 + 12 * k] for k in range(12)], rng.integers(4, 9, 24),
                             outliers_up_to(rng, 0.5), near_axis=3, **MODELS_NOISE))
    for i, sc in enumerate(scenes):
        if i < 11:
            check_distortion(sc)
        assert sc["hidden"] > 0, "scene %d: no observation is cut by the image or behind its view" % i
        for rt in (0, 1):
            r, bad, e = run(pool, orc, sc, base_options(rt, min_tri_angle=0.02 if rt else 0.0))
            r["scene"] = i
            runs.append(r)
            stats.append((bad, e))
        print("  models scene %d: %d observations cut or behind, %d at the threshold" % (i, sc["hidden"], sc["at_threshold"]), flush=True)
    return finish_set("models", scenes, runs, stats)


OPTION_ROWS = (dict(), dict(confidence=1.0), dict(confidence=0.5), dict(min_inlier_ratio=0.5), dict(max_num_trials=1), dict(max_num_trials=5),
               dict(min_num_trials=10 ** 6), dict(dyn_num_trials_multiplier=1.0), dict(min_tri_angle=0.02), dict(min_tri_angle=0.2))


def options_set(pool, orc):
    rng = np.random.default_rng(20261022)
    P, centers = make_views(rng, 12)
    lengths = rng.permutation(np.repeat(np.arange(3, 11), 4))
    # 40 % outliers over the set (21 of every 52 observations), placed so that four observations of every point stay true - and so that the first five
    # samples, which all hold observations 0 and 1, reach a support above three: under max_num_trials = 5 the track would otherwise end in a tie of exact fits
    sc = make_scene(rng, P, centers, np.zeros(12), [2], [intr_row(2, [800.0, CX, CY, 0.01])], [[1280, 960]], lengths, lambda n: max(0, min(n - 4, int(round(0.6 * n)))),
                    place=lambda out: not out[:2].any() and not out[2:7].all())
    share = sc["is_outlier"].mean()
    assert 0.39 < share < 0.41, share
    tiny = dict(sc, cam_size=np.array([[1, 1]], dtype=np.int32), base=0)      # an image of one pixel: every support is empty
    runs, stats = [], []
    for rt in (0, 1):
        for row in OPTION_ROWS:
            r, bad, e = run(pool, orc, sc, base_options(rt, **row))
            r["scene"] = 0
            runs.append(r)
            stats.append((bad, e))
        for row in (dict(), dict(max_num_trials=5)):
            r, bad, e = run(pool, orc, tiny, base_options(rt, **row))
            r["scene"] = 1
            n3 = [ref.n_choose_3(n) for n in lengths]
            assert r["num_trials"] == [min(c, row.get("max_num_trials", c)) for c in n3] and "1" not in r["ok"]
            runs.append(r)
            stats.append((bad, e))
    return finish_set("options", [sc, tiny], runs, stats)


def degenerate_set(pool, orc):
    rng = np.random.default_rng(20261023)
    P, centers = make_views(rng, 12)
    lengths = [8] * 8 + [7] * 8 + [8] * 8 + [6] * 8
    sc = make_scene(rng, P, centers, np.zeros(12), [2], [intr_row(2, [800.0, CX, CY, 0.01])], [[1280, 960]], lengths, lambda n: 0)
    ts, lines, ov = sc["track_start"], sc["lines"], sc["obs_view"]
    for t in range(32):
        e0 = ts[t]
        if t < 8:                                      # one observation, verbatim, as the first three entries
            for i in (1, 2):
                lines[e0 + i] = lines[e0]
                ov[e0 + i] = ov[e0]
        elif t < 16:                                   # one observation repeated once among good ones
            a, b = rng.permutation(7)[:2]
            lines[e0 + b] = lines[e0 + a]
            ov[e0 + b] = ov[e0 + a]
        elif t < 24:                                   # the first sample: three planes along one common direction, their point at infinity
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            for i in range(3):
                l = np.cross(P[ov[e0 + i]][:, :3] @ d, rng.uniform(-1, 1, 3))
                lines[e0 + i] = l / np.linalg.norm(l[:2])          # not rounded to 1e-6: perpendicular to d to the last bit
                sc.setdefault("exact_lines", set()).add(int(e0 + i))
        else:                                          # exactly three inliers, three outliers: every sample fits its three lines exactly
            for i in rng.permutation(6)[:3]:
                lines[e0 + i] = quantise(observe(rng, P[ov[e0 + i]], sc["points"][t], 0.0, "far"))
    runs, stats = [], []
    for rt in (0, 1):
        r, bad, e = run(pool, orc, sc, base_options(rt, confidence=0.9999))
        r["scene"] = 0
        runs.append(r)
        stats.append((bad, e))
    return finish_set("degenerate", [sc], runs, stats, capped=False)


def main():
    import oracle_lib
    oracle_lib.build()
    oracle_lib.lib()
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        sets = [f(pool, oracle_lib) for f in (grid_set, models_set, options_set, degenerate_set)]
    out = os.path.join(HERE, "triangulation_golden.json")
    with open(out, "w") as f:
        json.dump({"generator": "tests/golden/gen_triangulation_golden.py", "digits": 50, "decided_margin": ref.DECIDED_MARGIN, "sets": sets}, f, separators=(",", ":"))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
