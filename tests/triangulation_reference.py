"""EstimateTriangulation in 50-digit arithmetic - TEST INFRASTRUCTURE (tests/golden/gen_triangulation_golden.py mints the golden file with it,
tests/test_triangulation_reference.py holds the oracle to it on the CPU, tests/test_gpu_triangulation_exact.py the device).

A restatement of oracle/triangulation.h (reference estimators/triangulation.cc:55-149, optim/loransac.h:88-235, base/projection.cc:161-203, 238-262)
over mpmath at 50 digits, generic over the 11 camera models (the formulas of tests/golden/gen_line_cost_golden.py as plain functions; the piecewise
models take the branch the C++ takes).  The null vector of a minimal sample is the vector of exact 3x3 minors, the local optimisation's the eigenvector
of the 4x4 Gram matrix for its smallest eigenvalue.  With zero inliers the trial bound is "never abort" (csrc/tri_device.hpp, TriNumTrials).

Besides its result every track returns its MARGIN: the smallest separation of any comparison the reference met on its own trajectory.  A track is
DECIDED when the margin is at least DECIDED_MARGIN = 1e-6: every correct double implementation then takes the reference's branches, so success flag, trial
count and inlier mask must equal the reference's exactly.  The separations (relative ones against the larger operand):
  proj_z against DBL_EPSILON (0 for the angular residual)   |proj_z - bound| / |P X|: against the length of the ray, because against the larger operand
                                                            a comparison with 0 would always separate by 1
  the projection against the four image borders             in pixels, over the image's width or height
  each triangulation angle against min_tri_angle            every pair of the sample, also the ones a short-circuit skips.  min_tri_angle = 0 accepts every
                                                            angle that is a number, so there the separation is the acos argument's distance from +-1
  each residual against max_residual
  residual_sum against best_sum at equal inlier counts      two sums both below SUM_FLOOR * max_residual are EQUAL (separation 0): the exact fits of three
                                                            inliers, rounding noise in double.  Two empty sums are both exactly 0 in any implementation and
                                                            separate by 1.
  the real number inside ceil() of a trial bound            against the nearest integer
  (sigma_3 - sigma_4) / sigma_1 of every system solved      sigma_4 = 0 for a minimal sample's 3 x 4 system
  |h_3| / |h| of every null vector
One comparison may be FORGOTTEN: residual_sum against best_sum at a count of three or less.  Its two outcomes differ in the best model held and in a
best_sum that is rounding noise either way; neither a local optimisation (it needs more than three inliers) nor the trial bound (a function of the count)
sees the difference.  So once a later hypothesis wins on the COUNT, or the track ends below three inliers (no point is reported), nothing reported
depends on it any more, and it no longer enters the margin.  Without this rule every track with an outlier among its first observations were undecided."""
import json
import math
import os

import mpmath
import numpy as np

mp = mpmath.MPContext()
mp.dps = 50

DECIDED_MARGIN = 1e-6
SUM_FLOOR = 1e-12
NUM_PARAMS = (3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12)
DBL_EPSILON = mp.mpf(2.220446049250313e-16)
_FOV_EPS = mp.mpf(1e-4)
_HALF_PI = mp.pi / 2

DEFAULT_OPTIONS = dict(min_tri_angle=0.0, residual_type=0, max_error=0.0, min_inlier_ratio=0.1, confidence=0.99, dyn_num_trials_multiplier=3.0,
                       min_num_trials=0, max_num_trials=2 ** 64 - 1)


def _fisheye(u, v, ks):
    r = mp.sqrt(u * u + v * v)
    if not r > DBL_EPSILON:
        return u, v
    th = mp.atan(r)
    series = 1
    for i, k in enumerate(ks):
        series = series + k * th ** (2 * (i + 1))
    thd = th * series
    return u * thd / r, v * thd / r


def world_to_image(model, p, u, v):
    """(u, v) on the normalised plane -> pixels (reference base/camera_models.h, WorldToImage of the 11 models)"""
    if model == 0:
        return p[0] * u + p[1], p[0] * v + p[2]
    if model == 1:
        return p[0] * u + p[2], p[1] * v + p[3]
    if model == 2:
        rad = p[3] * (u * u + v * v)
        return p[0] * (u + u * rad) + p[1], p[0] * (v + v * rad) + p[2]
    if model == 3:
        r2 = u * u + v * v
        rad = p[3] * r2 + p[4] * r2 * r2
        return p[0] * (u + u * rad) + p[1], p[0] * (v + v * rad) + p[2]
    if model == 4:
        u2, uv, v2 = u * u, u * v, v * v
        r2 = u2 + v2
        rad = p[4] * r2 + p[5] * r2 * r2
        du = u * rad + 2 * p[6] * uv + p[7] * (r2 + 2 * u2)
        dv = v * rad + 2 * p[7] * uv + p[6] * (r2 + 2 * v2)
        return p[0] * (u + du) + p[2], p[1] * (v + dv) + p[3]
    if model == 5:
        xd, yd = _fisheye(u, v, p[4:8])
        return p[0] * xd + p[2], p[1] * yd + p[3]
    if model == 6:
        u2, uv, v2 = u * u, u * v, v * v
        r2 = u2 + v2
        r4 = r2 * r2
        r6 = r4 * r2
        rad = (1 + p[4] * r2 + p[5] * r4 + p[8] * r6) / (1 + p[9] * r2 + p[10] * r4 + p[11] * r6)
        xd = u * rad + 2 * p[6] * uv + p[7] * (r2 + 2 * u2)
        yd = v * rad + 2 * p[7] * uv + p[6] * (r2 + 2 * v2)
        return p[0] * xd + p[2], p[1] * yd + p[3]
    if model == 7:
        om = p[4]
        rad2 = u * u + v * v
        om2 = om * om
        if om2 < _FOV_EPS:
            f = (om2 * rad2) / 3 - om2 / 12 + 1
        elif rad2 < _FOV_EPS:
            th = mp.tan(om / 2)
            f = (-2 * th * (4 * rad2 * th * th - 3)) / (3 * om)
        else:
            rad = mp.sqrt(rad2)
            f = mp.atan(rad * 2 * mp.tan(om / 2)) / (rad * om)
        return p[0] * (u * f) + p[2], p[1] * (v * f) + p[3]
    if model == 8:
        xd, yd = _fisheye(u, v, p[3:4])
        return p[0] * xd + p[1], p[0] * yd + p[2]
    if model == 9:
        xd, yd = _fisheye(u, v, p[3:5])
        return p[0] * xd + p[1], p[0] * yd + p[2]
    if model == 10:
        uu, vv = _fisheye(u, v, ())
        u2, uv, v2 = uu * uu, uu * vv, vv * vv
        r2 = u2 + v2
        r4 = r2 * r2
        r6 = r4 * r2
        r8 = r6 * r2
        rad = p[4] * r2 + p[5] * r4 + p[8] * r6 + p[9] * r8
        du = uu * rad + 2 * p[6] * uv + p[7] * (r2 + 2 * u2) + p[10] * r2
        dv = vv * rad + 2 * p[7] * uv + p[6] * (r2 + 2 * v2) + p[11] * r2
        return p[0] * (uu + du) + p[2], p[1] * (vv + dv) + p[3]
    raise ValueError(model)


class View:
    def __init__(self, P, center, model, params, width, height):
        self.P = [mp.mpf(float(x)) for x in P]
        self.center = [mp.mpf(float(x)) for x in center]
        self.model = int(model)
        self.params = [mp.mpf(float(x)) for x in params]
        self.width, self.height = mp.mpf(int(width)), mp.mpf(int(height))

    def ray(self, X):
        P = self.P
        return [P[4 * r] * X[0] + P[4 * r + 1] * X[1] + P[4 * r + 2] * X[2] + P[4 * r + 3] for r in range(3)]

    def row(self, l):
        P = self.P
        return [l[0] * P[c] + l[1] * P[4 + c] + l[2] * P[8 + c] for c in range(4)]


class Track:
    """the observations of one track: views[i] sees lines[i]"""

    def __init__(self, views, lines, residual_type):
        self.views, self.lines, self.residual_type = views, lines, int(residual_type)
        self.n = len(views)


def scene_views(scene):
    """the scene's views (the arrays of synthetic.make_track_scene) at 50 digits"""
    Pm, ctr, intr, cs = scene["P"], scene["centers"], scene["intr"], scene["cam_size"]
    out = []
    for v in range(len(scene["view_camera"])):
        k = int(scene["view_camera"][v])
        out.append(View(np.asarray(Pm[v], dtype=np.float64).reshape(12), ctr[v], scene["camera_model"][k], intr[k], cs[k][0], cs[k][1]))
    return out


def scene_track(scene, views, t, residual_type):
    e0, e1 = int(scene["track_start"][t]), int(scene["track_start"][t + 1])
    return Track([views[int(scene["obs_view"][e])] for e in range(e0, e1)], [[mp.mpf(float(x)) for x in scene["lines"][e]] for e in range(e0, e1)], residual_type)


def _rel(a, b):
    m = max(abs(a), abs(b))
    return mp.mpf(0) if m == 0 else abs(a - b) / m


def _norm(v):
    return mp.sqrt(sum(x * x for x in v))


def _residual(tr, i, X):
    """-> (residual, or None where the C++ returns DBL_MAX; the smallest separation of the comparisons that accept or reject the observation)"""
    v, l = tr.views[i], tr.lines[i]
    r0, r1, r2 = v.ray(X)
    bound = DBL_EPSILON if tr.residual_type == 1 else mp.mpf(0)
    sep = abs(r2 - bound) / max(_norm((r0, r1, r2)), DBL_EPSILON)
    if r2 < bound:
        return None, sep
    u, w = r0 / r2, r1 / r2
    ix, iy = world_to_image(v.model, v.params, u, w)
    sep = min(sep, abs(ix) / v.width, abs(ix - v.width) / v.width, abs(iy) / v.height, abs(iy - v.height) / v.height)
    if not (ix >= 0 and ix < v.width and iy >= 0 and iy < v.height):
        return None, sep
    if tr.residual_type == 1:
        alpha = l[0] * u + l[1] * w + l[2]
        jx, jy = world_to_image(v.model, v.params, u - l[0] * alpha, w - l[1] * alpha)
        return (ix - jx) ** 2 + (iy - jy) ** 2, sep
    d = (l[0] * r0 + l[1] * r1 + l[2] * r2) / (_norm(l) * _norm((r0, r1, r2)))
    return abs(_HALF_PI - mp.acos(min(abs(d), mp.mpf(1)))) ** 2, sep


def residuals(xyz, track, max_residual=None):
    """The 50-digit residuals of the track's observations at xyz (mp.inf where the C++ returns DBL_MAX).  With max_residual: (residuals, separations) -
    per observation the smallest separation of the comparisons that make it an inlier or not at this point."""
    X = [x if isinstance(x, mp.mpf) else mp.mpf(float(x)) for x in xyz]
    rs, seps = [], []
    for i in range(track.n):
        r, sep = _residual(track, i, X)
        if r is not None and max_residual is not None:
            sep = min(sep, _rel(r, max_residual if isinstance(max_residual, mp.mpf) else mp.mpf(float(max_residual))))
        rs.append(mp.inf if r is None else r)
        seps.append(sep)
    return rs if max_residual is None else (rs, seps)


def _tri_angle_cos(c1, c2, X):
    b2 = sum((a - b) ** 2 for a, b in zip(c1, c2))
    r1 = sum((x - a) ** 2 for x, a in zip(X, c1))
    r2 = sum((x - a) ** 2 for x, a in zip(X, c2))
    den = 2 * mp.sqrt(r1 * r2)
    if den == 0:
        return None
    return (r1 + r2 - b2) / den


def _num_trials_bound(num_inliers, num_samples, confidence, multiplier):
    """RANSAC::ComputeNumTrials (optim/ransac.h:158-176) -> (bound, None = never abort; separation of the ceil argument from the nearest integer)"""
    ratio = mp.mpf(num_inliers) / num_samples
    nom = 1 - mp.mpf(float(confidence))
    if nom <= 0:
        return None, mp.mpf(1)
    denom = 1 - ratio ** 3
    if denom <= 0:
        return 1, mp.mpf(1)
    if num_inliers == 0:
        return None, mp.mpf(1)                       # log(1) = 0 in the denominator: never abort
    v = mp.log(nom) / mp.log(denom) * mp.mpf(float(multiplier))
    if v < 0:
        return None, mp.mpf(1)
    return int(mp.ceil(v)), _rel(v, mp.floor(v + mp.mpf(0.5)))


class _Margin:
    def __init__(self):
        self.hard = mp.mpf(1)
        self.soft = mp.mpf(1)

    def add(self, sep):
        self.hard = min(self.hard, sep)


def _estimate(tr, idx, min_tri_angle, mg):
    """TriangulationEstimator::Estimate on the observations idx -> X or None"""
    rows = [tr.views[i].row(tr.lines[i]) for i in idx]
    if len(idx) == 3:
        a, b, c = rows

        def det3(i0, i1, i2):
            return a[i0] * (b[i1] * c[i2] - b[i2] * c[i1]) - a[i1] * (b[i0] * c[i2] - b[i2] * c[i0]) + a[i2] * (b[i0] * c[i1] - b[i1] * c[i0])
        h = [det3(1, 2, 3), -det3(0, 2, 3), det3(0, 1, 3), -det3(0, 1, 2)]
        G = mp.matrix(3, 3)
        for r in range(3):
            for s in range(3):
                G[r, s] = sum(rows[r][k] * rows[s][k] for k in range(4))
        ev = sorted(mp.eigsy(G, eigvals_only=True))
        s_small, s_large = mp.sqrt(max(ev[0], 0)), mp.sqrt(max(ev[2], 0))
        mg.add(s_small / s_large if s_large > 0 else mp.mpf(0))
    else:
        S = mp.matrix(4, 4)
        for row in rows:
            for r in range(4):
                for s in range(4):
                    S[r, s] += row[r] * row[s]
        E, Q = mp.eigsy(S)
        order = sorted(range(4), key=lambda k: E[k])
        sig = [mp.sqrt(max(E[k], 0)) for k in order]
        mg.add((sig[1] - sig[0]) / sig[3] if sig[3] > 0 else mp.mpf(0))
        h = [Q[r, order[0]] for r in range(4)]
    hn = _norm(h)
    if hn == 0 or h[3] == 0:
        mg.add(mp.mpf(0))
        return None
    mg.add(abs(h[3]) / hn)
    X = [h[0] / h[3], h[1] / h[3], h[2] / h[3]]
    front = True
    for i in idx:
        r0, r1, r2 = tr.views[i].ray(X)
        mg.add(abs(r2 - DBL_EPSILON) / max(_norm((r0, r1, r2)), DBL_EPSILON))
        front = front and r2 >= DBL_EPSILON
    if not front:
        return None
    mta = mp.mpf(float(min_tri_angle))
    wide = False
    for a in range(len(idx)):
        for b in range(a):
            c = _tri_angle_cos(tr.views[idx[a]].center, tr.views[idx[b]].center, X)
            if c is None:
                ang = mp.mpf(0)
                mg.add(_rel(ang, mta))
            else:
                ang = abs(mp.acos(max(min(c, mp.mpf(1)), mp.mpf(-1))))
                ang = min(ang, mp.pi - ang)
                mg.add(_rel(ang, mta) if mta > 0 else 1 - abs(c))
            wide = wide or ang >= mta
    return X if wide else None


def _support(tr, X, max_residual, mg):
    inl, total, flags = 0, mp.mpf(0), []
    for i in range(tr.n):
        r, sep = _residual(tr, i, X)
        mg.add(sep)
        ok = False
        if r is not None:
            mg.add(_rel(r, max_residual))
            ok = r <= max_residual
        if ok:
            inl += 1
            total += r
        flags.append(ok)
    return inl, total, flags


def _better(inl, total, best_inl, best_sum, max_residual, mg):
    if inl != best_inl:
        return inl > best_inl
    if best_sum is None:                              # the default Support: zero inliers, residual_sum = DBL_MAX
        return True
    if inl == 0:                                      # two empty sums: exactly 0 both
        return False
    floor = SUM_FLOOR * max_residual
    sep = mp.mpf(0) if (total < floor and best_sum < floor) else _rel(total, best_sum)
    if inl <= 3:
        mg.soft = min(mg.soft, sep)
    else:
        mg.add(sep)
    return total < best_sum


def triangulate_track(tr, options):
    """EstimateTriangulation of one track -> dict(ok, xyz (three mpf), mask, num_trials, margin, support, near): `support` the winner's inlier count,
    `near` the number of observations whose comparisons at the winner separate by less than DECIDED_MARGIN"""
    o = dict(DEFAULT_OPTIONS)
    o.update(options)
    n = tr.n
    out = dict(ok=False, xyz=[mp.mpf(0)] * 3, mask=[False] * n, num_trials=0, margin=1.0, support=0, near=0)
    if n < 3:
        return out
    mg = _Margin()
    max_residual = mp.mpf(float(o["max_error"])) ** 2
    cap, sep = _num_trials_bound(int(float(o["min_inlier_ratio"]) * 100000), 100000, o["confidence"], o["dyn_num_trials_multiplier"])
    mg.add(sep)
    max_num_trials = int(o["max_num_trials"]) if cap is None else min(int(o["max_num_trials"]), cap)
    max_num_trials = min(max_num_trials, n * (n - 1) * (n - 2) // 6)
    min_num_trials = int(o["min_num_trials"])
    best_inl, best_sum, best, best_flags, best_seps = 0, None, [mp.mpf(0)] * 3, [False] * n, None
    dyn = max_num_trials
    abort = False
    comb = [0, 1, 2]
    trials = 0
    while trials < max_num_trials:
        if abort:
            trials += 1
            break
        sample = list(comb)
        if comb[2] + 1 < n:
            comb[2] += 1
        elif comb[1] + 2 < n:
            comb[1] += 1
            comb[2] = comb[1] + 1
        elif comb[0] + 3 < n:
            comb[0] += 1
            comb[1], comb[2] = comb[0] + 1, comb[0] + 2
        else:
            comb = [0, 1, 2]
        X = _estimate(tr, sample, o["min_tri_angle"], mg)
        if X is None:                                 # "continue": the abort test below is skipped too
            trials += 1
            continue
        inl, total, flags = _support(tr, X, max_residual, mg)
        if _better(inl, total, best_inl, best_sum, max_residual, mg):
            if inl > best_inl:
                mg.soft = mp.mpf(1)
            best_inl, best_sum, best, best_flags = inl, total, X, flags
            if inl > 3:
                L = _estimate(tr, [i for i in range(n) if flags[i]], o["min_tri_angle"], mg)
                if L is not None:
                    linl, ltotal, lflags = _support(tr, L, max_residual, mg)
                    if _better(linl, ltotal, best_inl, best_sum, max_residual, mg):
                        best_inl, best_sum, best, best_flags = linl, ltotal, L, lflags
            dyn, sep = _num_trials_bound(best_inl, n, o["confidence"], o["dyn_num_trials_multiplier"])
            mg.add(sep)
        if (dyn is not None and trials >= dyn) and trials >= min_num_trials:
            abort = True
        trials += 1
    out["num_trials"] = trials
    out["support"] = best_inl
    margin = mg.hard if best_inl < 3 else min(mg.hard, mg.soft)
    out["margin"] = float(min(margin, mp.mpf(1)))
    if best_inl < 3:
        return out
    out["ok"] = True
    out["xyz"] = best
    out["mask"] = best_flags
    _, seps = residuals(best, tr, max_residual)
    out["near"] = sum(1 for s in seps if s < DECIDED_MARGIN)
    return out


def triangulate_scene(scene, options, tracks=None):
    """the reference on the tracks (default: all) of a scene dict; -> list of triangulate_track results"""
    views = scene_views(scene)
    T = len(scene["track_start"]) - 1
    rt = int(options.get("residual_type", 0))
    return [triangulate_track(scene_track(scene, views, t, rt), options) for t in (range(T) if tracks is None else tracks)]


def n_choose_3(n):
    return math.comb(int(n), 3)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "triangulation_golden.json")
_SCENE_TYPES = dict(track_start=np.int32, obs_view=np.int32, view_camera=np.int32, camera_model=np.int32, intr=np.float64, cam_size=np.int32)


def round_margin(m):
    """a margin to three digits, never upwards: the form the golden file holds and classifies by"""
    r = float("%.2e" % m)
    return r if r <= m else float("%.2e" % (m * 0.995))


def _scene(sc, scenes):
    """a scene of the golden file as arrays: the lines are whole multiples of 1e-6 (`lines_exact`: index and coefficients of those that are not), `views_of`
    names the scene whose views it shares, `base` the scene it repeats with another cam_size"""
    if "base" in sc:
        return dict(scenes[sc["base"]], cam_size=np.array(sc["cam_size"], dtype=np.int32))
    out = {k: np.array(sc[k], dtype=t).reshape((-1, 2) if k == "cam_size" else (-1, 12) if k == "intr" else -1) for k, t in _SCENE_TYPES.items()}
    src = scenes[sc["views_of"]] if "views_of" in sc else sc
    out["P"], out["centers"] = np.array(src["P"], dtype=np.float64).reshape(-1, 12), np.array(src["centers"], dtype=np.float64).reshape(-1, 3)
    out["lines"] = np.array(sc["lines_1e6"], dtype=np.int64).reshape(-1, 3) / 1e6
    for e, a, b, c in sc.get("lines_exact", ()):
        out["lines"][e] = (a, b, c)
    return out


def load_golden(path=GOLDEN):
    """tests/golden/triangulation_golden.json as {set name: set}: the scenes as numpy arrays, per run `ok`, `mask`, `decided` as bool arrays, `xyz`,
    `margin`, `num_trials`, `support`, `near` as arrays (the file holds each set's distinct points and margins once and indices per run)"""
    with open(path) as f:
        g = json.load(f)
    bits = lambda text: np.frombuffer(text.encode(), dtype=np.uint8) == ord("1")
    out = {}
    for s in g["sets"]:
        scenes = []
        for sc in s["scenes"]:
            scenes.append(_scene(sc, scenes))
        s["scenes"] = scenes
        points, margins = np.array(s["points"], dtype=np.float64).reshape(-1, 3), np.array(s["margins"], dtype=np.float64)
        for r in s["runs"]:
            r["ok"], r["mask"] = bits(r["ok"]), bits(r["mask"])
            r["xyz"] = points[np.array(r["xyz"], dtype=np.int64)].reshape(-1, 3)
            r["margin"], r["num_trials"] = margins[np.array(r["margin"], dtype=np.int64)], np.array(r["num_trials"])
            for k in ("support", "near"):
                r[k] = np.array([int(c, 16) for c in r[k]])
            r["decided"] = r["margin"] >= g["decided_margin"]
        out[s["name"]] = s
    return out
