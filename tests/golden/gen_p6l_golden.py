#!/usr/bin/env python3
"""Generate tests/golden/p6l_golden.json.

Three quadrics in three unknowns (re3q3) and six-line absolute poses (P6L), solved exactly by tests/p6l_reference.py: per system the real roots
rounded to double and their number (exact), the number of finite roots, the smallest separation `sep`, per real root the condition number `kappa` (see
that module); the complex roots only of an undecided system; the P6L poses are evaluated from the roots on loading (ref.poses_at).
The inputs are written out as arrays, not as seeds: whole multiples of 2^-13 (quadrics), 2^-24 (lines) and 2^-20 (points), as integers.  The oracle
(tests/test_p6l_reference.py) and the HIP kernel K5 (tests/test_gpu_p6l_exact.py) are both held to these numbers: root by root on the DECIDED systems (every sep >= 1e-3), by invariants on the others.

Sets (see main):
  quadrics_random       uniform coefficients in [-1, 1]
  quadrics_elim         each of elim = 0, 1, 2 chosen by a clear margin (the largest of Re3q3Device's three determinants at least four times the next),
                        and a `near_tie` half where the two largest are within a factor of two of each other
  quadrics_degenerate   the four constructions of test_re3q3_reference_properties (one of the three determinants exactly 0, two in the fourth) and
                        the +-1 cube (all three 0: the fixed change of variables)
  quadrics_scaled       systems of quadrics_random (`parent`) with each row scaled by 2^+-40, and one with all coefficients scaled by 2^-200
  p6l_clean             exact six-tuples drawn as synthetic.make_ransac_scene draws them; the ground-truth pose is among the reference's poses (asserted)
  p6l_outliers          noisy six-tuples with one to three outlier lines
  p6l_degenerate_lines  lines 0-2 through one image point (det B^T = 0: the mix branch), lines 3-5, both; one to five gravity-aligned flags; all six
                        (no model)
  quadrics_special      four systems as full doubles, no cap: the regular system FOUND below and the same times 2^-40; two systems with root pairs 2^-12
                        and 2^-16 apart, undecided on purpose
There is no p6l_minor set (a 2x2 minor m00 m11 - m10 m01 of the back substitution below 1e-6 of its terms at a real root): a search of 20 000 six-tuples
drawn like p6l_clean and p6l_outliers (`python tests/golden/p6l_host_check.py minor`) found none - the smallest ratio was 1.3e-5, twelve were below 1e-4.

At most 2 % of a set's systems may be undecided (the near-tie half of quadrics_elim apart); the script asserts it and prints the share.  It also runs the
CPU oracle on every decided system, asserts that it returns the exact number of real roots and matches them one to one, and records per system
  oracle_sys    the oracle's largest |s - s*|_inf / (2^-52 kappa (1 + |s*|_inf)) over the system's real roots; for a six-tuple over the twelve entries of
                its poses (P6L returns poses only), normalised by the root's kappa and size.  The largest over the system itself and 32 copies with
                every input moved by one unit in the last place (ref.oracle_error): one run alone may sit far below the system's amplification by luck
and per set oracle_floor, the nine-tenths quantile of oracle_sys (quadrics_special: that of quadrics_random), and oracle_max.  The device is held, system
by system, to 4 x max(oracle_sys, oracle_floor): the elimination both share amplifies roundings by a factor that belongs to the system (median about 10,
a few systems at 1e5 and more), so one maximum for a whole set would leave every other system unbounded by six orders; where the oracle was merely lucky,
the set's ordinary level holds.  These numbers come from the oracle and the reference, never from the kernel.

Run from the repo root (minutes, CPU only):  python tests/golden/gen_p6l_golden.py
"""
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import p6l_reference as ref  # noqa: E402

UNDECIDED_CAP = 0.02


def elim_dets(c):
    """the three determinants by which Re3q3Device picks the unknown to eliminate"""
    return np.array(ref.elim_choice(c)[2])


def grid(a, unit):
    """a rounded to whole multiples of the file's unit (a power of two): what the JSON holds"""
    return np.rint(np.asarray(a, dtype=np.float64) / unit) * unit


def draw_quadrics(rng):
    return grid(rng.uniform(-1, 1, (3, 10)), 2 * ref.QUADRIC_UNIT)          # on twice the unit: the halves of quadrics_degenerate are exact


def quadrics_random(rng, n=66):
    return [dict(c=draw_quadrics(rng)) for _ in range(n)]


def quadrics_elim(rng, clear_each=10, ties=34):
    out, clear, near = [], {0: 0, 1: 0, 2: 0}, 0
    while min(clear.values()) < clear_each or near < ties:
        c = draw_quadrics(rng)
        d = elim_dets(c)
        e = int(np.argmax(d))
        first, second = np.sort(d)[::-1][:2]
        tight = near % 3 == 0                          # every third near tie within 5 %
        if first >= 4 * second and clear[e] < clear_each:
            clear[e] += 1
            out.append(dict(c=c, elim=e, near_tie=0))
        elif first < (1.05 if tight else 2.0) * second and near < ties:
            near += 1
            out.append(dict(c=c, elim=e, near_tie=1))
    return out


def quadrics_degenerate(rng, each=16):
    out = []
    for kind in range(4):
        for _ in range(each):
            c = draw_quadrics(rng)
            if kind == 0:                              # degenerate for x
                c[:, 3] = 0.5 * (c[:, 5] + c[:, 4])
            if kind in (1, 3):                         # y
                c[:, 0] = 0.5 * (c[:, 5] + c[:, 2])
            if kind == 2:                              # z
                c[:, 0] = 0.5 * (c[:, 1] + c[:, 3])
            if kind == 3:                              # two at once
                c[:, 3] = 0.5 * (c[:, 5] + c[:, 4])
            assert (elim_dets(c) == 0).sum() == (2 if kind == 3 else 1)
            out.append(dict(c=c, kind=kind))
    cube = np.zeros((3, 10))
    cube[0, 0] = cube[1, 3] = cube[2, 5] = 1.0
    cube[:, 9] = -1.0
    out.append(dict(c=cube, kind=4))
    return out


def quadrics_scaled(rng, parents):
    out = []
    for i in range(63):
        e = [int(v) for v in rng.choice([-40, 40], 3)]
        out.append(dict(c=parents[i]["c"] * (2.0 ** np.array(e, dtype=np.float64))[:, None], parent=i, exp=e))
    out.append(dict(c=parents[63]["c"] * 2.0 ** -200, parent=63, exp=[-200] * 3))
    return out


# the regular system found while these sets were first drawn (then with full 52-bit coefficients): every row times 2^-40 it falls under the absolute 1e-10
# determinant test and takes the change of variables, where one well-conditioned root comes out 1e6 roundings off (tests/test_gpu_p6l_exact.py)
FOUND = [-0.9267888740892305, -0.2499154746136707, -0.6592717464406999, -0.9946518867139567, -0.38500111408227866, 0.5337957746595654, -0.3526902093392392,
         0.7308473013499026, 0.4293765102467635, 0.5947302124466651, -0.8427567305574653, -0.9713524251500969, -0.27320964726850194, 0.9462456207375933,
         -0.03136789109732718, 0.1485184326906137, -0.42919779014704584, 0.43496906783398503, -0.44622173632655615, 0.10866013140718644, -0.7986625683473563,
         -0.03755214188376521, 0.08387709424397549, 0.6120759033006942, 0.6374983885536538, -0.854653969614801, -0.29980344119015867, 0.7701664760822473,
         0.3346909769908919, 0.1003158647314435]


def quadrics_special():
    """0: FOUND; 1: FOUND times 2^-40; 2, 3: eight real roots in four pairs 2^-12 and 2^-16 apart in x - undecided on purpose, so that the invariants on
    all systems meet roots that a double solver may or may not tell apart"""
    out = [dict(c=np.array(FOUND).reshape(3, 10)), dict(c=np.array(FOUND).reshape(3, 10) * 2.0 ** -40)]
    for d in (2.0 ** -12, 2.0 ** -16):
        c = np.zeros((3, 10))
        c[0, 0], c[0, 6], c[0, 9] = 1.0, -(1.0 + d), 0.5 * (0.5 + d)          # (x - 1/2)(x - 1/2 - d)
        c[1, 3], c[1, 1], c[1, 9] = 1.0, 0.5, -1.0                            # y^2 + xy/2 - 1
        c[2, 5], c[2, 4], c[2, 9] = 1.0, 0.25, -2.0                           # z^2 + yz/4 - 2
        out.append(dict(c=c))
    return out


def on_grid(t):
    t["lines"], t["points"] = grid(t["lines"], ref.LINE_UNIT), grid(t["points"], ref.POINT_UNIT)
    return t


def six_tuple(rng, noise_px, num_outliers, focal=1000.0):
    """six correspondences as synthetic.make_ransac_scene draws them, with exactly num_outliers outlier lines, rounded to the file's grid (lines 2^-24,
    points 2^-20: 6e-5 and 1e-3 of a pixel at this focal length)"""
    from privacy_preserving_sfm_amd import synthetic
    sc = synthetic.make_ransac_scene(6, outlier_ratio=0.0, noise_px=noise_px, focal=focal, seed=int(rng.integers(1 << 31)))
    lines = sc["lines"].copy()
    for i in rng.permutation(6)[:num_outliers]:
        x = rng.uniform(-0.5, 0.5, 2)
        th = rng.uniform(0, 2 * np.pi)
        lines[i] = [np.cos(th), np.sin(th), -(np.cos(th) * x[0] + np.sin(th) * x[1])]
    return on_grid(dict(lines=lines, points=sc["points"], aligned=np.zeros(6, dtype=np.uint8), gt_pose=sc["gt_pose"]))


def p6l_clean(rng, n=64):
    return [six_tuple(rng, 0.0, 0) for _ in range(n)]


def p6l_outliers(rng, n=64):
    return [six_tuple(rng, 0.5, int(rng.integers(1, 4))) for _ in range(n)]


def concurrent_tuple(rng, groups):
    """a six-tuple of a true pose whose lines of every group (0: lines 0-2, 1: lines 3-5) pass through ONE image point: image points on a 2^-12 grid,
    l = p x x_i without normalisation (whole multiples of 2^-24), so the three lines are exactly dependent"""
    from privacy_preserving_sfm_amd import synthetic
    sc = synthetic.make_ransac_scene(6, outlier_ratio=0.0, noise_px=0.0, seed=int(rng.integers(1 << 31)))
    R, t = sc["gt_pose"][:, :3], sc["gt_pose"][:, 3]
    x = np.rint(rng.uniform(-0.4, 0.4, (6, 2)) * 4096) / 4096
    Xc = np.concatenate([x, np.ones((6, 1))], axis=1) * rng.uniform(2, 6, (6, 1))
    points = (Xc - t) @ R
    lines = np.zeros((6, 3))
    for g in range(2):
        if g in groups:
            p = np.append(np.rint(rng.uniform(-0.4, 0.4, 2) * 4096) / 4096, 1.0)
            for i in range(3 * g, 3 * g + 3):
                lines[i] = np.cross(p, np.append(x[i], 1.0))
                assert np.dot(lines[i], p) == 0.0 and np.array_equal(grid(lines[i], ref.LINE_UNIT), lines[i])
        else:
            for i in range(3 * g, 3 * g + 3):
                th = rng.uniform(0, 2 * np.pi)
                lines[i] = [np.cos(th), np.sin(th), -(np.cos(th) * x[i, 0] + np.sin(th) * x[i, 1])]
    return on_grid(dict(lines=lines, points=points, aligned=np.zeros(6, dtype=np.uint8), gt_pose=sc["gt_pose"], groups="".join(str(g) for g in groups)))


def p6l_degenerate_lines(rng):
    out = [concurrent_tuple(rng, (0,)) for _ in range(16)] + [concurrent_tuple(rng, (1,)) for _ in range(16)] + [concurrent_tuple(rng, (0, 1)) for _ in range(8)]
    for k in range(24):                                # one to five flags, then all six
        s = six_tuple(rng, 0.0, 0)
        flags = 1 + k % 5 if k < 20 else 6
        s["aligned"][rng.permutation(6)[:flags]] = 1
        s["groups"] = "-"
        out.append(s)
    return out


def _solve(system):
    res = ref.solve_quadrics(system["c"]) if "c" in system else ref.solve_p6l(system["lines"], system["points"])
    assert res is not None, "no shape basis"
    return ref.system_json(res)


def ints(a, unit):
    q = np.asarray(a, dtype=np.float64).reshape(-1) / unit
    assert np.array_equal(q, np.rint(q))
    return [int(v) for v in q]


def build_set(pool, orc, name, systems, parents=None, capped=True, floor=None, full=False):
    res = pool.map(_solve, systems, chunksize=1)
    if parents is not None:                            # the same rational system up to units: the reference's roots are the parent's, bit for bit.  The
        for s, e in zip(systems, res):                 # conditioning of a root does not depend on a row's scale; kappa's formula, with the largest row's
            assert dict(e, kappa=0) == dict(parents[1][s["parent"]], kappa=0), (name, s["parent"])       # size, does (up to 2^80): the parent's kappa holds
            e["kappa"] = parents[1][s["parent"]]["kappa"]
    undecided = capped_total = capped_undecided = 0
    per_system, measured = [], []
    for i, (s, e) in enumerate(zip(systems, res)):
        decided = e["sep"] >= ref.DECIDED_SEP
        undecided += not decided
        if not s.get("near_tie", 0):
            capped_total += 1
            capped_undecided += not decided
        r = 0.0
        if decided and not (s.get("aligned") is not None and s["aligned"].all()):
            m = ref.oracle_error(orc, name, i, dict(s, real=e["real"], kappa=e["kappa"]))
            assert m is not None, "%s system %d: the ORACLE's roots differ from the exact real roots in number, or do not match them one to one" % (name, i)
            r = m[0]
            if e["num_real"]:
                measured.append(ref.round_up(r))
            if m[1]:
                print("  %s system %d: %d moved copies left out" % (name, i, m[1]), flush=True)
        elif decided:
            assert len(orc.p6l(s["lines"], s["points"], s["aligned"])) == 0
        per_system.append(ref.round_up(r))
    share = capped_undecided / capped_total
    measured.sort()
    if floor is None:
        floor = measured[int(0.9 * len(measured))]
    print("%-22s %3d systems, undecided %d (%.2f %% of the capped ones), oracle rho: median %.4g, floor (0.9 quantile) %.4g, max %.4g" %
          (name, len(systems), undecided, 100 * share, measured[len(measured) // 2], floor, measured[-1]), flush=True)
    if capped:
        assert share <= UNDECIDED_CAP, "%s: %.2f %% of the systems are undecided - change the set's inputs, not the separation or the cap" % (name, 100 * share)
    out = dict(name=name, n=len(systems), undecided_share=share, oracle_max=measured[-1], oracle_floor=floor, oracle_sys=per_system)
    if parents is not None:
        out.update(parent_set=parents[0], parent=[s["parent"] for s in systems], exp=[s["exp"] for s in systems])
        return out, res
    if full:
        out["c_full"] = [float(v) for s in systems for v in s["c"].reshape(-1)]
    elif "c" in systems[0]:
        out["c"] = [v for s in systems for v in ints(s["c"], ref.QUADRIC_UNIT)]
    else:
        out["lines"] = [v for s in systems for v in ints(s["lines"], ref.LINE_UNIT)]
        out["points"] = [v for s in systems for v in ints(s["points"], ref.POINT_UNIT)]
        out["aligned"] = "".join(str(int(v)) for s in systems for v in s["aligned"])
    for key in ("elim", "near_tie", "kind"):
        if key in systems[0]:
            out[key] = "".join(str(s[key]) for s in systems)
    if "groups" in systems[0]:
        out["groups"] = [s["groups"] for s in systems]
    out.update(num_real="".join(str(e["num_real"]) for e in res), num_finite="".join(str(e["num_finite"]) for e in res), real=[v for e in res for r in e["real"] for v in r],
               kappa=[v for e in res for v in e["kappa"]], sep=[e["sep"] for e in res])
    cplx = {str(i): e["cplx"] for i, e in enumerate(res) if "cplx" in e}
    if cplx:
        out["cplx"] = cplx
    return out, res


def check_clean(systems, res):
    """the ground-truth pose is among the reference's poses of every clean tuple, to what the grid of the file leaves of it"""
    worst = 0.0
    for s, e in zip(systems, res):
        poses = ref.poses_at(s["lines"], s["points"], np.array(e["real"]).reshape(-1, 3))
        worst = max(worst, min([np.abs(P - s["gt_pose"]).max() for P in poses] or [np.inf]))
    print("  p6l_clean: the ground truth is within %.3g of a reference pose on every tuple" % worst, flush=True)
    assert worst < 1e-4, worst


def main():
    import oracle_lib
    oracle_lib.build()
    oracle_lib.lib()
    sets = []
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        rnd = quadrics_random(np.random.default_rng(20261101))
        s, rnd_res = build_set(pool, oracle_lib, "quadrics_random", rnd)
        sets.append(s)
        sets.append(build_set(pool, oracle_lib, "quadrics_elim", quadrics_elim(np.random.default_rng(20261102)))[0])
        sets.append(build_set(pool, oracle_lib, "quadrics_degenerate", quadrics_degenerate(np.random.default_rng(20261103)))[0])
        sets.append(build_set(pool, oracle_lib, "quadrics_scaled", quadrics_scaled(np.random.default_rng(20261104), rnd), parents=("quadrics_random", rnd_res))[0])
        sets.append(build_set(pool, oracle_lib, ref.SPECIAL_SET, quadrics_special(), capped=False, floor=sets[0]["oracle_floor"], full=True)[0])
        clean = p6l_clean(np.random.default_rng(20261105))
        s, clean_res = build_set(pool, oracle_lib, "p6l_clean", clean)
        sets.append(s)
        check_clean(clean, clean_res)
        sets.append(build_set(pool, oracle_lib, "p6l_outliers", p6l_outliers(np.random.default_rng(20261106)))[0])
        sets.append(build_set(pool, oracle_lib, "p6l_degenerate_lines", p6l_degenerate_lines(np.random.default_rng(20261107)))[0])
    out = os.path.join(HERE, "p6l_golden.json")
    with open(out, "w") as f:
        json.dump({"generator": "tests/golden/gen_p6l_golden.py", "digits": 60, "decided_sep": ref.DECIDED_SEP, "sets": sets}, f, separators=(",", ":"))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
