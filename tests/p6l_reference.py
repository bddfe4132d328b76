"""Three quadrics in three unknowns and the six-line absolute pose, solved EXACTLY - TEST INFRASTRUCTURE (tests/golden/gen_p6l_golden.py mints the golden
file with it, tests/test_p6l_reference.py holds the oracle to it on the CPU, tests/test_gpu_p6l_exact.py the device's Re3q3Device and P6LDevice).

The kernel, the oracle and the reference's re3q3 all run the same elimination (the same M(X), the same octic, the same back substitution).  This module
shares none of it: a double is an exact rational, and the lexicographic Groebner basis over Q of the three quadrics has the shape form
{z - g(u), y - h(u), p(u)} in a separating variable u = x + a y + b z (a = b = 0 first, then small integers in a fixed order until the form appears).
p is the eliminant, of degree the number of FINITE roots (below 8 when roots lie at infinity); Sturm's theorem counts its real roots exactly,
mpmath.polyroots gives all of them at 60 digits, g and h give the other two unknowns.

solve_p6l eliminates the translation exactly in rationals as well: the six incidences are l_i . (R~(x, y, z) X_i + t') = 0 with R~ the unnormalised
Cayley matrix and t' = (1 + x^2 + y^2 + z^2) t; t' comes from the three lines whose 3x3 determinant is the largest (NOT the kernel's lines 0-2), the other
three incidences are the quadrics.  A rotation by 180 degrees has no Cayley parameters: it is a root at infinity of the quadrics, and neither this
reference nor the device returns it.

Per root, from the reference alone:
  sep    the smallest |r_i - r_j| / (1 + |r_i|) over the complex roots of the eliminant, conjugates included (so 2 |Im| counts)
  kappa  |J(s)^-1|_inf * max_r sum_j |c_rj| |m_j(s)|, J the Jacobian of the three quadrics at the root s, m the ten monomials
A system is DECIDED when every root has sep >= DECIDED_SEP = 1e-3: the |Im| <= 1e-8 acceptance of a double solver that works on THIS eliminant then cannot
differ from the exact real-root count.  The kernel's octic is in x, y, z or a rotated unknown, not in u: two roots apart in u can still be close in the
kernel's unknown, so for the kernel `decided` is a strong indication, not an implication; a decided system on which it miscounts is looked at, not excused."""
import json
import os
import zlib
from fractions import Fraction

import mpmath
import numpy as np

mp = mpmath.MPContext()
mp.dps = 60

DECIDED_SEP = 1e-3
EPS = 2.0 ** -52
# (a, b) of the separating variable u = x + a y + b z, in the order tried
SEPARATORS = ((0, 0), (1, 0), (0, 1), (1, 1), (1, -1), (2, 1), (1, 2), (2, -1), (-1, 2), (3, 1), (1, 3), (3, 2), (2, 3), (2, 4), (3, 5), (2, 5), (3, 7))
# exponents (x, y, z) of the device's monomial order x^2, xy, xz, y^2, yz, z^2, x, y, z, 1
MONOMIALS = ((2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))

_SYMBOLS = None


def _symbols():
    """sympy and the three symbols, imported on first use: loading the golden file needs neither"""
    global _SYMBOLS
    if _SYMBOLS is None:
        import sympy
        _SYMBOLS = (sympy,) + tuple(sympy.symbols("z y u"))
    return _SYMBOLS


def _frac(v):
    return v if isinstance(v, Fraction) else Fraction(*float(v).as_integer_ratio())


def _mpf(q):
    return mp.mpf(q.numerator) / mp.mpf(q.denominator)


def _substituted(row, a, b):
    """the quadric `row` (ten Fractions) as {(deg z, deg y, deg u): coefficient} after x = u - a y - b z"""
    x = {(0, 0, 1): Fraction(1)}
    if a:
        x[(0, 1, 0)] = Fraction(-a)
    if b:
        x[(1, 0, 0)] = Fraction(-b)
    y, z, one = {(0, 1, 0): Fraction(1)}, {(1, 0, 0): Fraction(1)}, {(0, 0, 0): Fraction(1)}

    def mul(p, q):
        out = {}
        for ep, cp in p.items():
            for eq, cq in q.items():
                e = (ep[0] + eq[0], ep[1] + eq[1], ep[2] + eq[2])
                out[e] = out.get(e, 0) + cp * cq
        return out
    out = {}
    for c, (ex, ey, ez) in zip(row, MONOMIALS):
        if c == 0:
            continue
        term = one
        for var, e in ((x, ex), (y, ey), (z, ez)):
            for _ in range(e):
                term = mul(term, var)
        for e, v in term.items():
            out[e] = out.get(e, 0) + c * v
    return {e: v for e, v in out.items() if v != 0}


def _shape_basis(rows, a, b):
    """-> (p, g, h): eliminant in u (sympy Poly over QQ), z = g(u), y = h(u); None when the lex basis is not in shape position"""
    sympy, _Z, _Y, _U = _symbols()
    polys = []
    for row in rows:
        d = _substituted(row, a, b)
        if not d:
            continue
        polys.append(sympy.Poly.from_dict({e: sympy.Rational(v.numerator, v.denominator) for e, v in d.items()}, gens=(_Z, _Y, _U), domain="QQ"))
    if len(polys) < 3:
        return None
    G = sympy.groebner(polys, _Z, _Y, _U, order="lex", domain="QQ")
    basis = [sympy.Poly(e, _Z, _Y, _U, domain="QQ") for e in G.exprs]
    if len(basis) != 3:
        return None
    by_lead = {}
    for q in basis:
        by_lead[q.monoms(order="lex")[0]] = q
    gz, hy = by_lead.get((1, 0, 0)), by_lead.get((0, 1, 0))
    p = [q for q in basis if q.degree(_Z) == 0 and q.degree(_Y) == 0]
    if gz is None or hy is None or len(p) != 1 or p[0].degree(_U) < 1:
        return None
    if gz.degree(_Y) != 0 or gz.degree(_Z) != 1 or hy.degree(_Z) != 0 or hy.degree(_Y) != 1:
        return None
    # z - g(u): every other term is free of z and y; likewise y - h(u)
    if any(m[0] or m[1] for m in gz.monoms()[1:]) or any(m[0] or m[1] for m in hy.monoms()[1:]):
        return None
    pu = sympy.Poly(p[0].as_expr(), _U, domain="QQ")
    g = sympy.Poly(-(gz.as_expr() / gz.LC() - _Z), _U, domain="QQ")
    h = sympy.Poly(-(hy.as_expr() / hy.LC() - _Y), _U, domain="QQ")
    return pu, g, h


def _horner(coeffs, x):
    v = mp.mpc(0)
    for c in coeffs:
        v = v * x + c
    return v


def monomials(s):
    x, y, z = s
    return [x * x, x * y, x * z, y * y, y * z, z * z, x, y, z, mp.mpf(1)]


def _kappa(cm, s):
    """cm: the 3x10 coefficients as mpf; s: the root"""
    x, y, z = s
    J = mp.matrix(3, 3)
    for r in range(3):
        c = cm[r]
        J[r, 0] = 2 * c[0] * x + c[1] * y + c[2] * z + c[6]
        J[r, 1] = c[1] * x + 2 * c[3] * y + c[4] * z + c[7]
        J[r, 2] = c[2] * x + c[4] * y + 2 * c[5] * z + c[8]
    m = [abs(v) for v in monomials(s)]
    size = max(sum(abs(c[j]) * m[j] for j in range(10)) for c in cm)
    try:
        Ji = mp.inverse(J)
    except ZeroDivisionError:
        return float("inf")
    norm = max(sum(abs(Ji[r, k]) for k in range(3)) for r in range(3))
    return float(norm * size)


def solve_quadrics(c):
    """c: 3x10 doubles (or Fractions) in the device's monomial order.  -> dict(
         roots      every finite complex root (x, y, z) as mpc triples at 60 digits, the real ones first, ascending in x, then by (Re u, Im u)
         num_real   the exact number of real roots (Sturm)
         num_finite the degree of the eliminant
         sep, kappa per root, in the order of `roots`
         separator  (a, b) of the u = x + a y + b z that gave the shape form
         decided    every root has sep >= DECIDED_SEP)
    None when no separator of SEPARATORS gives a shape basis (a positive-dimensional or otherwise degenerate system)."""
    rows = [[_frac(v) for v in row] for row in np.asarray(c, dtype=object).reshape(3, 10).tolist()]
    for a, b in SEPARATORS:
        shape = _shape_basis(rows, a, b)
        if shape is not None:
            break
    else:
        return None
    sympy, _Z, _Y, _U = _symbols()
    p, g, h = shape
    deg = p.degree()
    sqf = sympy.Poly(sympy.gcd(p, p.diff()), _U, domain="QQ")
    num_real = int(sympy.Poly(sympy.quo(p, sqf), _U, domain="QQ").count_roots()) if sqf.degree() > 0 else int(p.count_roots())
    pc = [_mpf(Fraction(int(q.p), int(q.q))) for q in p.all_coeffs()]
    pc = [v / pc[0] for v in pc]
    try:
        us = mp.polyroots(pc, maxsteps=500, extraprec=400)
    except mp.NoConvergence:
        us = mp.polyroots(pc, maxsteps=5000, extraprec=2000, error=False)
    us = [mp.mpc(u) for u in us]
    # the num_real roots of smallest |Im| are the real ones (exact count); with a multiple root (sep = 0 below) the split is by count alone
    order = sorted(range(deg), key=lambda k: abs(us[k].imag))
    real = set(order[:num_real]) if sqf.degree() == 0 else {k for k in range(deg) if abs(us[k].imag) <= mp.mpf(10) ** -25 * (1 + abs(us[k]))}
    us = [mp.mpc(us[k].real, 0) if k in real else us[k] for k in range(deg)]
    gc = [_mpf(Fraction(int(q.p), int(q.q))) for q in g.all_coeffs()]
    hc = [_mpf(Fraction(int(q.p), int(q.q))) for q in h.all_coeffs()]
    cm = [[_mpf(v) for v in row] for row in rows]
    def entry(k, u, conj=False):
        z, y = _horner(gc, u), _horner(hc, u)
        x = u - a * y - b * z
        if k in real:
            x, y, z = mp.mpc(x.real, 0), mp.mpc(y.real, 0), mp.mpc(z.real, 0)
        sep = min([abs(u - w) / (1 + abs(u)) for j, w in enumerate(us) if j != k] or [mp.mpf(1)])
        return dict(root=(x, y, z), u=u, sep=float(sep), kappa=_kappa(cm, (x, y, z)))
    reals = sorted((entry(k, us[k]) for k in real), key=lambda r: (float(r["root"][0].real), float(r["root"][1].real), float(r["root"][2].real)))
    upper = sorted((entry(k, us[k]) for k in range(deg) if k not in real and us[k].imag > 0), key=lambda r: (float(r["u"].real), float(r["u"].imag)))
    if len(reals) + 2 * len(upper) != deg:
        return None
    out = list(reals)
    for r in upper:                                    # a conjugate pair: the member with Im u > 0, then its conjugate
        out += [r, dict(r, root=tuple(mp.conj(v) for v in r["root"]), u=mp.conj(r["u"]))]
    return dict(roots=[r["root"] for r in out], num_real=len(reals), num_finite=deg, sep=[r["sep"] for r in out], kappa=[r["kappa"] for r in out],
                separator=(a, b), decided=all(r["sep"] >= DECIDED_SEP for r in out), sturm=num_real)


def cayley(s):
    """the unnormalised Cayley matrix R~ of (x, y, z), row-major, and 1 + x^2 + y^2 + z^2"""
    x, y, z = s
    R = [x * x - y * y - z * z + 1, 2 * x * y - 2 * z, 2 * y + 2 * x * z,
         2 * z + 2 * x * y, y * y - x * x - z * z + 1, 2 * y * z - 2 * x,
         2 * x * z - 2 * y, 2 * x + 2 * y * z, z * z - y * y - x * x + 1]
    return R, 1 + x * x + y * y + z * z


# R~ entries over the ten monomials (x^2, xy, xz, y^2, yz, z^2, x, y, z, 1)
_CAYLEY_ROWS = (
    (1, 0, 0, -1, 0, -1, 0, 0, 0, 1), (0, 2, 0, 0, 0, 0, 0, 0, -2, 0), (0, 0, 2, 0, 0, 0, 0, 2, 0, 0),
    (0, 2, 0, 0, 0, 0, 0, 0, 2, 0), (-1, 0, 0, 1, 0, -1, 0, 0, 0, 1), (0, 0, 0, 0, 2, 0, -2, 0, 0, 0),
    (0, 0, 2, 0, 0, 0, 0, -2, 0, 0), (0, 0, 0, 0, 2, 0, 2, 0, 0, 0), (-1, 0, 0, -1, 0, 1, 0, 0, 0, 1))


def _det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def p6l_quadrics(L, X):
    """-> (three quadrics as rows of ten Fractions, the 3x10 Fractions of t' over the monomials), the translation eliminated exactly; None when no three
    of the six lines are independent"""
    L = [[_frac(v) for v in row] for row in np.asarray(L, dtype=np.float64).reshape(6, 3).tolist()]
    X = [[_frac(v) for v in row] for row in np.asarray(X, dtype=np.float64).reshape(6, 3).tolist()]
    # q_i = l_i . R~ X_i over the monomials
    q = [[sum(L[i][r] * X[i][col] * _CAYLEY_ROWS[3 * r + col][j] for r in range(3) for col in range(3)) for j in range(10)] for i in range(6)]
    best, pick = Fraction(0), None
    for i0 in range(6):
        for i1 in range(i0 + 1, 6):
            for i2 in range(i1 + 1, 6):
                d = abs(_det3([L[i0], L[i1], L[i2]]))
                if d > best:
                    best, pick = d, (i0, i1, i2)
    if pick is None:
        return None
    A = [L[i] for i in pick]
    d = _det3(A)
    tp = []                                            # Cramer: t'_k = -det(A with column k replaced by the q's) / det A, per monomial
    for k in range(3):
        row = []
        for j in range(10):
            Ak = [[(q[pick[r]][j] if col == k else A[r][col]) for col in range(3)] for r in range(3)]
            row.append(-_det3(Ak) / d)
        tp.append(row)
    rest = [i for i in range(6) if i not in pick]
    quadrics = [[q[i][j] + sum(L[i][k] * tp[k][j] for k in range(3)) for j in range(10)] for i in rest]
    return quadrics, tp


def solve_p6l(L, X):
    """L: 6x3 lines, X: 6x3 points.  -> the dict of solve_quadrics on the three quadrics left after the exact elimination of t', plus
    poses: per root the 3x4 [R | t] as twelve mpc at 60 digits (row-major).  None where solve_quadrics gives None."""
    pq = p6l_quadrics(L, X)
    if pq is None:
        return None
    quadrics, tp = pq
    res = solve_quadrics(quadrics)
    if res is None:
        return None
    tpm = [[_mpf(v) for v in row] for row in tp]
    poses = []
    for s in res["roots"]:
        R, n = cayley(s)
        m = monomials(s)
        t = [sum(tpm[k][j] * m[j] for j in range(10)) / n for k in range(3)]
        poses.append([v for r in range(3) for v in (R[3 * r] / n, R[3 * r + 1] / n, R[3 * r + 2] / n, t[r])])
    res["poses"] = poses
    return res


# ---- the golden file -------------------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p6l_golden.json")
QUADRIC_SETS = ("quadrics_random", "quadrics_elim", "quadrics_degenerate", "quadrics_scaled")
P6L_SETS = ("p6l_clean", "p6l_outliers", "p6l_degenerate_lines")
SPECIAL_SET = "quadrics_special"                      # four systems written out as full doubles, see tests/golden/gen_p6l_golden.py
# the inputs of the file are whole multiples of these units, written as integers
QUADRIC_UNIT, LINE_UNIT, POINT_UNIT = 2.0 ** -13, 2.0 ** -24, 2.0 ** -20


def round_up(v, fmt="%.3e"):
    """v to four digits, never downwards: the form the file holds the oracle's error in"""
    r = float(fmt % v)
    return r if r >= v else float(fmt % (v * 1.0005))


def elim_choice(c):
    """-> (the unknown Re3q3Device eliminates: the largest of its three determinants, the first on a tie; whether it changes variables first: all three
    below 1e-10) - a restatement of csrc/p6l_device.hpp / re3q3.h:17-43 in its operation order"""
    c = np.asarray(c, dtype=np.float64).reshape(3, 10)

    def det(cols):
        m = c[:, cols].tolist()
        return abs(m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    d = [det([3, 5, 4]), det([0, 5, 2]), det([3, 0, 1])]
    elim = 0
    for k in (1, 2):
        if d[elim] < d[k]:
            elim = k
    return elim, d[elim] < 1e-10, d


def round_down(v, fmt="%.2e"):
    """v to three digits, never upwards: the form the file holds a separation in"""
    r = float(fmt % v)
    return r if r <= v else float(fmt % (v * 0.995))


def system_json(res):
    """The result of solve_quadrics / solve_p6l as the golden file holds it: the real roots rounded to double, their kappa, the SMALLEST sep of the system;
    the complex roots (nine digits, of a conjugate pair the member with Im u > 0) only where the system is undecided - on a decided one every check
    against them follows from the exact comparison with the real roots."""
    n = res["num_real"]
    out = dict(num_real=n, num_finite=res["num_finite"], real=[[float(v.real) for v in res["roots"][k]] for k in range(n)],
               kappa=[float("%.3e" % res["kappa"][k]) for k in range(n)], sep=round_down(min(res["sep"] or [1.0])))
    if out["sep"] < DECIDED_SEP:
        out["cplx"] = [float("%.9g" % f) for k in range(n, res["num_finite"], 2) for v in res["roots"][k] for f in (float(v.real), float(v.imag))]
    return out


def poses_at(lines, points, roots):
    """the poses [R | t] of the six-tuple at the given Cayley roots (doubles), evaluated at 60 digits through the exact elimination of t' and rounded to
    double: [n, 3, 4].  The file holds the roots only; a root's own rounding moves a pose entry by a few 2^-52 of its size."""
    tp = p6l_quadrics(lines, points)[1]
    tpm = [[_mpf(v) for v in row] for row in tp]
    out = np.zeros((len(roots), 3, 4))
    for k, s in enumerate(roots):
        s = [mp.mpf(float(v)) for v in s]
        R, n = cayley(s)
        m = monomials(s)
        for r in range(3):
            out[k, r, :3] = [float(R[3 * r + c] / n) for c in range(3)]
            out[k, r, 3] = float(sum(tpm[r][j] * m[j] for j in range(10)) / n)
    return out


def load_golden(path=GOLDEN):
    """tests/golden/p6l_golden.json as {set name: set}; a set's `systems` is a list of dicts: the inputs (`c` 3x10, or `lines`, `points` 6x3 and `aligned`),
    `num_real`, `num_finite`, `real` [n, 3], `kappa` [n], `sep` (the system's smallest), `decided`, for P6L `poses` [n, 3, 4] (poses_at the real roots),
    `roots` [num_finite, 3] complex with the conjugates restored where the system is undecided (else None), and the set's own labels (`elim`, `near_tie`,
    `kind`, `groups`, `parent`, `exp`).  A system of quadrics_scaled holds its parent's index and the three row exponents; its roots and kappa are its
    parent's (the generator asserts the identity of the roots for every one of them; the conditioning of a root does not depend on the scale of a row, while
    kappa's formula, with the largest row's size, would grow by up to 2^80).  Per system `oracle_rho`, the oracle's largest normalised error on it; per set
    `oracle_floor`, the nine-tenths quantile of those."""
    with open(path) as f:
        g = json.load(f)
    out = {}
    for s in g["sets"]:
        n = s["n"]
        if "parent" in s:
            src = out[s["parent_set"]]["systems"]
            systems = [dict(src[p], c=src[p]["c"] * (2.0 ** np.array(e, dtype=np.float64))[:, None], parent=p, exp=e) for p, e in zip(s["parent"], s["exp"])]
            for i, e in enumerate(systems):           # roots and kappa are the parent's; the oracle's error is the system's own
                e["oracle_rho"] = s["oracle_sys"][i]
        else:
            nr, real, kappa = [int(ch) for ch in s["num_real"]], np.array(s["real"], dtype=np.float64).reshape(-1, 3), np.array(s["kappa"], dtype=np.float64)
            at = np.concatenate([[0], np.cumsum(nr)])
            systems = []
            for i in range(n):
                e = dict(num_real=nr[i], num_finite=int(s["num_finite"][i]), real=real[at[i]:at[i + 1]], kappa=kappa[at[i]:at[i + 1]], sep=s["sep"][i], roots=None)
                e["decided"] = e["sep"] >= g["decided_sep"]
                e["oracle_rho"] = s["oracle_sys"][i]
                if "c_full" in s:
                    e["c"] = np.array(s["c_full"][30 * i: 30 * i + 30], dtype=np.float64).reshape(3, 10)
                elif "c" in s:
                    e["c"] = np.array(s["c"][30 * i: 30 * i + 30], dtype=np.float64).reshape(3, 10) * QUADRIC_UNIT
                else:
                    e["lines"] = np.array(s["lines"][18 * i: 18 * i + 18], dtype=np.float64).reshape(6, 3) * LINE_UNIT
                    e["points"] = np.array(s["points"][18 * i: 18 * i + 18], dtype=np.float64).reshape(6, 3) * POINT_UNIT
                    e["aligned"] = np.array([int(ch) for ch in s["aligned"][6 * i: 6 * i + 6]], dtype=np.uint8)
                    e["poses"] = poses_at(e["lines"], e["points"], e["real"])
                for key in ("elim", "near_tie", "kind"):
                    if key in s:
                        e[key] = int(s[key][i])
                if "groups" in s and s["groups"][i] != "-":
                    e["groups"] = [int(ch) for ch in s["groups"][i]]
                cp = s.get("cplx", {}).get(str(i))
                if cp is not None:
                    z = np.array(cp, dtype=np.float64).reshape(-1, 3, 2)
                    z = z[..., 0] + 1j * z[..., 1]
                    e["roots"] = np.concatenate([e["real"].astype(np.complex128), z, z.conj()])
                    assert len(e["roots"]) == e["num_finite"]
                systems.append(e)
        s["systems"] = systems
        out[s["name"]] = s
    return out


def match(got, want):
    """one-to-one assignment of the rows of `got` to rows of `want` (nearest first, in |.|_inf): -> index into want per row of got, or None when two rows
    of got claim the same row of want"""
    got, want = np.asarray(got), np.asarray(want)
    used, idx = set(), []
    for r in got:
        d = np.abs(want - r).reshape(len(want), -1).max(axis=1)
        k = int(np.argmin(d))
        if k in used:
            return None
        used.add(k)
        idx.append(k)
    return idx


def root_rho(got, want, kappa):
    """|s - s*|_inf / (2^-52 kappa (1 + |s*|_inf)), the normalised error of one root"""
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / (EPS * kappa * (1.0 + np.abs(want).max())))


def pose_rho(got, want, kappa, root):
    """the same for the twelve pose entries, normalised by the root's kappa and size"""
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / (EPS * kappa * (1.0 + np.abs(root).max())))


ORACLE_DRAWS = 32


def oracle_error(orc, name, i, e):
    """The yardstick of one decided system: the largest normalised error of the CPU oracle (module oracle_lib) against the real roots e["real"] (kappa
    e["kappa"]) over the system itself and ORACLE_DRAWS copies with every input moved by one unit in the last place, up or down (fixed seed per system).
    Two double implementations of one elimination differ by such backward perturbations; the elimination amplifies them by a factor that belongs to the
    system, and ONE run of the oracle may sit far below that factor by luck.  The exact roots of a copy differ from the system's by kappa roundings, a few
    units of this measure.  -> None when the oracle's count on the system itself differs from the exact one or its results do not match one to one; a
    copy on which that happens is left out (-> rho, copies left out)."""
    rng = np.random.default_rng([zlib.crc32(name.encode()), i])
    quadrics = "c" in e
    real, kappa = np.asarray(e["real"], dtype=np.float64).reshape(-1, 3), e["kappa"]
    want = real if quadrics else poses_at(e["lines"], e["points"], real).reshape(-1, 12)
    rho, left_out = 0.0, 0
    for draw in range(ORACLE_DRAWS + 1):
        def moved(a):
            a = np.asarray(a, dtype=np.float64)
            return a if draw == 0 else np.nextafter(a, np.where(rng.integers(0, 2, a.shape) == 1, np.inf, -np.inf))
        if quadrics:
            got = orc.re3q3(moved(e["c"])).T
        else:
            got = orc.p6l(moved(e["lines"]), moved(e["points"]), e["aligned"]).reshape(-1, 12)
        idx = match(got, want) if len(got) == len(want) else None
        if idx is None:
            if draw == 0:
                return None
            left_out += 1
            continue
        for k, j in enumerate(idx):
            rho = max(rho, root_rho(got[k], want[j], kappa[j]) if quadrics else pose_rho(got[k], want[j], kappa[j], real[j]))
    return rho, left_out
