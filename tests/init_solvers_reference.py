"""The initialisation solvers of K6 as mathematical functions at 50 digits - TEST INFRASTRUCTURE (tests/golden/gen_init_solvers_golden.py mints the golden
file with it, tests/test_init_solvers_reference.py holds the oracle to it on the CPU, tests/test_gpu_init_solvers_exact.py the device's
k_fourview2d_minimal, k_pose2d_solve, k_planar_solve, k_fourview2d_evaluate and k_fourview2d_errors_stored).

The kernels and the oracle take every null vector from the Gram matrix A^T A by cyclic Jacobi in double.  This module shares none of that arithmetic: a
double enters as the exact number it is, every operation runs in mpmath at 50 digits, and a singular vector comes from a singular value decomposition of A
ITSELF (mpmath's svd_r), so neither an error the two double implementations share nor the cost of squaring the conditioning can hide in it.  What is
computed is the function the reference defines (FourView2dEstimator::MinimalSolver with factorize_trifocal_tensor, metric_upgrade and AbsPoseSolver,
AbsolutePose2dEstimator::NonMinimalSolver, PlanarOffsetEstimator::MinimalSolver up to the offsets, three_view_triangulate2d with
FourView2dEstimator::EvaluateModelOnPoint), stated from its equations: the trilinear incidence, the quadratic of the factorisation, the seven equations of the
third camera, the least-squares upgrade, the pose of the fourth camera.

Per result, from the reference alone:
  K        for a null vector lambda_max / (lambda_1 - lambda_0) of the spectrum of A^T A (the squares of A's singular values): the factor by which a
           rounding of the Gram matrix turns the vector.  Four-view: per root of the quadratic the larger of the trifocal system's and that root's 7x6
           system's.  A track: lambda_max / lambda_min of its 2x2 normal matrix.  Planar offsets: max_c sum_i |A^+[c, i]| cond_i s_i / max(1, |t|_inf),
           A^+ the pseudo-inverse of the final system, cond_i the infinity-norm condition of track i's 3x3 solve, s_i = |A_i| |t| + |b_i| the size of
           its equation - the first-order bound on what roundings of the per-track solves do to the offsets.  (The product of the final 3x3 matrix's
           condition - A for three tracks, A^T A for more - and the WORST track's condition was tried first and is kept in the file as `cond`: it
           charges every equation with the worst track's amplification and the solution with the normal matrix's condition, which the reference's and
           the oracle's QR of A does not pay; the oracle's normalised errors then spread over a factor 1800 between their 10 % and 90 % quantiles on
           exact data with ten tracks, 750 with noise.  With the bound above they spread over a factor 6 to 8 in all four sets.)
  decided  no branch of the function is within rounding of its threshold: |beta| >= 1e-6 sqrt(beta^2 + |4 alpha gamma|), |disc| >= 1e-6 (beta^2 +
           |4 alpha gamma|), every value whose sign is tested (the chirality of the first sample point, the depth of a track in a view) at least 1e-6 of
           the sum of the magnitudes of its terms, and 2^-52 K <= 1e-3.

The normalised error of a result is rho = max|got - want| / (max(1, max|want|) 2^-52 K).

The sign of a null vector is not part of the function.  The trifocal vector's changes nothing (alpha, beta, gamma are quadratic in it, the 7x6 system is
linear in it).  The third camera's negates that camera, which the upgrade leaves negated: within a root candidate k becomes candidate k ^ 1 (flip3).
fourview_rho allows exactly that exchange, the same for all eight candidates of a root, and nothing else.  The fourth camera depends on the first three
through the triangulated sample points only, and a least-squares point does not change when a camera is negated: of the sixteen fourth cameras the four
that share a root and flip1 are one and the same, and the golden file holds each once (the generator asserts the identity at 1e-45)."""
import base64
import json
import os
import zlib

import mpmath
import numpy as np

mp = mpmath.MPContext()
mp.dps = 50

EPS = 2.0 ** -52
DECIDED_REL = 1e-6
DECIDED_COND = 1e-3
ORACLE_DRAWS = 32
FACTOR = 4.0


def _m(v):
    return mp.mpf(float(v))


def _vec(a):
    return [_m(v) for v in np.asarray(a, dtype=np.float64).reshape(-1)]


def _dot(a, b):
    return mp.fsum(p * q for p, q in zip(a, b))


def null_vector(rows):
    """rows: m lists of k numbers.  -> (the unit right singular vector of the smallest singular value, K, the k eigenvalues of the Gram matrix descending).
    Fewer rows than columns are filled up with zero rows (the missing singular values are exact zeros)."""
    k = len(rows[0])
    A = mp.matrix(max(len(rows), k), k)
    for i, r in enumerate(rows):
        for j in range(k):
            A[i, j] = r[j]
    _, S, V = mp.svd_r(A)
    order = sorted(range(k), key=lambda i: -S[i])
    lam = [S[i] * S[i] for i in order]
    v = [V[order[-1], j] for j in range(k)]
    nr = mp.sqrt(_dot(v, v))
    gap = lam[-2] - lam[-1]
    return [e / nr for e in v], (float(lam[0] / gap) if gap > 0 else float("inf")), lam


def gram_residual(rows, v):
    """|A^T A v - (v^T A^T A v) v|_inf / lambda_max-free scale: the defining equation of the null vector (for exact data simply |A^T A v|)"""
    k = len(v)
    Av = [_dot(r, v) for r in rows]
    g = [mp.fsum(rows[i][j] * Av[i] for i in range(len(rows))) for j in range(k)]
    lam = _dot(g, v)
    return max(abs(g[j] - lam * v[j]) for j in range(k))


def _rel(value, terms):
    """|value| as a share of the summed magnitude of its terms"""
    s = mp.fsum(abs(t) for t in terms)
    return float(abs(value) / s) if s > 0 else 0.0


def _lsq2(rows, b):
    """least squares of an m x 2 system -> (x0, x1), the 2x2 normal matrix (n00, n01, n11)"""
    n00 = mp.fsum(r[0] * r[0] for r in rows); n01 = mp.fsum(r[0] * r[1] for r in rows); n11 = mp.fsum(r[1] * r[1] for r in rows)
    q0 = mp.fsum(r[0] * v for r, v in zip(rows, b)); q1 = mp.fsum(r[1] * v for r, v in zip(rows, b))
    det = n00 * n11 - n01 * n01
    return [(n11 * q0 - n01 * q1) / det, (n00 * q1 - n01 * q0) / det], (n00, n01, n11)


def triangulate3(cams, xs):
    """the least-squares point of three views: cams three 2x3 (lists of lists), xs three bearings.  Row j: x_a P_j[1, :2] - x_b P_j[0, :2], right side
    x_b P_j[0, 2] - x_a P_j[1, 2] (the point's image is parallel to the bearing).  -> (X, normal matrix)"""
    rows, b = [], []
    for P, (xa, xb) in zip(cams, xs):
        rows.append([xa * P[1][0] - xb * P[0][0], xa * P[1][1] - xb * P[0][1]])
        b.append(xb * P[0][2] - xa * P[1][2])
    return _lsq2(rows, b)


def abs_pose(x4, X):
    """the fourth camera [a -b t0; b a t1] from bearings x4 and points X (lists of pairs), the first point in front.
    -> (a, b, t0, t1), the chirality value as a share of its terms, the residual of the defining equation"""
    A = [[P[0] * x[1] - P[1] * x[0], -P[0] * x[0] - P[1] * x[1]] for x, P in zip(x4, X)]
    B = [[x[1], -x[0]] for x in x4]
    b00 = mp.fsum(r[0] * r[0] for r in B); b01 = mp.fsum(r[0] * r[1] for r in B); b11 = mp.fsum(r[1] * r[1] for r in B)
    det = b00 * b11 - b01 * b01
    inv = [[b11 / det, -b01 / det], [-b01 / det, b00 / det]]
    BtA = [[mp.fsum(B[i][r] * A[i][c] for i in range(len(A))) for c in range(2)] for r in range(2)]
    C = [[-(inv[r][0] * BtA[0][c] + inv[r][1] * BtA[1][c]) for c in range(2)] for r in range(2)]
    M = [[A[i][c] + B[i][0] * C[0][c] + B[i][1] * C[1][c] for c in range(2)] for i in range(len(A))]
    ab, _, _ = null_vector(M)
    t = [C[0][0] * ab[0] + C[0][1] * ab[1], C[1][0] * ab[0] + C[1][1] * ab[1]]
    terms = [ab[1] * X[0][0], ab[0] * X[0][1], t[1]]
    front = mp.fsum(terms)
    out = [ab[0], ab[1], t[0], t[1]]
    if front < 0:
        out = [-v for v in out]
    return out, _rel(front, terms), gram_residual(M, ab)


# the seven equations G d = 0 of the third camera's entries d, as (row, column, [(tensor entry, camera-2 entry, sign)]): camera 2 is [a1 b1 c1; a2 b2 c2]
_G = ((0, 1, ((7, "c2", 1),)), (0, 2, ((0, "c1", -1),)), (0, 4, ((0, "b1", 1),)), (0, 5, ((7, "a2", -1),)),
      (1, 2, ((1, "c1", -1),)), (1, 3, ((7, "c2", 1),)), (1, 4, ((1, "b1", 1),)), (1, 5, ((7, "b2", -1),)),
      (2, 1, ((7, "c1", -1),)), (2, 2, ((2, "c1", -1),)), (2, 4, ((2, "b1", 1),)), (2, 5, ((7, "a1", 1),)),
      (3, 2, ((3, "c1", -1),)), (3, 3, ((7, "c1", -1),)), (3, 4, ((3, "b1", 1),)), (3, 5, ((7, "b1", 1),)),
      (4, 0, ((7, "c2", -1),)), (4, 2, ((4, "c1", -1),)), (4, 4, ((7, "a2", 1), (4, "b1", 1))),
      (5, 2, ((5, "c1", -1), (7, "c2", -1))), (5, 4, ((7, "b2", 1), (5, "b1", 1))),
      (6, 0, ((7, "c1", 1),)), (6, 2, ((6, "c1", -1),)), (6, 4, ((7, "a1", -1), (6, "b1", 1))))


def _matmul(A, B):
    return [[mp.fsum(A[r][k] * B[k][c] for k in range(len(B))) for c in range(len(B[0]))] for r in range(len(A))]


def fourview2d_minimal(x, sample, frames, only_k=False):
    """x: [4, n, 2] unit bearings (doubles), sample: track indices, frames: the three 2x2 changes of image coordinates, row-major (12 doubles).
    -> dict(count 0 or 16, cams: 16 x 4 cameras (2x3 lists of mpf) or None, pre: per root [camera 2, camera 3] before the flips, cam4: per root and flip1 the
    fourth camera (a, b, t0, t1), K: per root, K_tri, K_third: per root, decided, margins: the smallest share met per kind of decision, residual: the largest
    residual of a defining equation).  Candidate 8 root + 4 flip1 + 2 flip2 + flip3.  only_k stops after K and the decisions of the quadratic."""
    x = np.asarray(x, dtype=np.float64)
    fr = _vec(frames)
    A1, A2, A3 = ([[fr[4 * k], fr[4 * k + 1]], [fr[4 * k + 2], fr[4 * k + 3]]] for k in range(3))
    bear = [[[_m(x[j, s, 0]), _m(x[j, s, 1])] for s in sample] for j in range(4)]
    rows = []
    for i in range(len(sample)):
        mono = [bear[0][i][e & 1] * bear[1][i][(e >> 1) & 1] * bear[2][i][e >> 2] for e in range(8)]
        # sum_abc T[a + 2b + 4c] x1_a x2_b x3_c = 0 with the calibration T[0] = t1 + t3 + t4, T[1] = t5 - t0 - t2, T[k + 2] = t_k
        row = [mono[k + 2] for k in range(6)]
        for k in (1, 3, 4):
            row[k] += mono[0]
        row[5] += mono[1]; row[0] -= mono[1]; row[2] -= mono[1]
        rows.append(row)
    t, K_tri, _ = null_vector(rows)
    residual = gram_residual(rows, t)
    T = [t[1] + t[3] + t[4], t[5] - t[0] - t[2]] + list(t)
    AT = [mp.fsum(A1[f & 1][e & 1] * A2[(f >> 1) & 1][(e >> 1) & 1] * A3[f >> 2][e >> 2] * T[f] for f in range(8)) for e in range(8)]
    alpha = AT[2] * AT[7] - AT[3] * AT[6]
    beta_terms = [AT[1] * AT[6], AT[3] * AT[4], -AT[0] * AT[7], -AT[2] * AT[5]]
    beta = mp.fsum(beta_terms)
    gamma = AT[0] * AT[5] - AT[1] * AT[4]
    disc = beta * beta - 4 * alpha * gamma
    size = beta * beta + abs(4 * alpha * gamma)
    margins = dict(beta=float(abs(beta) / mp.sqrt(size)), disc=float(abs(disc) / size), chirality=1.0)
    out = dict(K_tri=K_tri, margins=margins, residual=residual, beta_positive=bool(beta > 0))
    if disc < 0:
        out.update(count=0, cams=None, pre=None, cam4=None, K=[K_tri, K_tri], K_third=[0.0, 0.0])
        out["decided"] = margins["beta"] >= DECIDED_REL and margins["disc"] >= DECIDED_REL and EPS * K_tri <= DECIDED_COND
        return out
    sq = mp.sqrt(disc)
    aa0 = 2 * gamma / (-beta - sq) if beta > 0 else 2 * gamma / (-beta + sq)       # the root of alpha a^2 + beta a + gamma free of cancellation, then the other
    aa = [aa0, gamma / (alpha * aa0)]
    A1det = A1[0][0] * A1[1][1] - A1[0][1] * A1[1][0]
    A1inv = [[A1[1][1] / A1det, -A1[0][1] / A1det], [-A1[1][0] / A1det, A1[0][0] / A1det]]
    pre, K_third, thirds = [], [], []
    for root in range(2):
        sn = mp.sqrt(1 + aa[root] * aa[root])
        c2 = dict(a1=aa[root] / sn, a2=1 / sn)
        rho = -(AT[1] * c2["a2"] - AT[3] * c2["a1"]) / (AT[2] * c2["a1"] - AT[0] * c2["a2"])
        c2.update(b1=rho * c2["a1"], b2=rho * c2["a2"], c1=-c2["a2"], c2=c2["a1"])
        G = [[mp.mpf(0)] * 6 for _ in range(7)]
        for r, c, terms in _G:
            G[r][c] = mp.fsum(sign * AT[k] * c2[name] for k, name, sign in terms)
        d, Kg, _ = null_vector(G)
        residual = max(residual, gram_residual(G, d))
        K_third.append(Kg)
        thirds.append((c2, d))
    out.update(K_third=K_third, K=[max(K_tri, k) for k in K_third])
    if only_k:
        out["decided"] = margins["beta"] >= DECIDED_REL and margins["disc"] >= DECIDED_REL and EPS * max(out["K"]) <= DECIDED_COND
        return out
    cams, cam4 = [], []
    x4 = bear[3]
    for root in range(2):
        c2, d = thirds[root]
        P = []
        for Af, Q in ((A2, [[c2["a1"], c2["b1"], c2["c1"]], [c2["a2"], c2["b2"], c2["c2"]]]), (A3, [[d[0], d[2], d[4]], [d[1], d[3], d[5]]])):
            M = _matmul(Af, Q)                          # back to the image's own coordinates, the first camera back to [I 0]
            L = _matmul([r[:2] for r in M], A1inv)
            P.append([[L[r][0], L[r][1], M[r][2]] for r in range(2)])
        # metric upgrade: H = [1 0 0; 0 1 0; h0 h1 1] with P H calibrated ([p -q; q p] blocks) in the least-squares sense
        ur, ub = [], []
        for Q in P:
            ur += [[Q[0][2], -Q[1][2]], [Q[1][2], Q[0][2]]]
            ub += [Q[1][1] - Q[0][0], -Q[0][1] - Q[1][0]]
        h, _ = _lsq2(ur, ub)
        P = [[[Q[r][0] + Q[r][2] * h[0], Q[r][1] + Q[r][2] * h[1], Q[r][2]] for r in range(2)] for Q in P]
        for v in range(2):
            nr = mp.sqrt(P[v][0][0] ** 2 + P[v][1][0] ** 2)
            P[v] = [[e / nr for e in r] for r in P[v]]
        sc = mp.sqrt(P[0][0][2] ** 2 + P[0][1][2] ** 2)
        P = [[[r[0], r[1], r[2] / sc] for r in Q] for Q in P]
        if len(sample) == 5:                            # a minimal sample's tensor is a calibrated one: both cameras come out as [p -q; q p], p^2 + q^2 = 1
            residual = max([residual] + [max(abs(Q[0][0] - Q[1][1]), abs(Q[0][1] + Q[1][0])) for Q in P])
        pre.append(P)
        per_flip1 = []
        for flips in range(8):
            f1, f2, f3 = flips & 4, flips & 2, flips & 1
            c = [[[mp.mpf(1), mp.mpf(0), mp.mpf(0)], [mp.mpf(0), mp.mpf(1), mp.mpf(0)]], [list(r) for r in P[0]], [list(r) for r in P[1]]]
            if f1:
                for v in (1, 2):
                    for r in range(2):
                        c[v][r][2] = -c[v][r][2]
            if f2:
                c[1] = [[-e for e in r] for r in c[1]]
            if f3:
                c[2] = [[-e for e in r] for r in c[2]]
            Xs = [triangulate3(c, [bear[j][i] for j in range(3)])[0] for i in range(len(sample))]
            p4, share, res4 = abs_pose(x4, Xs)
            margins["chirality"] = min(margins["chirality"], share)
            residual = max(residual, res4)
            if not (f2 or f3):
                per_flip1.append(p4)
            else:                                       # the same fourth camera as the candidate without flip2 and flip3
                residual = max(residual, max(abs(u - w) for u, w in zip(p4, per_flip1[-1])))
            c.append([[p4[0], -p4[1], p4[2]], [p4[1], p4[0], p4[3]]])
            cams.append(c)
        cam4.append(per_flip1)
    out.update(count=16, cams=cams, pre=pre, cam4=cam4, residual=residual)
    out["decided"] = all(margins[k] >= DECIDED_REL for k in margins) and EPS * max(out["K"]) <= DECIDED_COND
    return out


def pose2d(x, X, sample):
    """x: [n, 2] unit bearings, X: [n, 2] points.  The pose [a -b t0; b a t1] whose (a, b, t0, t1) is the null vector of the rows
    [X1 x2 - X2 x1, -X1 x1 - X2 x2, x2, -x1], scaled to a^2 + b^2 = 1, the first sample point in front.  -> dict(pose 2x3, K, decided, margin, residual)"""
    rows = []
    for s in sample:
        x1, x2, X1, X2 = _m(x[s][0]), _m(x[s][1]), _m(X[s][0]), _m(X[s][1])
        rows.append([X1 * x2 - X2 * x1, -X1 * x1 - X2 * x2, x2, -x1])
    t, K, _ = null_vector(rows)
    residual = gram_residual(rows, t)
    nr = mp.sqrt(t[0] * t[0] + t[1] * t[1])
    t = [v / nr for v in t]
    X0 = [_m(X[sample[0]][0]), _m(X[sample[0]][1])]
    terms = [t[1] * X0[0], t[0] * X0[1], t[3]]
    front = mp.fsum(terms)
    if front < 0:
        t = [-v for v in t]
    margin = _rel(front, terms)
    return dict(pose=[[t[0], -t[1], t[2]], [t[1], t[0], t[3]]], K=K, margin=margin, residual=residual,
                decided=margin >= DECIDED_REL and EPS * K <= DECIDED_COND)


def _cond_inf(M):
    return float(mp.mnorm(M, mp.inf) * mp.mnorm(mp.inverse(M), mp.inf))


def planar_offsets(scene, sample):
    """scene: dict(poses [4, 3, 4] with t_y = 0, lines [4, n, 3], Rg [4, 3, 3]).  Per track of the sample: with lg_j = Rg_j l_j, the point is
    X = Rg_0^T A0^-1 (B0 (t_y1, t_y2, t_y3, 1)), A0 rows lg_j^T R_j, B0 rows (lg_j[1] e_j, lg_j[0] t_jx + lg_j[2] t_jz), j = 1..3; its incidence with the
    line of view 0 is one linear equation in the three offsets.  Three tracks: the solution; more: the least-squares solution.
    -> dict(offsets [3], K, cond_final, cond_track, decided, residual)"""
    poses = [[[_m(v) for v in r] for r in P] for P in np.asarray(scene["poses"], dtype=np.float64).reshape(4, 3, 4)]
    Rg = [[[_m(v) for v in r] for r in R] for R in np.asarray(scene["Rg"], dtype=np.float64).reshape(4, 3, 3)]
    lines = np.asarray(scene["lines"], dtype=np.float64)
    A, b, cond_track, conds = [], [], 0.0, []
    for s in sample:
        A0, B0 = mp.matrix(3, 3), mp.matrix(3, 4)
        for j in (1, 2, 3):
            l = _vec(lines[j][s])
            lg = [_dot(Rg[j][r], l) for r in range(3)]
            for c in range(3):
                A0[j - 1, c] = mp.fsum(lg[r] * poses[j][r][c] for r in range(3))
            B0[j - 1, j - 1] = lg[1]
            B0[j - 1, 3] = lg[0] * poses[j][0][3] + lg[2] * poses[j][2][3]
        conds.append(_cond_inf(A0))
        cond_track = max(cond_track, conds[-1])
        S = mp.inverse(A0) * B0
        RB = mp.matrix(Rg[0]).T * S
        l0 = _vec(lines[0][s])
        A.append([mp.fsum(l0[r] * RB[r, c] for r in range(3)) for c in range(3)])
        b.append(-mp.fsum(l0[r] * RB[r, 3] for r in range(3)))
    if len(sample) == 3:
        M, rhs = mp.matrix(A), mp.matrix(b)
    else:
        M = mp.matrix([[mp.fsum(r[i] * r[j] for r in A) for j in range(3)] for i in range(3)])
        rhs = mp.matrix([mp.fsum(r[i] * v for r, v in zip(A, b)) for i in range(3)])
    tt = mp.inverse(M) * rhs
    tt = [tt[i] for i in range(3)]
    # the defining equation: the normal equations A^T (A t - b) = 0 (for three tracks A t = b itself)
    res = [_dot(r, tt) - v for r, v in zip(A, b)]
    residual = max(abs(v) for v in res) if len(sample) == 3 else max(abs(mp.fsum(A[i][c] * res[i] for i in range(len(A)))) for c in range(3))
    cond_final = _cond_inf(M)
    # first-order perturbation: row i of (A, b) comes out of its own 3x3 solve, known to 2^-52 cond_i of its size s_i = |A_i| |t| + |b_i|; the solution
    # moves by the pseudo-inverse times these
    pinv = mp.inverse(M) if len(sample) == 3 else mp.inverse(M) * mp.matrix(A).T
    size = [mp.fsum(abs(A[i][c]) * abs(tt[c]) for c in range(3)) + abs(b[i]) for i in range(len(A))]
    K = float(max(mp.fsum(abs(pinv[c, i]) * conds[i] * size[i] for i in range(len(A))) for c in range(3)) / max(1, max(abs(v) for v in tt)))
    return dict(offsets=tt, K=K, cond_final=cond_final, cond_track=cond_track, residual=residual, decided=EPS * K <= DECIDED_COND)


def _projection(cams, X, xs):
    """per view: (1D error |x_a / x_b - z_0 / z_1|, depth z_1 as a share of its terms, the size of the terms the error is rounded in)"""
    out = []
    for P, (xa, xb) in zip(cams, xs):
        t0 = [P[0][0] * X[0], P[0][1] * X[1], P[0][2]]
        t1 = [P[1][0] * X[0], P[1][1] * X[1], P[1][2]]
        z0, z1 = mp.fsum(t0), mp.fsum(t1)
        m0, m1 = mp.fsum(abs(v) for v in t0), mp.fsum(abs(v) for v in t1)
        scale = abs(xa / xb) + m0 / abs(z1) + abs(z0 / z1) * m1 / abs(z1)
        out.append((abs(xa / xb - z0 / z1), z1, _rel(z1, t1), scale))
    return out


def fourview2d_errors_at(cams, x, X, i):
    """the error of track i of the model (cams [4, 2, 3], the point X given): the largest 1D error over the four views, 1e6 when the point is behind a view.
    -> (err, scale: the size of the terms the error is rounded in, the smallest depth share)"""
    cm = [[[_m(v) for v in r] for r in P] for P in np.asarray(cams, dtype=np.float64).reshape(4, 2, 3)]
    xs = [[_m(x[j][i][0]), _m(x[j][i][1])] for j in range(4)]
    pr = _projection(cm, [_m(X[0]), _m(X[1])], xs)
    err = mp.mpf(1000000) if any(p[1] < 0 for p in pr) else max(p[0] for p in pr)
    return err, float(max(p[3] for p in pr)), min(p[2] for p in pr)


def fourview2d_track(cams, x, i):
    """the three-view least-squares point of track i and its error in the four views -> dict(X [2], err, K, decided, margin)"""
    cm = [[[_m(v) for v in r] for r in P] for P in np.asarray(cams, dtype=np.float64).reshape(4, 2, 3)]
    xs = [[_m(x[j][i][0]), _m(x[j][i][1])] for j in range(4)]
    X, (n00, n01, n11) = triangulate3(cm[:3], xs[:3])
    half, mid = mp.sqrt(((n00 - n11) / 2) ** 2 + n01 * n01), (n00 + n11) / 2
    K = float((mid + half) / (mid - half))
    pr = _projection(cm, X, xs)
    err = mp.mpf(1000000) if any(p[1] < 0 for p in pr) else max(p[0] for p in pr)
    margin = min(p[2] for p in pr)
    return dict(X=X, err=err, K=K, margin=margin, decided=margin >= DECIDED_REL and EPS * K <= DECIDED_COND)


# ---- comparison ----------------------------------------------------------------------------------------------------------------------------------------
def rho(got, want, K):
    """max|got - want| / (max(1, max|want|) 2^-52 K)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    d = np.abs(got - want).max()
    if not np.isfinite(d):
        return float("inf")
    return float(d / (max(1.0, np.abs(want).max()) * EPS * K))


def candidates(pre, cam4):
    """the sixteen candidates [16, 4, 2, 3] from the file's content: pre [2 roots, 2 cameras, 2, 3] before the flips, cam4 [2 roots, 2 flip1, 4] as
    (a, b, t0, t1).  flip1 negates the translations of cameras 2 and 3, flip2 camera 2, flip3 camera 3; flip1 is the outermost."""
    pre, cam4 = np.asarray(pre, dtype=np.float64), np.asarray(cam4, dtype=np.float64)
    out = np.zeros((16, 4, 2, 3))
    for root in range(2):
        for flips in range(8):
            c = out[8 * root + flips]
            c[0] = [[1, 0, 0], [0, 1, 0]]
            c[1], c[2] = pre[root, 0], pre[root, 1]
            if flips & 4:
                c[1:3, :, 2] *= -1.0
            if flips & 2:
                c[1] *= -1.0
            if flips & 1:
                c[2] *= -1.0
            a, b, t0, t1 = cam4[root, (flips >> 2) & 1]
            c[3] = [[a, -b, t0], [b, a, t1]]
    return out


def fourview_rho(got, want, K):
    """got, want: [16, 4, 2, 3]; K: per root.  Candidate by candidate in order; per root the better of `as is` and `k <-> k ^ 1 for all eight`.
    -> (the largest rho over the sixteen candidates, the exchange taken per root)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    worst, taken = 0.0, []
    for root in range(2):
        per = []
        for swap in (0, 1):
            per.append(max(rho(got[8 * root + k], want[8 * root + (k ^ swap)], K[root]) for k in range(8)))
        taken.append(int(per[1] < per[0]))
        worst = max(worst, min(per))
    return worst, taken


def moved(a, rng, draw):
    """a itself (draw 0) or a copy with every entry moved by one unit in the last place, up or down"""
    a = np.asarray(a, dtype=np.float64)
    return a if draw == 0 else np.nextafter(a, np.where(rng.integers(0, 2, a.shape) == 1, np.inf, -np.inf))


def draws(name, i):
    """the sample itself and ORACLE_DRAWS copies of its inputs moved by one unit in the last place (fixed seed per sample): the yardstick of a sample is the
    oracle's largest error over these, in the form of tests/p6l_reference.py's oracle_error - two double implementations of one function differ by such
    backward perturbations (the device's constructors alone renormalise every bearing), and ONE run of the oracle may sit far below what the sample's
    conditioning allows by luck"""
    rng = np.random.default_rng([zlib.crc32(name.encode()), i])
    for draw in range(ORACLE_DRAWS + 1):
        yield draw, rng


def oracle_fourview_rho(orc, name, i, x, sample, frames, e):
    """-> the oracle's largest fourview_rho over the draws; None when its count differs from the reference's on any draw"""
    worst = 0.0
    for draw, rng in draws(name, i):
        cams, cnt = orc.fourview2d_minimal(moved(x, rng, draw), np.asarray(sample, dtype=np.int32)[None], frames)
        if cnt[0] != e["count"]:
            return None
        if cnt[0]:
            worst = max(worst, fourview_rho(cams[0], e["cams"], e["K"])[0])
    return worst


def oracle_pose2d_rho(orc, name, i, x, X, sample, e):
    return max(rho(orc.abspose2d_nonminimal(moved(x, rng, draw), moved(X, rng, draw), sample), e["pose"], e["K"]) for draw, rng in draws(name, i))


def oracle_planar_rho(orc, name, i, scene, sample, e):
    worst = 0.0
    for draw, rng in draws(name, i):
        sc = dict(scene, lines=moved(scene["lines"], rng, draw))
        worst = max(worst, rho(orc.planar_minimal(sc, np.asarray(sample, dtype=np.int32)[None])[0], e["offsets"], e["K"]))
    return worst


def oracle_track_rho(orc, name, cams, x, tracks):
    """per track the oracle's largest rho of (X0, X1, err) over the draws (all tracks at once per draw)"""
    worst = np.zeros(len(tracks))
    for draw, rng in draws(name, 0):
        _, _, err, X = orc.fourview2d_score(cams, moved(x, rng, draw), 1.0)
        for i, t in enumerate(tracks):
            worst[i] = max(worst[i], rho([X[i, 0], X[i, 1], err[i]], [t["X"][0], t["X"][1], t["err"]], t["K"]))
    return worst


def round_up(v, fmt="%.3e"):
    """v to four digits, never downwards: the form the file holds the oracle's error in"""
    r = float(fmt % v)
    return r if r >= v else float(fmt % (v * 1.0005))


def quantile(values, q):
    v = sorted(values)
    return v[min(len(v) - 1, int(q * len(v)))]


# ---- the golden file ------------------------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init_solvers_golden.json")
FOURVIEW_SETS = ("fourview_a", "fourview_b", "fourview_c", "fourview_d", "fourview_e")
POSE2D_SETS = tuple("pose2d_%s_m%d" % (kind, m) for kind in ("exact", "noise") for m in (3, 6, 21))
PLANAR_SETS = tuple("planar_%s_m%d" % (kind, m) for kind in ("exact", "noise") for m in (3, 10))
TRACK_SET = "track"


def pack(a, dtype=np.float64):
    """an array as base64 of its little-endian bytes: the file holds every double bit for bit"""
    return base64.b64encode(np.ascontiguousarray(a, dtype=np.dtype(dtype).newbyteorder("<")).tobytes()).decode("ascii")


def unpack(s, shape, dtype=np.float64):
    return np.frombuffer(base64.b64decode(s), dtype=np.dtype(dtype).newbyteorder("<")).astype(dtype).reshape(shape)


def decode_set(s, data):
    """one set of the file (its JSON object) with the arrays `data` of the inputs -> the set as load_golden describes it"""
    name, N = s["name"], s["n"]
    e = dict(name=name, n=N, oracle_floor=s["oracle_floor"], share_K=s["share_K"], share_sqrtK=s["share_sqrtK"],
             oracle_rho=np.array(s["oracle_rho"], dtype=np.float64), decided=np.array([ch == "1" for ch in s["decided"]]))
    if name in FOURVIEW_SETS:
        e["x"], e["frames"] = data[s["x"]], data[s["frames"]]
        e["samples"] = unpack(s["samples"], (N, s["m"]), np.uint8).astype(np.int32)
        e["count"] = np.array([16 if ch == "1" else 0 for ch in s["full"]], dtype=np.int32)
        e["beta_positive"] = np.array([ch == "1" for ch in s["beta_positive"]])
        e["K"] = np.array(s["K"], dtype=np.float64).reshape(N, 2)
        full = int((e["count"] == 16).sum())
        pre, cam4 = unpack(s["pre"], (full, 2, 2, 2, 3)), unpack(s["cam4"], (full, 2, 2, 4))
        e["cams"] = np.full((N, 16, 4, 2, 3), np.nan)
        e["cams"][e["count"] == 16] = [candidates(p, c) for p, c in zip(pre, cam4)]
    elif name in POSE2D_SETS:
        e["x"], e["X"] = data[s["x"]][1], data[s["X"]]    # camera 1 of the four-view bearings
        e["samples"] = unpack(s["samples"], (N, s["m"]), np.uint8).astype(np.int32)
        e["K"] = np.array(s["K"], dtype=np.float64)
        e["pose"] = unpack(s["pose"], (N, 2, 3))
    elif name in PLANAR_SETS:
        e["scene"] = dict(poses=data[s["scene"] + "_poses"], lines=data[s["scene"] + "_lines"], Rg=data[s["scene"] + "_Rg"])
        e["samples"] = unpack(s["samples"], (N, s["m"]), np.uint8).astype(np.int32)
        e["K"] = np.array(s["K"], dtype=np.float64)
        e["cond"] = np.array(s["cond"], dtype=np.float64).reshape(N, 2)
        e["offsets"] = unpack(s["offsets"], (N, 3))
    else:
        e["x"], e["cams"] = data[s["x"]], unpack(s["cams"], (4, 2, 3))
        e["K"] = np.array(s["K"], dtype=np.float64)
        e["X"], e["err"], e["err_stored"], e["scale"] = unpack(s["X"], (N, 2)), unpack(s["err"], (N,)), unpack(s["err_stored"], (N,)), np.array(s["scale"])
    return e


def load_golden(path=GOLDEN):
    """tests/golden/init_solvers_golden.json as {set name: set}.  Every set holds its inputs (`x`, `frames`; `x`, `X`; `scene`; `cams`, `x`), `samples`
    [N, m], per sample `K`, `decided`, `oracle_rho`, the reference result as doubles, and per set `oracle_floor` (the nine-tenths quantile of oracle_rho),
    `share_K` and `share_sqrtK` (the share of samples with 2^-52 K, resp. 2^-52 sqrt K, above 1e-7).  Four-view: `count` [N], `beta_positive` [N] (the branch of the quadratic's first root), `cams` [N, 16, 4, 2, 3] built
    by `candidates` (NaN where count is 0), `K` [N, 2] per root.  pose2d: `pose` [N, 2, 3].  planar: `offsets` [N, 3].  track: `X` [n, 2], `err` [n],
    `scale` [n] and `err_stored` [n] (the error at the file's rounded points)."""
    with open(path) as f:
        g = json.load(f)
    data = {k: unpack(v["data"], v["shape"]) for k, v in g["inputs"].items()}
    out = {s["name"]: decode_set(s, data) for s in g["sets"]}
    out["_meta"] = dict(default_frames=data["frames_default"], digits=g["digits"])
    return out


def bound(s, i):
    """FACTOR x max(the sample's oracle rho, the set's floor): the form of tests/test_gpu_p6l_exact.py"""
    return FACTOR * max(float(s["oracle_rho"][i]), s["oracle_floor"])


def check_fourview_decided(s, cams, cnt, first=None):
    """The exact comparison one implementation (the oracle on the CPU, the device on the GPU) is held to: on every decided sample the count is the
    reference's and the sixteen candidates equal the reference's in order, up to the one exchange, within the bound.  -> largest rho / bound"""
    worst = 0.0
    for i in range(s["n"] if first is None else first):
        if not s["decided"][i]:
            continue
        assert cnt[i] == s["count"][i], (s["name"], i, "count", int(cnt[i]), int(s["count"][i]))
        if cnt[i] == 0:
            continue
        r, _ = fourview_rho(cams[i], s["cams"][i], s["K"][i])
        assert r <= bound(s, i), (s["name"], i, "rho", r, "bound", bound(s, i), "K", s["K"][i].tolist())
        worst = max(worst, r / bound(s, i))
    return worst


def check_rows_decided(s, got, key):
    """the same for one result per sample (pose2d: key 'pose', planar: 'offsets') -> largest rho / bound"""
    worst = 0.0
    for i in range(s["n"]):
        if not s["decided"][i]:
            continue
        r = rho(got[i], s[key][i], s["K"][i])
        assert r <= bound(s, i), (s["name"], i, "rho", r, "bound", bound(s, i), "K", float(s["K"][i]))
        worst = max(worst, r / bound(s, i))
    return worst


def check_track_decided(s, X, err):
    worst = 0.0
    for i in range(s["n"]):
        if not s["decided"][i]:
            continue
        r = rho([X[i, 0], X[i, 1], err[i]], [s["X"][i, 0], s["X"][i, 1], s["err"][i]], s["K"][i])
        assert r <= bound(s, i), (s["name"], i, "rho", r, "bound", bound(s, i), "K", float(s["K"][i]))
        worst = max(worst, r / bound(s, i))
    return worst
