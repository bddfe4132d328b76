"""Host-only judge for pp_ba_covariance_blocks: the covariance block of any pair of parameter blocks from the refined Schur route of
tests/covariance_reference.py (cr.SchurCovariance: inv, inv_plain, WVi, Vinv, pos, lin).  With G = S^-1:

    Cov(c, c') = G[c, c']      Cov(c, p) = -G WVi[:, 3p : 3p + 3]      Cov(p, q) = WVi_p^T G WVi_q  (+ Vinv[p] when p == q)

A side is (kind, index), kind "pose" (6 rows), "intrinsics" (12 rows: the block's parameter slots) or "point" (3 rows), indices in the scene's order.  Rows
and columns of constant parameters are zero.  The dense route (cr.dense_covariance(sc).full) holds the same blocks but carries kappa(H_scaled), which is
larger than kappa(S_scaled): it checks the formulas here (tests/test_covariance_blocks_reference.py), it does not judge the device.

Error of a block: e = ||Sigma_ab - Sigma*_ab||_F / sqrt(||Sigma*_aa||_F ||Sigma*_bb||_F); bar: cr.bar(e_LAPACK, kappa, n), e_LAPACK the same error between
the plain float64 (inv_plain) and the refined (inv) Schur route over the requested blocks.

What judges is G = S^-1 with S FORMED in long double from lin.J (schur_inverse_ld below), not SchurCovariance.inv as it stands.  inv refines the inversion
of a float64 S, and S = U - W V^-1 W^T cancels: with one camera shared by every image the float64 S of cfg 1 (f and k variable) is 6.6e-14 off, relative to
its diagonal, and kappa(S_scaled) = 8.9e3 carries that into inv.  Measured on that scene against an inverse taken in long double throughout (and confirmed
by the dense route, which has no Schur complement and sits 2.2e-12 from it): inv is 1.2e-10 off in EVERY kind of block, pose x pose included, where the bar
is 1.06e-11; the device, the blocks of pp_ba_covariance too, is 6.9e-12 off.  So inv cannot judge at its own bar there; the bar itself is computed as
stated above, from inv_plain against inv, and keeps the values it has with inv as the judge."""
import numpy as np

import covariance_reference as cr

WIDTH = {"pose": 6, "intrinsics": 12, "point": 3}
LD = np.longdouble


def schur_inverse_ld(schur):
    """S^-1, S = U - W V^-1 W^T summed in long double over the observations of lin.J (the camera columns schur.cam, the points behind them), then two
    Newton steps X + X (I - S_scaled X) from schur.inv with long-double residuals.  Cached on the SchurCovariance."""
    if hasattr(schur, "_inverse_ld"):
        return schur._inverse_ld
    lin, n = schur.lin, schur.n
    Jc = lin.J[:, schur.cam].tocsr()
    Jx = lin.J[:, lin.ncam:].tocsr()
    Jc.sort_indices()
    S = np.zeros((n, n), dtype=LD)
    M2 = lin.J.shape[0]
    obs_point = np.empty(M2 // 2, dtype=np.int64)
    A_of, cols_of, B_of = [], [], []

    def two_rows(mat, o):
        return [(mat.indices[mat.indptr[r]:mat.indptr[r + 1]], mat.data[mat.indptr[r]:mat.indptr[r + 1]]) for r in (2 * o, 2 * o + 1)]

    for o in range(M2 // 2):
        rows = two_rows(Jc, o)
        cols = np.union1d(rows[0][0], rows[1][0])
        A = np.zeros((2, len(cols)), dtype=LD)
        for r, (ix, v) in enumerate(rows):
            A[r, np.searchsorted(cols, ix)] = v
        rows = two_rows(Jx, o)
        p = int(rows[0][0][0] // 3)      # (an observation's rows hold its point's three columns)
        B = np.zeros((2, 3), dtype=LD)
        for r, (ix, v) in enumerate(rows):
            B[r, ix - 3 * p] = v
        obs_point[o] = p
        A_of.append(A); cols_of.append(cols); B_of.append(B)
        S[np.ix_(cols, cols)] += A.T @ A
    xfree = lin.free[lin.ncam:].reshape(lin.P, 3)[:, 0]
    order = np.argsort(obs_point, kind="stable")
    first = np.searchsorted(obs_point[order], np.arange(lin.P + 1))
    I3 = np.eye(3, dtype=LD)
    for p in range(lin.P):
        if not xfree[p]:
            continue
        V = np.zeros((3, 3), dtype=LD)
        W = np.zeros((n, 3), dtype=LD)
        touched = []
        for o in order[first[p]:first[p + 1]]:
            V += B_of[o].T @ B_of[o]
            W[cols_of[o]] += A_of[o].T @ B_of[o]
            touched.append(cols_of[o])
        if not touched:
            continue
        nz = np.unique(np.concatenate(touched))
        Vi = np.linalg.inv(V.astype(np.float64)).astype(LD)
        for _ in range(3):
            Vi = Vi + Vi @ (I3 - V @ Vi)
        S[np.ix_(nz, nz)] -= W[nz] @ Vi @ W[nz].T
    S = (S + S.T) / 2
    d = np.sqrt(np.diag(S))
    H = S / d[:, None] / d[None, :]
    X = schur.inv * d.astype(np.float64)[:, None] * d.astype(np.float64)[None, :]      # the scaled inverse
    for _ in range(2):
        R = -(H @ X.astype(LD))
        R[np.arange(n), np.arange(n)] += 1.0
        X = X + X @ R.astype(np.float64)      # (the correction is small: its own rounding is far below u)
    X = (X.astype(LD) / d[:, None] / d[None, :]).astype(np.float64)
    schur._inverse_ld = 0.5 * (X + X.T)
    return schur._inverse_ld


def full_columns(lin, side):
    """the side's columns in the full layout of covariance_reference (pose c at 6 c, parameter j of intrinsics block k at 6 C + 12 k + j, points behind)"""
    kind, i = side
    first = {"pose": 6 * i, "intrinsics": 6 * lin.C + 12 * i, "point": lin.ncam + 3 * i}[kind]
    return np.arange(first, first + WIDTH[kind])


class SchurBlocks:
    """every block of H^-1 from a cr.SchurCovariance"""

    def __init__(self, schur):
        self.schur = schur
        self._sides = {}
        self._diag = {}

    def _side(self, side):
        """(rows of G the side touches, coefficients [rows, w]): Cov(a, b) = coef_a^T G[rows_a, rows_b] coef_b"""
        if side not in self._sides:
            s = self.schur
            kind, i = side
            if kind == "point":
                B = s.WVi[:, 3 * i:3 * i + 3].tocsc()
                rows = np.unique(B.indices)
                coef = -B[rows].toarray()
            else:
                pos = s.pos[full_columns(s.lin, side)]
                rows = pos[pos >= 0]
                coef = np.zeros((len(rows), WIDTH[kind]))
                coef[np.arange(len(rows)), np.flatnonzero(pos >= 0)] = 1.0
            self._sides[side] = (rows, coef)
        return self._sides[side]

    def block(self, a, b, route="judge"):
        """route: "judge" = schur_inverse_ld, "inv" / "plain" = SchurCovariance's refined / plain float64 inverse (the two e_LAPACK compares)"""
        G = {"judge": schur_inverse_ld, "inv": lambda s: s.inv, "plain": lambda s: s.inv_plain}[route](self.schur)
        (ra, ca), (rb, cb) = self._side(a), self._side(b)
        out = ca.T @ G[np.ix_(ra, rb)] @ cb
        if a == b and a[0] == "point":
            out = out + self.schur.Vinv[a[1]]
        return out

    def diag(self, a):
        if a not in self._diag:
            self._diag[a] = self.block(a, a)
        return self._diag[a]

    def error(self, got, a, b):
        return cr.block_error(got, self.block(a, b), self.diag(a), self.diag(b))

    def e_lapack(self, a, b):
        """the block's error between the plain float64 and the refined Schur route"""
        return cr.block_error(self.block(a, b, "plain"), self.block(a, b, "inv"), self.block(a, a, "inv"), self.block(b, b, "inv"))


def dense_block(dense, a, b):
    """the same block as a slice of cr.dense_covariance(sc).full"""
    return dense.full[np.ix_(full_columns(dense.lin, a), full_columns(dense.lin, b))]


def judge(tag, schur, blocks, got):
    """asserts every returned block inside the bar -> (bar, worst error); blocks: the request [(side_a, side_b)], got: the arrays returned for it"""
    assert schur.kappa < 1e10, "%s: kappa(S_scaled) = %.2e: not a scene this suite may judge by" % (tag, schur.kappa)
    ref = SchurBlocks(schur)
    assert len(got) == len(blocks)
    e_lapack = max([ref.e_lapack(a, b) for a, b in blocks] + [0.0])
    limit = cr.bar(e_lapack, schur.kappa, schur.n)
    worst, where = 0.0, None
    for (a, b), g in zip(blocks, got):
        assert g.shape == (WIDTH[a[0]], WIDTH[b[0]]) and np.isfinite(g).all(), (a, b)
        e = ref.error(g, a, b)
        if e > worst:
            worst, where = e, (a, b)
    print("ACCURACY %-32s kappa %.2e n %4d e_lapack %.2e bar %.2e blocks %5d worst %.2e" % (tag, schur.kappa, schur.n, e_lapack, limit, len(blocks), worst))
    assert limit < 1e-5
    assert worst <= limit, "%s: block %s %.3e > %.3e" % (tag, where, worst, limit)
    return limit, worst
