"""The Cholesky solver (csrc/cholesky.hip, csrc/chol_block.hpp) against LAPACK on ILL-CONDITIONED systems, and its failure report on every launch path.

The other Cholesky tests use strongly diagonally dominant matrices (condition below ~10, solution nearly b / diag A) and compare the project's paths
with each other.  Here every matrix has a Jacobi-scaled condition number kappa(H) of 1e4 .. 7e10, and the judge is LAPACK on the same matrix plus a
solution refined with long-double residuals (tests/cholesky_reference.py, itself checked by tests/test_cholesky_reference.py):

    eta(x) <= E = max(4 eta(x_lapack), sqrt(n) u)                    scaled backward error (the sharp bar), u = 2^-53
    fwd(x) <= max(4 fwd(x_lapack), kappa(H) E, 10 delta)             scaled forward error (what hides in the residual's null directions)

4: another, equally valid summation order (64-wide blocks, four-way split MFMA accumulators, the right-hand side as an extra row); sqrt(n) u: LAPACK often
lands far below u, and rounding errors of an n-term inner product grow like sqrt(n); 10 delta: below that the reference cannot judge.

Observed on an MI355X: the table at the end of this docstring (`pytest -s` prints one ACCURACY line per case).  The device sits beside LAPACK everywhere:
its largest eta is 5.2e-16 (forest_4) against a bar of 6.1e-15, and every forward error is within 7 x LAPACK's, orders of magnitude inside kappa(H) E.

The failure tests break a well-conditioned matrix at one pivot - in every panel of a tile (PotrfPanel16 for columns 0-47, PotrfLastPanelWithInverse for
48-63), in the first, a middle and the last block column and at the last unknown beside the right-hand side's row, on the small, one-launch and
per-column paths, inside a leaf and a separator of several-chain factorisations - and expect PP_ERR_NUMERIC, then a clean solve in the same process.
Only numpy's default quiet NaN is fed in: the back substitution keeps the all-ones pattern as its "not ready" marker.

Observed (device = dev, LAPACK = lap):
    case                                 n  kappa(H)   dev eta  dev fwd   lap eta  lap fwd   bar eta  bar fwd
    geometric 1e+04                      1   1.0e+00   0.0e+00  0.0e+00   0.0e+00  0.0e+00   1.1e-16  1.1e-16
    geometric 1e+08                      1   1.0e+00   0.0e+00  0.0e+00   0.0e+00  0.0e+00   1.1e-16  1.1e-16
    geometric 1e+10                      1   1.0e+00   0.0e+00  0.0e+00   0.0e+00  0.0e+00   1.1e-16  1.1e-16
    geometric 1e+04                      2   9.5e+03   5.2e-17  3.2e-13   3.5e-17  3.3e-13   1.6e-16  1.5e-12
    geometric 1e+08                      2   9.6e+07   5.1e-17  1.0e-09   7.2e-17  6.4e-09   2.9e-16  2.8e-08
    geometric 1e+10                      2   3.7e+09   6.9e-17  1.3e-07   5.0e-17  1.3e-07   2.0e-16  7.4e-07
    geometric 1e+04                     15   4.7e+03   1.5e-16  8.6e-15   2.9e-17  8.8e-14   4.3e-16  2.0e-12
    geometric 1e+08                     15   1.6e+07   2.0e-16  9.8e-11   2.4e-17  1.1e-10   4.3e-16  7.1e-09
    geometric 1e+10                     15   2.9e+09   4.7e-17  6.8e-09   2.9e-17  2.3e-08   4.3e-16  1.2e-06
    geometric 1e+04                     16   6.3e+03   7.0e-17  4.4e-14   2.7e-17  3.4e-14   4.4e-16  2.8e-12
    geometric 1e+08                     16   1.0e+08   6.3e-17  3.2e-10   1.8e-17  4.8e-10   4.4e-16  4.5e-08
    geometric 1e+10                     16   4.0e+09   2.8e-17  6.8e-09   7.7e-17  3.0e-08   4.4e-16  1.8e-06
    geometric 1e+04                     17   1.0e+04   3.8e-17  7.5e-14   4.2e-17  3.8e-14   4.6e-16  4.7e-12
    geometric 1e+08                     17   9.7e+06   1.2e-16  2.6e-11   3.7e-17  1.6e-10   4.6e-16  4.4e-09
    geometric 1e+10                     17   2.4e+09   3.1e-17  1.3e-09   2.6e-17  2.6e-08   4.6e-16  1.1e-06
    geometric 1e+04                     63   1.3e+04   2.2e-17  5.1e-14   2.3e-17  4.2e-14   8.8e-16  1.2e-11
    geometric 1e+08                     63   5.1e+07   3.4e-17  1.1e-10   2.8e-17  1.4e-10   8.8e-16  4.5e-08
    geometric 1e+10                     63   2.6e+09   2.6e-17  4.4e-09   2.1e-17  3.7e-09   8.8e-16  2.3e-06
    geometric 1e+04                     64   1.1e+04   4.0e-17  5.6e-14   3.6e-17  7.6e-14   8.9e-16  1.0e-11
    geometric 1e+08                     64   4.6e+07   8.0e-17  9.7e-11   2.3e-17  1.5e-10   8.9e-16  4.1e-08
    geometric 1e+10                     64   3.7e+09   1.6e-16  2.0e-08   3.8e-17  1.4e-08   8.9e-16  3.3e-06
    geometric 1e+04                     65   1.7e+04   3.4e-17  2.4e-14   1.9e-17  4.4e-14   9.0e-16  1.6e-11
    geometric 1e+08                     65   8.9e+07   1.9e-16  9.1e-10   3.1e-17  2.7e-10   9.0e-16  8.0e-08
    geometric 1e+10                     65   6.0e+09   1.1e-16  3.5e-08   2.7e-17  5.6e-09   9.0e-16  5.4e-06
    geometric 1e+04                    190   1.6e+04   2.1e-17  2.1e-14   3.8e-17  3.1e-14   1.5e-15  2.4e-11
    geometric 1e+08                    190   1.2e+08   1.4e-17  4.6e-11   4.2e-17  2.6e-10   1.5e-15  1.9e-07
    geometric 1e+10                    190   5.8e+09   1.2e-17  2.1e-09   4.4e-17  4.5e-09   1.5e-15  8.8e-06
    geometric 1e+04                    191   1.7e+04   2.1e-17  6.6e-14   3.8e-17  3.4e-14   1.5e-15  2.6e-11
    geometric 1e+08                    191   1.1e+08   1.2e-17  2.1e-10   2.9e-17  1.7e-10   1.5e-15  1.7e-07
    geometric 1e+10                    191   1.0e+10   1.2e-17  9.2e-09   3.1e-17  2.1e-08   1.5e-15  1.6e-05
    geometric 1e+04                    192   1.7e+04   1.2e-17  3.1e-14   5.6e-17  3.3e-14   1.5e-15  2.7e-11
    geometric 1e+08                    192   6.0e+07   9.4e-18  7.3e-11   3.0e-17  1.0e-10   1.5e-15  9.2e-08
    geometric 1e+10                    192   7.0e+09   1.5e-17  2.0e-09   4.8e-17  2.7e-08   1.5e-15  1.1e-05
    geometric 1e+04                    255   2.3e+04   1.5e-17  2.9e-14   2.4e-17  1.9e-14   1.8e-15  4.0e-11
    geometric 1e+08                    255   9.0e+07   8.8e-18  4.4e-11   3.5e-17  1.6e-10   1.8e-15  1.6e-07
    geometric 1e+10                    255   1.0e+10   7.6e-18  1.9e-09   2.8e-17  5.6e-09   1.8e-15  1.8e-05
    geometric 1e+04                    700   4.5e+04   6.6e-18  1.0e-14   2.5e-17  2.0e-14   2.9e-15  1.3e-10
    geometric 1e+04 columns            700   4.5e+04   6.6e-18  1.0e-14   2.5e-17  2.0e-14   2.9e-15  1.3e-10
    geometric 1e+08                    700   3.8e+08   4.7e-18  4.6e-11   2.1e-17  1.1e-10   2.9e-15  1.1e-06
    geometric 1e+08 columns            700   3.8e+08   4.7e-18  4.6e-11   2.1e-17  1.1e-10   2.9e-15  1.1e-06
    geometric 1e+10                    700   1.8e+10   7.2e-18  6.8e-09   2.4e-17  5.7e-09   2.9e-15  5.3e-05
    geometric 1e+10 columns            700   1.8e+10   7.2e-18  6.8e-09   2.4e-17  5.7e-09   2.9e-15  5.3e-05
    geometric 1e+04                   3001   9.4e+04   3.0e-18  1.5e-14   4.8e-18  5.7e-15   6.1e-15  5.7e-10
    geometric 1e+04 columns           3001   9.4e+04   3.0e-18  1.5e-14   4.8e-18  5.7e-15   6.1e-15  5.7e-10
    geometric 1e+04 pairs=0           3001   9.4e+04   3.0e-18  1.5e-14   4.8e-18  5.7e-15   6.1e-15  5.7e-10
    geometric 1e+08                   3001   6.8e+08   1.5e-18  2.6e-11   6.1e-18  3.3e-11   6.1e-15  4.2e-06
    geometric 1e+08 columns           3001   6.8e+08   1.5e-18  2.6e-11   6.1e-18  3.3e-11   6.1e-15  4.2e-06
    geometric 1e+08 pairs=0           3001   6.8e+08   1.7e-18  2.6e-11   6.1e-18  3.3e-11   6.1e-15  4.2e-06
    geometric 1e+10                   3001   6.7e+10   1.4e-18  1.1e-09   5.7e-18  2.6e-09   6.1e-15  4.1e-04
    geometric 1e+10 columns           3001   6.7e+10   1.4e-18  1.1e-09   5.7e-18  2.6e-09   6.1e-15  4.1e-04
    geometric 1e+10 pairs=0           3001   6.7e+10   1.6e-18  1.1e-09   5.7e-18  2.6e-09   6.1e-15  4.1e-04
    geometric 1e+04                   3071   8.8e+04   2.7e-18  8.8e-15   4.2e-18  8.2e-15   6.2e-15  5.4e-10
    geometric 1e+08                   3071   7.4e+08   1.7e-18  4.9e-11   3.6e-18  3.9e-11   6.2e-15  4.6e-06
    geometric 1e+10                   3071   6.9e+10   1.4e-18  6.0e-10   5.4e-18  2.5e-09   6.2e-15  4.2e-04
    geometric 1e+04                   4500   1.1e+05   2.5e-18  4.1e-15   4.4e-18  8.3e-15   7.4e-15  8.1e-10
    geometric 1e+04 columns           4500   1.1e+05   2.4e-18  4.5e-15   4.4e-18  8.3e-15   7.4e-15  8.1e-10
    geometric 1e+08                   4500   1.0e+09   9.1e-19  3.9e-11   2.6e-18  2.3e-11   7.4e-15  7.6e-06
    geometric 1e+08 columns           4500   1.0e+09   9.9e-19  3.9e-11   2.6e-18  2.3e-11   7.4e-15  7.6e-06
    geometric 1e+10                   4500   7.4e+10   1.2e-18  5.9e-10   2.7e-18  1.5e-09   7.4e-15  5.5e-04
    geometric 1e+10 columns           4500   7.4e+10   1.3e-18  4.6e-10   2.7e-18  1.5e-09   7.4e-15  5.5e-04
    geometric 1e+08                   8191   1.5e+09   1.0e-18  3.5e-11   2.6e-18  1.1e-11   1.0e-14  1.5e-05
    geometric 1e+08                   8200   1.9e+09   7.2e-19  2.7e-11   1.7e-18  1.6e-11   1.0e-14  1.9e-05
    one_small 1e+08                    700   4.4e+06   2.0e-16  3.7e-10   1.0e-16  1.6e-10   2.9e-15  1.3e-08
    one_small 1e+06                   3001   1.3e+03   1.9e-16  7.1e-14   9.8e-17  3.4e-14   6.1e-15  8.0e-12
    two_leaves                        2988   2.3e+08   1.2e-16  3.4e-09   9.0e-17  3.3e-09   6.1e-15  1.4e-06
    two_leaves one chain              2988   2.3e+08   1.3e-16  3.6e-09   9.0e-17  3.3e-09   6.1e-15  1.4e-06
    uneven                            2986   9.6e+07   6.4e-17  1.1e-09   9.2e-17  1.9e-09   6.1e-15  5.8e-07
    uneven one chain                  2986   9.6e+07   6.5e-17  1.1e-09   9.2e-17  1.9e-09   6.1e-15  5.8e-07
    four_leaves                       2980   7.4e+07   1.5e-16  1.0e-09   9.9e-17  1.3e-09   6.1e-15  4.5e-07
    four_leaves one chain             2980   7.4e+07   1.5e-16  1.1e-09   9.9e-17  1.3e-09   6.1e-15  4.5e-07
    two_level                         2988   7.5e+06   7.6e-17  9.0e-11   1.0e-16  1.7e-10   6.1e-15  4.5e-08
    two_level one chain               2988   7.5e+06   7.5e-17  9.4e-11   1.0e-16  1.7e-10   6.1e-15  4.5e-08
    twelve_leaves                     3252   1.8e+07   1.9e-16  3.9e-10   6.6e-17  1.6e-10   6.3e-15  1.2e-07
    twelve_leaves one chain           3252   1.8e+07   2.1e-16  3.9e-10   6.6e-17  1.6e-10   6.3e-15  1.2e-07
    band_1000_150                     1000   6.6e+06   1.6e-16  4.3e-10   6.5e-17  1.7e-10   3.5e-15  2.3e-08
    band_1000_150 one chain           1000   6.6e+06   1.6e-16  4.3e-10   6.5e-17  1.7e-10   3.5e-15  2.3e-08
    band_2990_900                     2990   5.3e+07   5.0e-17  1.4e-09   8.3e-17  2.1e-09   6.1e-15  3.2e-07
    band_2990_900 one chain           2990   5.3e+07   5.0e-17  1.4e-09   8.3e-17  2.1e-09   6.1e-15  3.2e-07
    forest_0                          1634   8.9e+06   2.2e-16  3.8e-10   7.1e-17  1.4e-10   4.5e-15  4.0e-08
    forest_0 one chain                1634   8.9e+06   2.1e-16  3.5e-10   7.1e-17  1.4e-10   4.5e-15  4.0e-08
    forest_2                          3367   1.5e+07   2.3e-16  4.7e-10   6.9e-17  1.7e-10   6.4e-15  9.7e-08
    forest_2 one chain                3367   1.5e+07   2.4e-16  4.7e-10   6.9e-17  1.7e-10   6.4e-15  9.7e-08
    forest_4                          2999   1.3e+08   5.2e-16  9.9e-09   7.9e-17  2.1e-09   6.1e-15  7.6e-07
    forest_4 one chain                2999   1.3e+08   4.9e-16  9.9e-09   7.9e-17  2.1e-09   6.1e-15  7.6e-07
    dense60 radius 1e+04               353   3.5e+03   1.6e-16  9.5e-15   9.2e-17  1.4e-14   2.1e-15  7.2e-12
    dense60 radius 1e+08               353   1.5e+04   1.4e-16  9.0e-14   9.8e-17  1.6e-13   2.1e-15  3.1e-11
    dense60 radius 1e+12               353   1.5e+04   1.3e-16  9.1e-14   1.1e-16  1.5e-13   2.1e-15  3.1e-11
    sequence150 radius 1e+04           893   7.5e+03   1.2e-16  7.6e-14   7.3e-17  4.8e-14   3.3e-15  2.5e-11
    sequence150 radius 1e+08           893   5.5e+06   1.1e-16  2.0e-11   7.3e-17  1.1e-11   3.3e-15  1.8e-08
    sequence150 radius 1e+12           893   6.0e+06   1.1e-16  8.6e-12   7.3e-17  6.1e-12   3.3e-15  2.0e-08
    dense500 radius 1e+04             2993   5.2e+03   2.2e-16  4.8e-14   1.1e-16  7.8e-15   6.1e-15  3.2e-11
    dense500 radius 1e+08             2993   7.4e+06   2.3e-16  1.7e-11   1.2e-16  1.2e-11   6.1e-15  4.5e-08
    dense500 radius 1e+12             2993   8.6e+06   2.3e-16  7.1e-11   1.3e-16  2.4e-11   6.1e-15  5.2e-08
"""
import numpy as np
import pytest

import cholesky_reference as cr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not cr.longdouble_is_extended(), reason="numpy.longdouble has no more digits than double on this host")]

COLUMNS = {"PPSFM_CHOL_MODE": "columns"}
_last = [None, None]      # one-slot cache: the variants of a case are parametrised next to each other and share the host's work


def _reference(key, build):
    if _last[0] != key:
        _last[0], _last[1] = None, None      # (drop the old matrix before the new one is built)
        _last[1] = cr.Reference(*build())
        _last[0] = key
    return _last[1]


def _solve(A, b, env, monkeypatch, **kw):
    from privacy_preserving_sfm_amd.device import dense_cholesky_solve
    for k, v in env.items():
        monkeypatch.setenv(k, v)      # (read when the entry point starts)
    try:
        return dense_cholesky_solve(A, b, **kw)[0]
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _judge(R, x, what):
    E, F = R.bounds()
    e, f = R.eta(x), R.fwd(x)
    print("\nACCURACY %-44s n=%-5d kappa(H) %.1e | device eta %.1e fwd %.1e | lapack eta %.1e fwd %.1e | delta %.1e | bars %.1e %.1e" %
          (what, R.n, R.kappa, e, f, R.eta_lapack, R.fwd_lapack, R.delta, E, F))
    assert R.reference_conditions(), (what, R.row())      # the judge first
    assert np.all(np.isfinite(x)), what
    assert e <= E, (what, "eta", e, E)
    assert f <= F, (what, "fwd", f, F)


def _spectrum_params():
    out = []
    for n, kappa, spectrum in cr.SPECTRUM_CASES:
        envs = [{}]
        if n in (700, 3001, 4500) and spectrum == "geometric":
            envs.append(COLUMNS)
        if n == 3001 and spectrum == "geometric":
            envs.append({"PPSFM_BACKSUB_PAIRS": "0"})
        out += [pytest.param(n, kappa, spectrum, env, id="%d-%.0e-%s-%s" % (n, kappa, spectrum, "+".join("%s=%s" % kv for kv in env.items()) or "default"))
                for env in envs]
    return out


@pytest.mark.parametrize("n,kappa,spectrum,env", _spectrum_params())
def test_prescribed_spectrum(n, kappa, spectrum, env, monkeypatch):
    """builder (a): n = 1 .. 192 the single-workgroup path (fewer than four block columns with the right-hand side's row), 255 .. 8191 the one-launch task
    path (3001 / 3071: 47 / 48 block columns; also launched per column, and with the block-by-block back substitution), 8200 per column by size"""
    R = _reference(("a", n, kappa, spectrum), lambda: cr.spectrum_case(n, kappa, spectrum))
    _judge(R, _solve(R.A, R.b, env, monkeypatch), "spectrum %s %.0e %s" % (spectrum, kappa, env or ""))


@pytest.mark.parametrize("env", [{}, {"PPSFM_CHOL_CHAINS": "1"}], ids=["default", "one_chain"])
@pytest.mark.parametrize("name", list(cr.STRUCTURE_CASES))
def test_block_structures(name, env, monkeypatch):
    """builder (b): dissected / banded / random-forest tile maps without a dominant diagonal, with the chains the plan finds and with one chain"""
    R = _reference(("b", name), cr.STRUCTURE_CASES[name])
    _judge(R, _solve(R.A, R.b, env, monkeypatch), "structure %s %s" % (name, env or ""))


@pytest.mark.parametrize("scene", list(cr.SCENES))
def test_reduced_camera_systems(scene):
    """builder (c): the handle's own reduced camera systems at trust-region radii 1e4, 1e8 and 1e12, the unknowns' columns in the handle's image order"""
    from privacy_preserving_sfm_amd.device import BAProblem, dense_cholesky_solve, plan_ordering
    sc = cr.make_scene(scene)
    order, info = plan_ordering(sc)
    pb = BAProblem(sc)
    systems = [pb.reduced_system(radius) for radius in cr.RADII]
    pb.close()
    for radius, (S, rhs) in zip(cr.RADII, systems):
        A, b = cr.camera_system(sc, S, rhs, order if info["reordered"] else None)
        _judge(cr.Reference(A, b), dense_cholesky_solve(A, b)[0], "scene %s radius %.0e" % (scene, radius))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# metamorphic: exact scalings

@pytest.mark.parametrize("n", [190, 700, 3001])
def test_power_of_two_scalings_commute_bitwise(n):
    """solve(A, s b) = s solve(A, b) for s = 2^k and solve(4^k A, b) = 4^-k solve(A, b), bit for bit: a scaling by a power of four commutes exactly with
    the reciprocal square root and its correction step, with every product and fma - as long as nothing overflows or goes subnormal -, so any difference is a
    hidden absolute constant.  The one there is - the pseudo-pivot 1e100 of the right-hand side's row - does not reach x while ||L^-1 b||^2 < 1e100; these
    exponents stay far inside that (include/ppsfm_hip.h)."""
    from privacy_preserving_sfm_amd.device import dense_cholesky_solve
    A, b = cr.spectrum_case(n, 1e8, "geometric")
    x = dense_cholesky_solve(A, b)[0]
    assert np.all(np.isfinite(x)) and np.any(x != 0)
    for k in (-60, -7, 9, 60):
        assert np.array_equal(dense_cholesky_solve(A, 2.0 ** k * b)[0], 2.0 ** k * x), ("b", k)
        assert np.array_equal(dense_cholesky_solve(4.0 ** k * A, b)[0], 4.0 ** -k * x), ("A", k)


@pytest.mark.parametrize("n", [190, 700])
def test_upper_triangle_is_not_read(n):
    from privacy_preserving_sfm_amd.device import dense_cholesky_solve
    A, b = cr.spectrum_case(n, 1e8, "geometric")
    G = A.copy()
    G[np.triu_indices(n, 1)] = 1e300
    assert np.array_equal(dense_cholesky_solve(G, b)[0], dense_cholesky_solve(A, b)[0])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# failure reporting

def _dominant(n, seed, cols=64):
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(n, cols))
    return B @ B.T + np.diag(rng.uniform(0.5, 2.0, n)) * n


def _band(n, band, seed):
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n))
    for i in range(0, n, 50):
        j = min(n, i + band)
        B = rng.normal(size=(j - i, 20))
        A[i:j, i:j] += B @ B.T
    return A + np.diag(rng.uniform(1.0, 2.0, n)) * 20


def _forest(seed):
    nz, n = cr._forest(seed)
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n))
    for i, j in zip(*np.nonzero(nz)):
        r0, r1, c0, c1 = 64 * i, min(n, 64 * i + 64), 64 * j, min(n, 64 * j + 64)
        A[r0:r1, c0:c1] = rng.normal(size=(r1 - r0, c1 - c0)) * 0.1
    A = np.tril(A) + np.tril(A, -1).T
    return A + np.diag(np.abs(A).sum(axis=1) + 1.0)


def _dissected(shape):
    from test_gpu_bundle_adjustment import _dissected_spd
    rng = np.random.default_rng(len(shape))
    return {"two_leaves": lambda: _dissected_spd(rng, [1344, 1344], 300, 200), "twelve_leaves": lambda: _dissected_spd(rng, [256] * 12, 180, 100)}[shape]()


# path -> (matrix, switches, {place: pivot index}).  The index of a place fixes block column and column inside the 64-wide tile.
PATHS = {
    "small100": (lambda: _dominant(100, 1), {}, {"middle": 37, "last": 99}),
    "tasks700": (lambda: _dominant(700, 2), {}, dict([("first", 20), ("last_column", 640 + 20), ("last", 699)] + [("tile5_col%d" % c, 320 + c) for c in (0, 15, 16, 47, 48, 63)])),
    "tasks3001": (lambda: _dominant(3001, 3), {}, {"middle": 64 * 23 + 48, "last": 3000}),
    "columns700": (lambda: _dominant(700, 2), COLUMNS, {"middle": 320 + 16, "last": 699}),
    "columns3001": (lambda: _dominant(3001, 3), COLUMNS, {"middle": 64 * 23 + 48, "last": 3000}),
    "columns8200": (lambda: _dominant(8200, 4), {}, {"middle": 64 * 70 + 63, "last": 8199}),
    "two_leaves": (lambda: _dissected("two_leaves"), {}, {"leaf": 1344 + 640 + 17, "separator": 2688 + 100}),       # (second leaf: not chain 0)
    "twelve_leaves": (lambda: _dissected("twelve_leaves"), {}, {"leaf": 256 * 7 + 128 + 33, "separator": 3072 + 50}),
    "band": (lambda: _band(2990, 300, 5), {}, {"middle": 64 * 20 + 47, "last": 2989}),
    "forest": (lambda: _forest(2), {}, {"middle": 64 * 11 + 15, "last": None}),      # (None: n - 1)
}
KINDS = ("minus_one", "exact_zero", "nan_diagonal", "inf_off_diagonal", "nan_rhs")


def _failure_params():
    out = [("tasks700", place, kind) for place in PATHS["tasks700"][2] if place.startswith("tile5") for kind in KINDS]
    for path, (_, _, places) in PATHS.items():
        out += [(path, place, kind) for place in places if not place.startswith("tile5") for kind in KINDS[:2]]
    return out


def _integer_factor(A0, seed):
    """unit lower-triangular L of small integers on the non-zero tiles of A0: at most one +-1 per row inside its diagonal tile (so the tile's inverse, which
    the solver multiplies with, has entries 0, +-1 only) and about one in three of its off-diagonal tiles.  Every intermediate of the factorisation of
    L L^T is then a small integer: the elimination is exact in any summation order, and a pivot that is zero in exact arithmetic is 0.0."""
    rng = np.random.default_rng(seed)
    n = A0.shape[0]
    nz = cr.tile_map(A0)
    rows = np.arange(n)
    tr = rows // 64
    L = np.eye(n)
    inner = rows[rows % 64 > 0]
    L[inner, 64 * tr[inner] + rng.integers(0, inner % 64)] = rng.choice([-1.0, 1.0], len(inner))
    for j in range(nz.shape[0]):
        sel = rows[(tr > j) & nz[tr, j] & (rng.random(n) < 0.3)]
        L[sel, 64 * j + rng.integers(0, 64, len(sel))] = rng.choice([-1.0, 1.0], len(sel))
    return L


_failure_cache = [None, None]


def _failure_system(path):
    if _failure_cache[0] != path:
        _failure_cache[0], _failure_cache[1] = None, None
        A0 = PATHS[path][0]()
        L = _integer_factor(A0, len(path))
        _failure_cache[1] = (A0, L, L @ L.T)
        _failure_cache[0] = path
    return _failure_cache[1]


def _healthy(A, x, b):
    r = A @ x - b
    return np.all(np.isfinite(x)) and np.abs(r).max() <= 1e-10 * (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())


@pytest.mark.parametrize("path,place,kind", _failure_params())
def test_broken_pivot_is_reported_and_leaves_nothing_behind(path, place, kind, monkeypatch):
    from privacy_preserving_sfm_amd._capi import PPError, PP_ERR_NUMERIC
    A0, L, I0 = _failure_system(path)
    env, p = PATHS[path][1], PATHS[path][2][place]
    n = A0.shape[0]
    p = n - 1 if p is None else p
    b = np.random.default_rng(p).normal(size=n)
    good = I0 if kind == "exact_zero" else A0
    A = good.copy()
    if kind == "minus_one":
        A[p, p] = -1.0
    elif kind == "exact_zero":      # row / column p repeats row / column p - 1: the pivot p is A[p,p] - sum L[p,k]^2 = 0 exactly
        L2 = L.copy()
        L2[p] = L2[p - 1]
        A[p, :] = A[:, p] = L2 @ L2[p]
        assert np.array_equal(A[p], A[p - 1]) and np.array_equal(cr.tile_map(A), cr.tile_map(I0))
    elif kind == "nan_diagonal":
        A[p, p] = np.nan
    elif kind == "inf_off_diagonal":
        A[p, p - 1] = A[p - 1, p] = np.inf
    else:
        b = b.copy()
        b[p] = np.nan
    with pytest.raises(PPError) as e:
        _solve(A, b, env, monkeypatch)
    assert e.value.code == PP_ERR_NUMERIC and "not positive definite" in str(e.value), str(e.value)
    b = np.random.default_rng(p).normal(size=n)
    assert _healthy(good, _solve(good, b, env, monkeypatch), b)      # state, graph and flag of the failed call did not leak


@pytest.mark.parametrize("scene", ["dense60", "sequence150"])
def test_lm_reports_a_nan_system_as_a_failure_not_as_a_timeout(scene):
    """a point with a NaN coordinate: every reduced system holds NaN.  On the one-launch path with six block columns and on the several-chain path the LM loop
    must see bit 0 of the factorisation's flag (invalid step) and not bit 2 (timeout: a fallback to per-column launches and a repeat of the step)."""
    from privacy_preserving_sfm_amd import _capi
    from privacy_preserving_sfm_amd.device import BAProblem, ba_options
    sc = cr.make_scene(scene)
    healthy = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    sc["points"][7] = np.array([np.nan, 0.0, 1.0])
    pb = BAProblem(sc)
    st = pb.structure()
    assert (st["chains"] >= 2) == (scene == "sequence150") and not st["iterative"]
    before = [a.copy() for a in pb.get_parameters()]
    with pytest.raises(_capi.PPError) as e:
        pb.solve(ba_options())
    s = e.value.summary
    after = pb.get_parameters()
    pb.close()
    assert e.value.code == _capi.PP_ERR_NUMERIC and s.termination == _capi.TERM_FAILURE
    assert s.cholesky_fallbacks == 0 and s.num_successful_steps == 0
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
    pb = BAProblem(healthy)
    s = pb.solve(ba_options(max_num_iterations=3))
    pb.close()
    assert s.cholesky_fallbacks == 0 and s.num_successful_steps >= 1 and s.final_cost < s.initial_cost
