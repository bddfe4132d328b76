"""The host reference of tests/test_gpu_cholesky_accuracy.py judged on its own, without a GPU: on every matrix the accuracy tests use, LAPACK's double
Cholesky solve is backward stable in the Jacobi-scaled sense (eta <= 4u), its forward error is inside the first-order bound kappa(H) u, and the
refined solution's own uncertainty is at most a tenth of LAPACK's forward error - so x_ref may judge a solver that is as good as LAPACK.
The reduced camera systems come from the oracle here (the device's agree with it to 1e-9, test_reduced_system_matches_oracle); the GPU tests repeat the
same conditions on the device's own systems before they use them."""
import numpy as np
import pytest

import cholesky_reference as cr

pytestmark = pytest.mark.skipif(not cr.longdouble_is_extended(), reason="numpy.longdouble has no more digits than double on this host")


def _check(R, what):
    print("\n%s n=%d: %s" % (what, R.n, R.row()))
    assert R.kappa <= 1e11, what
    assert R.eta_lapack <= 4 * cr.U, what
    assert R.fwd_lapack <= R.kappa * cr.U, what
    assert R.delta <= R.fwd_lapack / 10, what
    assert R.reference_conditions()


def test_longdouble_residual_sees_what_double_cannot():
    """b - A x for an x that is the double rounding of an exact solution: the long-double residual is the rounding of x, about u |A| |x|; a scaling of the
    rows by powers of two leaves eta untouched to the last bit"""
    rng = np.random.default_rng(1)
    A, b = cr.spectrum_spd(200, 1e6, 1)
    R = cr.Reference(A, b)
    s = 2.0 ** rng.integers(-20, 21, 200)
    R2 = cr.Reference(A * s[:, None] * s[None, :], b * s)
    assert R2.eta(R.x_lapack / s) == R.eta_lapack and 0 < R.eta_lapack < cr.U
    assert R.eta(R.x_ref) < R.eta_lapack or R.eta_lapack < 2.0 ** -60
    assert R.fwd(R.x_lapack * (1 + 1e-9)) > 0.9e-9


@pytest.mark.parametrize("n,kappa,spectrum", cr.SPECTRUM_CASES)
def test_reference_on_prescribed_spectra(n, kappa, spectrum):
    A, b = cr.spectrum_case(n, kappa, spectrum)
    assert np.array_equal(A, A.T)
    R = cr.Reference(A, b)
    _check(R, (n, kappa, spectrum))
    if n >= 64 and spectrum == "geometric":
        assert 0.1 * kappa <= R.kappa <= 30 * kappa      # (the Jacobi scaling moves the prescribed condition number by a modest factor only: 19 at n = 8200)


@pytest.mark.parametrize("name", list(cr.STRUCTURE_CASES))
def test_reference_on_block_structures(name):
    A, b = cr.STRUCTURE_CASES[name]()
    assert np.array_equal(A, A.T)
    R = cr.Reference(A, b)
    _check(R, name)
    assert 1e6 <= R.kappa <= 1e9, name
    tm = cr.tile_map(A)
    T = tm.shape[0]
    assert np.tril(tm).sum() < 0.6 * T * (T + 1) / 2, name      # the zero tiles stayed zero
    if name.startswith("forest"):
        nz, n = cr._forest(int(name[-1]))
        assert np.array_equal(np.tril(tm), nz.astype(bool)), name


def test_scaled_spectrum_by_lanczos_agrees_with_all_eigenvalues():
    A, _ = cr.STRUCTURE_CASES["forest_0"]()      # n = 1634: the Lanczos branch
    _, top, kappa = cr.scaled_spectrum(A)
    w = np.linalg.eigvalsh(cr.jacobi_scale(A)[1])
    assert abs(top - w[-1]) <= 1e-4 * w[-1] and abs(kappa - w[-1] / w[0]) <= 1e-3 * kappa


@pytest.mark.parametrize("scene", list(cr.SCENES))
def test_reference_on_reduced_camera_systems(oracle, scene):
    from privacy_preserving_sfm_amd.device import plan_ordering
    sc = cr.make_scene(scene)
    order, info = plan_ordering(sc)
    assert info["block_sparse"] == (scene == "sequence150") and (info["chains"] >= 2) == (scene == "sequence150")
    for radius in cr.RADII:
        ref = oracle.ba_reduced_system(sc, radius)
        A, b = cr.camera_system(sc, ref["S"], ref["rhs"], order if info["reordered"] else None)
        assert A.shape[0] == ref["nc"] == len(cr.var_cols(sc))
        _check(cr.Reference(A, b), (scene, radius))
