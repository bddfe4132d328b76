"""The judge of pp_ba_covariance_blocks tested on the host, before any device sees it: the blocks tests/covariance_blocks_reference.py forms from the Schur
route (G = S^-1, W V^-1, V^-1) must be the slices of the dense inverse of the full H, which knows nothing of a Schur complement.  Limit: the dense route's
own first-order forward error kappa_2(H_scaled) sqrt(free columns of H) u, u = 2^-53, in the suite's block error e.  Also the host side of the Python
mirror: how BAProblem.covariance_blocks lays its request out and cuts the output, with the library call stubbed.

Observed (worst e over the sampled blocks of every kind, limit):
    cfg1                               8.54e-14  6.61e-12   (kappa(H_scaled) 2.03e+03, 863 free columns; pose x point 6.62e-14)
    cfg1 shared camera, f k variable   1.91e-12  3.79e-09   (kappa(H_scaled) 1.16e+06, 865 free columns; pose x point 1.85e-12)
With SchurCovariance.inv (S formed in float64) in the judge's place the same two lines read 4.75e-14 (pose x point 3.78e-14) and 1.18e-10 (1.13e-10): the
1.1e-10 is the float64 Schur complement's, not the dense route's - test_the_float64_schur_complement_is_what_limits_the_refined_route pins that."""
import ctypes as C

import numpy as np
import pytest

import covariance_blocks_reference as cbr
import covariance_reference as cr
from privacy_preserving_sfm_amd import _capi, synthetic

CFG1 = dict(num_cams=20, num_points=250, track=8, seed=0xC0FFEE + 1, model=2)


def _shared_camera_scene():
    sc = synthetic.make_ba_scene(**CFG1)
    sc["camera_const_mask"][:] = 0xFFFF & ~0b1001      # SIMPLE_RADIAL: f and k variable
    return sc


def _request(sc, rng):
    Cn, Pn, Kn = sc["poses"].shape[0], sc["points"].shape[0], sc["intr"].shape[0]
    pts = [int(p) for p in range(0, Pn, 17)]
    blocks = [(("pose", i), ("point", p)) for i in range(Cn) for p in pts]
    blocks += [(("point", p), ("pose", i)) for i in (0, 1, 7) for p in pts]
    blocks += [(("pose", i), ("pose", j)) for i in range(Cn) for j in (0, 1, i)]
    blocks += [(("point", int(p)), ("point", int(q))) for p, q in rng.integers(0, Pn, (60, 2))] + [(("point", 3), ("point", 3))]
    for k in range(Kn):
        blocks += [(("intrinsics", k), ("intrinsics", k))] + [(("pose", i), ("intrinsics", k)) for i in range(Cn)] + [(("intrinsics", k), ("point", p)) for p in pts]
    return blocks


@pytest.mark.parametrize("name", ["cfg1", "cfg1 shared camera"])
def test_schur_blocks_are_the_slices_of_the_dense_inverse(oracle, name):
    sc = synthetic.make_ba_scene(**CFG1) if name == "cfg1" else _shared_camera_scene()
    dense, schur = cr.dense_covariance(sc), cr.SchurCovariance(sc)
    ref = cbr.SchurBlocks(schur)
    limit = dense.kappa * np.sqrt(dense.lin.free.sum()) * cr.U
    worst = {}
    for a, b in _request(sc, np.random.default_rng(11)):
        want = cbr.dense_block(dense, a, b)
        got = ref.block(a, b)
        assert got.shape == want.shape == (cbr.WIDTH[a[0]], cbr.WIDTH[b[0]])
        assert np.array_equal(got == 0, want == 0), (a, b)      # the zero rows and columns are the same ones
        e = cr.block_error(got, want, cbr.dense_block(dense, a, a), cbr.dense_block(dense, b, b))
        worst[(a[0], b[0])] = max(worst.get((a[0], b[0]), 0.0), e)
    print("%s: kappa(H_scaled) %.2e free columns %d limit %.2e worst by kinds %s" % (name, dense.kappa, dense.lin.free.sum(), limit,
                                                                                       {k: "%.2e" % v for k, v in worst.items()}))
    assert max(worst.values()) <= limit, worst
    # what is constant: pose 0, tvec[1].x; with the shared camera every slot but f (0) and k (3)
    assert not ref.block(("pose", 0), ("point", 17)).any() and not ref.block(("point", 17), ("pose", 1))[:, 3].any()
    kk = ref.block(("intrinsics", 0), ("intrinsics", 0))
    live = [0, 3] if name != "cfg1" else []
    assert all(kk[j].any() == (j in live) and kk[:, j].any() == (j in live) for j in range(12))
    if live:
        assert np.linalg.eigvalsh(kk[np.ix_(live, live)])[0] > 0


def test_a_point_block_is_the_schur_references_own(oracle):
    sc = synthetic.make_ba_scene(**CFG1)
    schur = cr.SchurCovariance(sc)
    ref = cbr.SchurBlocks(schur)
    for p in (0, 17, 249):
        assert np.allclose(ref.block(("point", p), ("point", p), "inv"), schur.point(p), rtol=1e-13, atol=0)
        assert np.allclose(ref.block(("point", p), ("point", p), "plain"), schur.point(p, True), rtol=1e-13, atol=0)
    for i, j in ((1, 1), (3, 19), (0, 4)):
        assert np.array_equal(ref.block(("pose", i), ("pose", j), "inv"), schur.pose(i, j))


def test_the_float64_schur_complement_is_what_limits_the_refined_route(oracle):
    """why covariance_blocks_reference judges by an S formed in long double: on the shared-camera scene the dense route, which never forms S, sits far closer
    to it than to SchurCovariance.inv, in every kind of block, and the bar kappa(S_scaled) sqrt(n) u lies between the two distances"""
    sc = _shared_camera_scene()
    dense, schur = cr.dense_covariance(sc), cr.SchurCovariance(sc)
    ref = cbr.SchurBlocks(schur)
    to_ld, to_inv = 0.0, 0.0
    for a, b in [(("pose", 3), ("pose", 3)), (("pose", 7), ("point", 17)), (("intrinsics", 0), ("intrinsics", 0)), (("point", 5), ("point", 200)), (("intrinsics", 0), ("point", 9))]:
        want, da, db = cbr.dense_block(dense, a, b), cbr.dense_block(dense, a, a), cbr.dense_block(dense, b, b)
        to_ld = max(to_ld, cr.block_error(ref.block(a, b), want, da, db))
        to_inv = max(to_inv, cr.block_error(ref.block(a, b, "inv"), want, da, db))
    bar = schur.kappa * np.sqrt(schur.n) * cr.U
    print("shared camera: dense to the long-double S %.2e, dense to the float64 S %.2e, kappa(S_scaled) sqrt(n) u %.2e" % (to_ld, to_inv, bar))
    assert to_ld < bar < to_inv


def test_python_mirror_lays_out_the_request_and_cuts_the_output(monkeypatch):
    from privacy_preserving_sfm_amd import device
    seen = {}

    class Lib:
        @staticmethod
        def pp_ba_options_default(o):
            return 0

        @staticmethod
        def pp_ba_covariance_blocks(h, o, num, req, out, capacity, info):
            seen["req"] = [(req[q].kind_a, req[q].index_a, req[q].kind_b, req[q].index_b) for q in range(num)]
            seen["capacity"] = capacity
            for i in range(capacity):
                out[i] = float(i)
            return 0

    monkeypatch.setattr(_capi, "lib", lambda: Lib)
    pb = device.BAProblem.__new__(device.BAProblem)
    pb._h = C.c_void_p()
    blocks = [(("pose", 4), ("point", 9)), (("intrinsics", 2), ("intrinsics", 0)), (("point", 1), ("point", 1)), (("point", 5), ("intrinsics", 1)), (("pose", 0), ("pose", 3))]
    out, info = pb.covariance_blocks(blocks, return_info=True)
    assert seen["req"] == [(0, 4, 2, 9), (1, 2, 1, 0), (2, 1, 2, 1), (2, 5, 1, 1), (0, 0, 0, 3)]
    assert seen["capacity"] == 18 + 144 + 9 + 36 + 36
    assert [b.shape for b in out] == [(6, 3), (12, 12), (3, 3), (3, 12), (6, 6)]
    first = 0
    for b in out:      # block q row-major at the prefix sum of the sizes before it
        assert np.array_equal(b.ravel(), np.arange(first, first + b.size))
        first += b.size
    assert isinstance(info, _capi.BACovarianceInfo)
    assert pb.covariance_blocks([]) == [] and seen["capacity"] == 0
    with pytest.raises(ValueError):
        pb.covariance_blocks([(("pose", 0), ("camera", 0))])
    pb._h = None      # (nothing to destroy)


def test_symbol_is_exported_and_bound():
    L = _capi.lib()
    assert "pp_ba_covariance_blocks" in _capi.exported_symbols()
    assert hasattr(L, "pp_ba_covariance_blocks") and len(L.pp_ba_covariance_blocks.argtypes) == 7
    assert C.sizeof(_capi.CovBlock) == 16 and (_capi.COV_POSE, _capi.COV_INTRINSICS, _capi.COV_POINT) == (0, 1, 2)


def test_invalid_requests_are_refused_before_any_device_work():
    from privacy_preserving_sfm_amd.device import ba_options
    L = _capi.lib()
    o = ba_options()
    one = (_capi.CovBlock * 1)(_capi.CovBlock(0, 0, 2, 0))
    out = np.zeros(18)
    assert L.pp_ba_covariance_blocks(None, C.byref(o), 1, one, _capi.dp(out), 18, None) == _capi.PP_ERR_INVALID
    assert b"null handle" in L.pp_last_error()


def test_cpp_mirror_compiles_links_and_lays_out_the_offsets(tmp_path):
    import os
    import subprocess

    from privacy_preserving_sfm_amd import build
    build.build_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path), "cpp_covariance_blocks_compile_test")
    libdir = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-o", exe, os.path.join(root, "tests", "cpp_covariance_blocks_compile_test.cpp"), "-L" + libdir,
                           "-lppsfm_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "null handle rc=-1" in out.stdout and "offsets 0 36 180 216 288 297 315\n" in out.stdout and "ok sizeof(block)=16 member=1 empty=0" in out.stdout
