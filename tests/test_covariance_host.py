"""pp_ba_covariance on the host: the symbol is exported and bound, and a NULL handle is refused before anything touches a device."""
import ctypes as C

from privacy_preserving_sfm_amd import _capi
from privacy_preserving_sfm_amd.device import BAProblem, ba_options


def test_symbol_is_exported_and_bound():
    L = _capi.lib()
    assert "pp_ba_covariance" in _capi.exported_symbols()
    assert hasattr(L, "pp_ba_covariance") and len(L.pp_ba_covariance.argtypes) == 10
    assert C.sizeof(_capi.BACovarianceInfo) == 32
    assert callable(getattr(BAProblem, "covariance"))


def test_null_handle_is_invalid():
    L = _capi.lib()
    o = ba_options()
    info = _capi.BACovarianceInfo()
    assert L.pp_ba_covariance(None, C.byref(o), 0, None, None, None, 0, None, None, C.byref(info)) == _capi.PP_ERR_INVALID
    assert b"null handle" in L.pp_last_error()


def test_cpp_mirror_compiles_links_and_refuses_a_null_handle(tmp_path):
    import subprocess

    from covariance_cpp_driver import build_driver
    out = subprocess.run([build_driver(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "null handle rc=-1" in out.stdout and "ok sizeof(info)=32 member=1" in out.stdout
