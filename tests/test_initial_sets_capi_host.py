"""CPU-only checks of the C ABI of K15 (pp_tracks_find_initial_sets): the symbols are exported and declared, the structs have the layout the header states,
and every argument that can be judged without the handle is PP_ERR_INVALID - an error code, not an abort - before any device work and before the handle is
read (the cases here pass a handle that must never be dereferenced).  A check image that is out of range or outside the subset needs the handle's image
count and runs in tests/test_gpu_initial_sets.py, with the calls themselves."""
import ctypes as C
import os
import re

import pytest

import initial_sets_scenes as scenes
from privacy_preserving_sfm_amd import _capi
from privacy_preserving_sfm_amd.device import TracksProblem, init_sets_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pp_init_sets_options_default", "pp_tracks_find_initial_sets")


def test_the_symbols_are_exported_and_declared():
    L = _capi.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppsfm_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert name in _capi.exported_symbols() and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert "pp_init_sets_options" in text and "pp_init_sets_report" in text
    assert C.sizeof(_capi.InitSetsOptions) == 4 * 4 + 8
    assert C.sizeof(_capi.InitSetsReport) == 4 * 8 + 6 * 4 + 3 * 8


def test_the_defaults_are_the_references():
    o = init_sets_options()
    assert (o.min_num_aligned_tracks, o.min_num_random_tracks, o.max_num_sets, o.max_candidates) == (20, 20, 10, 1 << 24)
    with pytest.raises(AttributeError):
        init_sets_options(min_tracks=3)


def _call(h, o, aligned, subset, check, num_check, rep, sets=True, track_lines=None, capacity=0):
    si, sa, sr, ts = (C.c_int32 * 40)(), (C.c_int32 * 10)(), (C.c_int32 * 10)(), (C.c_int64 * 21)()
    return _capi.lib().pp_tracks_find_initial_sets(h, o, aligned, subset, check, num_check, rep, si if sets else None, sa if sets else None, sr if sets else None,
                                                   ts if sets else None, track_lines, capacity)


def test_invalid_arguments_are_refused_before_the_handle_is_read():
    L = _capi.lib()
    o, rep = init_sets_options(), _capi.InitSetsReport()
    aligned, check, lines = (C.c_uint8 * 8)(), (C.c_int32 * 3)(0, 1, 2), (C.c_int32 * 16)()
    bogus = C.c_void_p(1)      # never dereferenced: every case below is refused on its other arguments first
    ok = dict(h=bogus, o=C.byref(o), aligned=aligned, subset=None, check=check, num_check=3, rep=C.byref(rep))
    assert _call(**dict(ok, h=None)) == _capi.PP_ERR_INVALID
    assert b"pp_tracks_find_initial_sets" in L.pp_last_error()
    for missing in ("o", "aligned", "check", "rep"):
        assert _call(**dict(ok, **{missing: None})) == _capi.PP_ERR_INVALID, missing
    for n in (0, -1):
        assert _call(**dict(ok, num_check=n)) == _capi.PP_ERR_INVALID
    assert _call(**dict(ok, check=(C.c_int32 * 3)(0, -1, 2))) == _capi.PP_ERR_INVALID      # a negative check image
    assert _call(**dict(ok, check=(C.c_int32 * 3)(2, 0, 2))) == _capi.PP_ERR_INVALID       # a repeated one
    assert b"twice" in L.pp_last_error()
    for field in ("min_num_aligned_tracks", "min_num_random_tracks", "max_num_sets", "max_candidates"):
        bad = init_sets_options(**{field: -1})
        assert _call(**dict(ok, o=C.byref(bad))) == _capi.PP_ERR_INVALID, field
        assert b"bad options" in L.pp_last_error()
    assert _call(**dict(ok, o=C.byref(init_sets_options(max_candidates=1 << 31)))) == _capi.PP_ERR_INVALID      # beyond what the sort's 32-bit sizes hold
    assert _call(capacity=4, **ok) == _capi.PP_ERR_INVALID            # capacity without track_lines
    assert _call(capacity=-1, track_lines=lines, **ok) == _capi.PP_ERR_INVALID
    assert _call(sets=False, **ok) == _capi.PP_ERR_INVALID            # max_num_sets = 10 without the set arrays
    assert b"set arrays" in L.pp_last_error()


def test_no_cpu_path_without_a_device():
    n = C.c_int()
    _capi.lib().pp_device_count(C.byref(n))
    if n.value:
        return      # (tests/test_gpu_initial_sets.py runs the calls)
    with pytest.raises(_capi.PPError) as e:
        TracksProblem(scenes.to_flat(scenes.three_neighbours()))
    assert e.value.code == _capi.PP_ERR_HIP
