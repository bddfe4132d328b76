"""CPU-only checks of the C ABI of K13 (pp_tracks_find_next_images / pp_tracks_estimate_image_pose / pp_tracks_register_image): the four symbols are
exported and declared, the defaults equal the reference's header (sfm/incremental_mapper.h: abs_pose_min_num_inliers 30, max_reg_trials 3,
image_selection_method MAX_VISIBLE_POINTS_RATIO), bad arguments are PP_ERR_INVALID before any device work, and without a device there is no CPU
path: the handle the three calls need cannot be created (PP_ERR_HIP)."""
import ctypes as C
import os
import re

import pytest

import register_image_scenes as scenes
from privacy_preserving_sfm_amd import _capi
from privacy_preserving_sfm_amd.device import TracksProblem, next_image_options, ransac_options
from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pp_next_image_options_default", "pp_tracks_find_next_images", "pp_tracks_estimate_image_pose", "pp_tracks_register_image")


def test_the_four_symbols_are_exported_and_declared():
    L = _capi.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppsfm_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert name in _capi.exported_symbols() and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, text), name


def test_defaults_equal_the_reference_header():
    o = next_image_options()
    assert (o.abs_pose_min_num_inliers, o.max_reg_trials, o.image_selection_method) == (30, 3, 1)
    assert C.sizeof(_capi.NextImageOptions) == 16 and C.sizeof(_capi.NextImageReport) == 40 and C.sizeof(_capi.ImagePoseReport) == 64
    assert (_capi.REG_OK, _capi.REG_FEW_VISIBLE, _capi.REG_FEW_CORRS, _capi.REG_NO_INLIERS, _capi.REG_ALIGNED, _capi.REG_NAN, _capi.REG_FEW_INLIERS) == tuple(range(7))
    # the mapper mirror's options carry the same defaults
    from privacy_preserving_sfm_amd.bundle_adjustment import IncrementalMapperOptions
    m = IncrementalMapperOptions()
    assert (m.abs_pose_max_error, m.abs_pose_min_num_inliers, m.abs_pose_min_inlier_ratio, m.abs_pose_refine_focal_length, m.abs_pose_refine_extra_params) == \
        (12.0, 30, 0.25, False, False)
    assert (m.max_reg_trials, m.image_selection_method, m.min_focal_length_ratio, m.max_focal_length_ratio, m.max_extra_param) == (3, 1, 0.1, 10.0, 1.0)


def test_bad_arguments_are_invalid_before_any_device_work():
    L = _capi.lib()
    L.pp_next_image_options_default(None)      # tolerated, as the other *_default functions
    o, r = next_image_options(), ransac_options(max_error=0.01)
    nrep, prep = _capi.NextImageReport(), _capi.ImagePoseReport()
    pose = (C.c_double * 7)(1, 0, 0, 0, 0, 0, 0)
    n = C.c_int64()
    assert L.pp_tracks_find_next_images(None, C.byref(o), None, None, C.byref(nrep), None, 0, None, None) == _capi.PP_ERR_INVALID
    assert L.pp_tracks_estimate_image_pose(None, C.byref(o), C.byref(r), 0, None, C.byref(prep), pose, None, None, None, 0) == _capi.PP_ERR_INVALID
    assert L.pp_tracks_register_image(None, 0, pose, 0, None, None, None, C.byref(n), None, None, 0) == _capi.PP_ERR_INVALID
    assert b"pp_tracks_register_image" in L.pp_last_error()


def test_no_cpu_path_without_a_device():
    n = C.c_int()
    _capi.lib().pp_device_count(C.byref(n))
    if n.value:
        return      # (tests/test_gpu_register_image.py runs the calls)
    w, _ = scenes.dedup()
    flat = IncrementalTriangulator(w.graph, w.rec).flatten()[0]
    with pytest.raises(_capi.PPError) as e:
        TracksProblem(flat)
    assert e.value.code == _capi.PP_ERR_HIP
