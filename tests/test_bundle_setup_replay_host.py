"""csrc/bundle_setup_replay.hpp - the host half of pp_tracks_bundle_setup (K16) - without a device and under the sanitizers: the header is std only,
tests/bundle_setup_replay_host_driver.cpp compiles with g++ -fsanitize=address,undefined and is fed configs and pose lists derived from
BundleAdjuster.flatten() on the worlds of tests/bundle_setup_worlds.py.  What the header decides - pose_const, pose_tvec_mask, pose_camera, the camera order
and camera_const_mask - must equal flatten()'s element for element; the de-duplication of the point lists keeps first occurrences; the exact count of
observations and points equals flatten()'s; the validation names what is wrong.  A sanitizer report ends the driver with a non-zero status."""
import os
import subprocess

import numpy as np
import pytest

import bundle_setup_worlds as bsw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE, CONST_POSE = 1, 2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bundle_setup_replay") / "bundle_setup_replay_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "bundle_setup_replay_host_driver.cpp")])
    return exe


def _run(exe, script):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    return [l.split() for l in out.stdout.splitlines()]


def _join(values):
    return " ".join(str(int(v)) for v in values)


def _config_script(rec, cfg, opt):
    """the config as pp_bundle_config states it, over the handle's indices: images, cameras and points in ascending id"""
    image_ids, cam_ids, point_ids = sorted(rec.images), sorted(rec.cameras), sorted(rec.points3D)
    cam_index, point_index = {c: k for k, c in enumerate(cam_ids)}, {p: k for k, p in enumerate(point_ids)}
    flags = [(IMAGE | (CONST_POSE if (not opt.refine_extrinsics) or cfg.HasConstantPose(i) else 0)) if cfg.HasImage(i) else 0 for i in image_ids]
    tvec = [sum(1 << x for x in cfg.ConstantTvec(i)) if cfg.HasConstantTvec(i) else 0 for i in image_ids]
    script = ["config %d %d" % (len(image_ids), len(cam_ids)), _join(flags), _join(tvec), _join(cfg.IsConstantCamera(c) for c in cam_ids)]
    if opt.refine_focal_length or opt.refine_principal_point or opt.refine_extra_params:
        masks = []
        for c in cam_ids:
            cam = rec.cameras[c]
            idxs = ([] if opt.refine_focal_length else list(cam.FocalLengthIdxs())) + ([] if opt.refine_principal_point else list(cam.PrincipalPointIdxs())) + \
                   ([] if opt.refine_extra_params else list(cam.ExtraParamsIdxs()))
            masks.append(sum(1 << x for x in idxs))
        script.append(_join(masks))
    else:
        script.append("none")
    script.append(_join(cam_index[rec.images[i].camera_id] for i in image_ids))
    variable, constant = [point_index[p] for p in sorted(cfg.VariablePoints())], [point_index[p] for p in sorted(cfg.ConstantPoints())]
    script.append("points %d %s %d %s" % (len(variable), _join(variable), len(constant), _join(constant)))
    return script, image_ids, cam_ids, point_ids


def _state_script(rec):
    """the tracks state of a handle over the reconstruction: lines numbered image by image"""
    image_ids, point_ids = sorted(rec.images), sorted(rec.points3D)
    point_index = {p: k for k, p in enumerate(point_ids)}
    offset, line_image, line_point = {}, [], []
    for c, i in enumerate(image_ids):
        offset[i] = len(line_image)
        for line in rec.images[i].lines:
            line_image.append(c)
            line_point.append(point_index[line.Point3DId()] if line.HasPoint3D() else -1)
    script = ["state %d %d %d" % (len(image_ids), len(point_ids), len(line_image)), _join(line_image), _join(line_point),
              _join(getattr(rec.images[i], "registered", True) for i in image_ids), _join(0 for _ in point_ids)]
    for p in point_ids:
        track = [offset[i] + idx for i, idx in rec.points3D[p].track]
        script.append("%d %s" % (len(track), _join(track)))
    return script


def _row(out, name):
    rows = [r for r in out if r[0] == name]
    assert len(rows) == 1, name
    return [int(x) for x in rows[0][1:]]


def _cases():
    rec = bsw.world_a()
    yield "local_refine_off", rec, bsw.local_config(rec), bsw.options(False)
    yield "local_focal_extra", rec, bsw.local_config(rec), bsw.options(True)
    yield "global_refine_off", rec, bsw.global_config(rec), bsw.options(False)
    yield "global_focal_extra", rec, bsw.global_config(rec), bsw.options(True)
    fixed = bsw.options(True)
    fixed.refine_extrinsics = False
    yield "local_extrinsics_fixed", rec, bsw.local_config(rec), fixed
    rec_c = bsw.world_a()
    yield "image_without_observation", rec_c, bsw.empty_image_config(rec_c), bsw.options(True)
    rec_d, cfg_d = bsw.bookkeeping_world()
    yield "bookkeeping", rec_d, cfg_d, bsw.options(True)


CASES = list(_cases())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_poses_and_cameras_equal_flatten(driver, case):
    _, rec, cfg, opt = case
    scene, pose_index, point_index, cam_index = bsw.flatten(rec, cfg, opt)
    script, image_ids, cam_ids, _ = _config_script(rec, cfg, opt)
    image_index = {i: c for c, i in enumerate(image_ids)}
    poses = [image_index[i] for i in pose_index]      # the pose list in the order of first appearance: what the device hands the replay
    out = _run(driver, script + ["poses %d %s" % (len(poses), _join(poses))] + _state_script(rec) + ["validate", "count"])
    assert _row(out, "pose_const") == scene["pose_const"].tolist()
    assert _row(out, "pose_tvec") == scene["tvec_const_mask"].tolist()
    assert _row(out, "pose_camera") == scene["pose_camera"].tolist()
    assert [cam_ids[k] for k in _row(out, "cameras")] == list(cam_index)
    assert _row(out, "camera_mask") == scene["camera_const_mask"].tolist()
    assert ["valid"] in out
    assert _row(out, "count") == [len(scene["lines"]), len(point_index)]


def test_the_local_config_has_what_it_is_meant_to_have():
    """one camera only seen from outside the config (constant), one in camera_const, one variable; a constant config pose, a tvec mask, outside observers"""
    rec = bsw.world_a()
    scene, pose_index, _, cam_index = bsw.flatten(rec, bsw.local_config(rec), bsw.options(True))
    assert list(pose_index)[:3] == [0, 1, 3] and len(pose_index) > 3
    masks = dict(zip(cam_index, scene["camera_const_mask"].tolist()))
    assert masks[1] == 0xFFFF and masks[2] == 0xFFFF and masks[0] not in (0, 0xFFFF)
    assert scene["pose_const"].tolist()[:3] == [1, 0, 0] and all(scene["pose_const"][3:]) and scene["tvec_const_mask"].tolist()[:3] == [0, 1, 0]
    off = bsw.flatten(rec, bsw.local_config(rec), bsw.options(False))[0]
    assert off["camera_const_mask"].tolist() == [0xFFFF] * 3


def test_an_image_without_observation_gets_no_pose():
    rec = bsw.world_a()
    cfg = bsw.empty_image_config(rec)
    _, pose_index, _, _ = bsw.flatten(rec, cfg, bsw.options(False))
    assert cfg.HasImage(4) and 4 not in pose_index


def test_dedup_keeps_first_occurrences(driver):
    script = ["config 2 1", "1 1", "none", "none", "none", "0 0", "points 6 5 2 5 7 2 0 4 7 3 3 9", "dedup 10"]
    out = _run(driver, script)
    assert _row(out, "list") == [5, 2, 7, 0, 3, 9]
    #                         0  1  2  3  4  5  6  7  8  9      1: listed, 2: in constant_points (7 and 3 and 9; 7 also variable)
    assert _row(out, "mark") == [1, 0, 1, 3, 0, 1, 0, 3, 0, 3]


def test_validation_names_what_is_wrong(driver):
    rec = bsw.world(3, 5, 3)
    state = _state_script(rec)
    state[3] = "1 1 0"       # image 2 is not registered
    state[4] = "0 0 0 1 0"   # point 3 is deleted
    state[-1] = "0 "         # point 4 has an empty track

    def verdict(flags, points):
        out = _run(driver, ["config 3 1", flags, "none", "none", "none", "0 0 0", points] + state + ["validate"])
        return " ".join([r for r in out if r[0] in ("valid", "invalid")][0])

    assert verdict("1 1 0", "points 2 0 1 1 2") == "valid"
    assert "image 2 of the config is not registered" in verdict("1 0 1", "points 0 0")
    assert "variable point 3 is deleted" in verdict("1 1 0", "points 2 0 3 0")
    assert "constant point 4 is deleted or has an empty track" in verdict("1 1 0", "points 1 0 1 4")
    assert "variable point 5 of 5" in verdict("1 1 0", "points 1 5 0")
    assert "constant point -1 of 5" in verdict("1 1 0", "points 0 1 -1")
