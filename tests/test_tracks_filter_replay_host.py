"""csrc/tracks_filter_replay.hpp - the sequential half of pp_tracks_filter_points / pp_tracks_filter_negative_depth / pp_tracks_filter_images - without a device
and under the sanitizers: the header is std only, tests/tracks_filter_replay_host_driver.cpp compiles with g++ -fsanitize=address,undefined as a stand-alone
program and is fed, for every scene of tracks_filter_scenes.py and every operation of it, the verdicts the plain-Python reference gives (what the kernels compute
on the device).  Events, counts and the final state must equal the reference's.  A sanitizer report ends the driver with a non-zero status, which fails the test."""
import os
import subprocess

import pytest

import tracks_filter_reference as ref
import tracks_filter_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tracks_filter_replay") / "tracks_filter_replay_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "tracks_filter_replay_host_driver.cpp")])
    return exe


def _run(exe, script):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    return [l.split() for l in out.stdout.splitlines()]


def _ints(a):
    return " ".join(str(int(x)) for x in a)


def _state_script(ix):
    _, _, tracks = ix.state()
    script = ["state %d %d %d" % (len(ix.image_ids), len(ix.line_ref), len(ix.point_ids)), "line_image " + _ints(ix.flat["line_image"]),
              "registered " + _ints(ix.flat["image_registered"])]
    return script + ["track %d %d %s" % (p, len(t), _ints(t)) for p, t in enumerate(tracks) if t]


def _op_script(ix, op, got_after):
    """the driver's input for one op: the device's verdicts, here the reference's.  Called with the state BEFORE the op for depth / images; the point filter's
    verdicts come out of the reference's own run (got_after)."""
    kind = op[0]
    if kind == "depth":
        return ["depth %d %s" % (len(ix.image_order()), _ints(ix.image_order())), _ints(ix.depth_flags())]
    if kind == "images":
        return ["images %d %s" % (len(ix.image_order()), _ints(ix.image_order())), _ints(ix.skip_flags())]
    lines, flags = [], []
    for pid in ix.point_ids:
        v = got_after["verdicts"].get(pid)
        if v is None:      # not tested: its flags are zero, as the kernel's memset leaves them
            lines.append("0 0 -0x1p+0")
            flags += [0] * len(got_after["tracks_before"][pid])
        else:
            lines.append("%d %d %s" % (v[0], v[1], float(got_after["errors"].get(pid, -1.0)).hex()))
            flags += v[2]
    return ["points " + " ".join(lines), _ints(flags)]


def _check(out, ix, got):
    events = [(int(r[1]), int(r[2])) for r in out if r[0] == "event"]
    assert events == ix.events(got["events"])
    counts = [int(x) for x in [r for r in out if r[0] == "counts"][0][1:]]
    assert counts[:3] == [got["num_filtered"], got["point_deleted"], got["obs_deleted"]]
    if "tested" in got:
        assert counts[3] == got["tested"]
        assert {int(r[1]): float.fromhex(r[2]) for r in out if r[0] == "error"} == {ix.point_index[p]: e for p, e in got["errors"].items()}
    if "filtered" in got:
        assert counts[4] == len(got["filtered"])
        assert [int(x) for x in [r for r in out if r[0] == "filtered"][0][1:]] == [ix.image_index[i] for i in got["filtered"]]
    line_point, deleted, tracks = ix.state()
    assert [int(x) for x in [r for r in out if r[0] == "line_point"][0][1:]] == list(line_point)
    assert [int(x) for x in [r for r in out if r[0] == "deleted"][0][1:]] == list(deleted)
    assert [[int(x) for x in r[2:]] for r in out if r[0] == "track"] == tracks
    reg = set(ix.rec.RegImageIds())
    assert [int(x) for x in [r for r in out if r[0] == "registered"][0][1:]] == [int(i in reg) for i in ix.image_ids]


@pytest.mark.parametrize("name,build", scenes.all_scenes(), ids=[n for n, _ in scenes.all_scenes()])
def test_replay_equals_the_reference(driver, name, build):
    rec, graph, ops, _ = build()
    ix = ref.Indexed(rec, graph)
    script = _state_script(ix)
    for op in ops:      # the driver keeps ONE state over the ops, as a live handle does: every op is checked on the state the ones before left
        before = len(script)
        tracks_before = {p: list(rec.points3D[p].track) if p in rec.points3D else [] for p in ix.point_ids}
        pre = _op_script(ix, op, None) if op[0] != "points" else None
        got = ref.run_op(rec, op)
        got["tracks_before"] = tracks_before
        script += pre if pre is not None else _op_script(ix, op, got)
        out = _run(driver, script + ["dump"])
        skip = sum(1 for l in script[:before] if l.split()[0] in ("points", "depth", "images"))      # the output of the ops before this one
        starts = [k for k, r in enumerate(out) if r[0] == "counts"]
        first = 0 if skip == 0 else starts[skip - 1] + 1
        while skip and first < len(out) and out[first][0] in ("error", "filtered"):
            first += 1
        _check(out[first:], ix, got)


def test_the_registration_order_is_checked(driver):
    rec, graph, _, _ = scenes.registration_order()
    rec.images[5].registered = False
    ix = ref.Indexed(rec, graph)
    order = ix.image_order()
    assert 5 not in order and len(order) == 23
    L, C = len(ix.line_ref), len(ix.image_ids)
    zeros = _ints([0] * L)
    out = _run(driver, _state_script(ix) + ["order %d %s" % (len(order), _ints(order)), "order %d %s" % (len(order) - 1, _ints(order[:-1])),
                                            "order %d %s" % (len(order), _ints(order[:-1] + [order[0]])), "order %d %s" % (len(order) + 1, _ints(order + [5])),
                                            "order %d %s" % (len(order), _ints(order[:-1] + [C])), "depth %d %s" % (len(order) - 1, _ints(order[:-1])), zeros, "dump"])
    assert [r[1] for r in out if r[0] == "order"] == ["1", "0", "0", "0", "0"]
    assert ["invalid"] in out and not [r for r in out if r[0] in ("event", "counts")]
    line_point, deleted, tracks = ix.state()
    assert [int(x) for x in [r for r in out if r[0] == "line_point"][0][1:]] == list(line_point)      # nothing changed
