"""csrc/tracks_image_replay.hpp (the host replay of TriangulateImage, std only) under AddressSanitizer and UBSan in a stand-alone program
(tests/tracks_image_replay_host_driver.cpp, plain g++): it is fed canned speculative answers - what the Python oracle answers for each line ALONE on the
untouched state, stale ones included - and, for a line it decides to redo, the oracle's answer on the state the sequential loop meets; its events,
counts and tracks must equal the oracle's sequential run.  No device, nothing loaded into Python."""
import copy
import os
import shutil
import subprocess

import pytest

import tracks_image_reference as tir
import tracks_image_scenes as scenes
from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the host replay driver")
    exe = str(tmp_path_factory.mktemp("replay") / "tracks_image_replay_host_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "privacy_preserving_sfm_amd", "csrc"), os.path.join(ROOT, "tests", "tracks_image_replay_host_driver.cpp"), "-o", exe])
    return exe


def _answer(decision, line_index, point_index):
    """a decision of the oracle as the words of one ImageLineResult; point_index(id) -> device index (new points: the order of creation)"""
    if decision is None:
        return "0 0 -1 0 0"
    ev = list(decision["events"])
    cont = -1
    if decision["continued"]:
        cont = point_index(ev[0][0])
        ev = ev[1:]
    created = decision["created"]
    sets, rounds, xyz = [], [], []
    for k, pid in enumerate(created):
        for p, el in ev:
            if p == pid:
                sets.append(line_index[el]); rounds.append(k + 1)
        xyz.extend(decision["xyz"][pid])
    lst = [line_index[el] for el in decision["list"]]
    ntri = sum(1 for t in decision["list_has_point"] if t)
    words = [len(lst)] + lst + [ntri, cont, len(sets)] + sets + rounds + [len(created)] + [repr(float(v)) for v in xyz]
    return " ".join(str(w) for w in words)


def _run_one(rec, graph, oo, image_id, line_indices):
    """the oracle over `line_indices` of the image on `rec` (changed in place) -> its decisions, each with the positions of the points it created and, per
    list entry, whether it had a point BEFORE the line was visited"""
    o = tir.ImageOracle(graph, rec)
    find = o.Find
    had = {}

    def spy(options, iid, idx, t):
        n, corrs = find(options, iid, idx, t)
        had[(iid, idx)] = [c.line.HasPoint3D() for c in corrs]
        return n, corrs
    o.Find = spy
    o.TriangulateImage(oo, image_id, line_indices)
    for d in o.decisions:
        d["xyz"] = {pid: [float(v) for v in rec.points3D[pid].xyz] for pid in d["created"]}
        d["list_has_point"] = had[d["line"]]
    return o


def _canned_run(driver, world, image_id, oo):
    rec, graph = world
    flat, point_ids, line_ref = IncrementalTriangulator(graph, rec).flatten()
    assert point_ids == list(range(len(point_ids)))
    line_index = {el: l for l, el in enumerate(line_ref)}
    P0 = len(point_ids)
    num_lines = len(rec.images[image_id].lines)
    # the speculative answers: every line alone on a copy of the untouched state (a point it creates is index P0, P0 + 1, ... of ITS answer only)
    spec = []
    for idx in range(num_lines):
        o1 = _run_one(copy.deepcopy(rec), graph, oo, image_id, [idx])
        spec.append(_answer(o1.decisions[0] if o1.decisions else None, line_index, lambda pid: pid))
    # the sequential run: its decisions are what a fresh evaluation answers
    seq = _run_one(copy.deepcopy(rec), graph, oo, image_id, None)
    by_line = {d["line"]: d for d in seq.decisions}
    fresh = [_answer(by_line.get((image_id, idx)), line_index, lambda pid: pid) for idx in range(num_lines)]
    # which lines the replay has to redo, derived here from the oracle's events alone: a line it read changed before its turn
    changed, redone = set(), 0
    for idx in range(num_lines):
        d = by_line.get((image_id, idx))
        o1 = spec[idx].split()
        read = {line_index[(image_id, idx)]} | set(int(v) for v in o1[1:1 + int(o1[0])])
        redone += bool(read & changed)
        if d is not None:
            changed |= set(line_index[el] for _, el in d["events"])
    words = [str(len(line_ref))] + [str(v) for v in flat["line_image"]] + [str(v) for v in flat["corr_start"]] + [str(v) for v in flat["corr_line"]]
    words += [str(len(flat["image_registered"]))] + [str(int(v)) for v in flat["image_registered"]] + [str(P0)]
    for p in range(P0):
        track = flat["track_line"][flat["track_start"][p]:flat["track_start"][p + 1]]
        words += [repr(float(v)) for v in flat["points"][p]] + [str(len(track))] + [str(v) for v in track]
    words.append(str(num_lines))
    for idx in range(num_lines):
        words += [str(line_index[(image_id, idx)]), spec[idx], fresh[idx]]
    out = subprocess.run([driver], input=" ".join(words), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [[int(v) for v in r.split()] for r in out.stdout.strip().split("\n")]
    error, num_tris, created, continued, got_redone, nev = rows[0]
    events = [(p, line_ref[l]) for p, l in rows[1:1 + nev]]
    tracks = [[line_ref[l] for l in r[1:]] for r in rows[2 + nev:]]
    return dict(error=error, num_tris=num_tris, created=created, continued=continued, redone=got_redone, events=events, tracks=tracks), seq, redone


@pytest.mark.parametrize("scene", [s for s in scenes.HAND_BUILT if "c" not in s()[1]["ops"]], ids=lambda f: f.__name__)
def test_replay_of_hand_built_scene(scene, driver, oracle):
    w, want = scene()
    oo = tir.Options(max_transitivity=want.get("transitivity", 1), **scenes.TIGHT)
    got, seq, redone = _canned_run(driver, (w.rec, w.graph), want["image"], oo)
    assert got["error"] == 0 and got["events"] == seq.events == want["events"]
    assert got["num_tris"] == want["num_changed"] and got["redone"] == redone == want["redone"]
    assert got["created"] == len(seq.created) and got["continued"] == seq.num_continued


@pytest.mark.parametrize("transitivity", [1, 2])
def test_replay_of_synthetic_scene(transitivity, driver, oracle):
    """stale answers in numbers: every conflict of the scene is redone with the sequential answer, and the result is the sequential loop's"""
    spec = scenes.SYNTHETIC[0]
    world = scenes.synthetic_world(spec["cfg"], spec["seed"], spec["image"])
    got, seq, redone = _canned_run(driver, world, spec["image"], tir.Options(max_transitivity=transitivity))
    assert got["error"] == 0 and got["events"] == seq.events and got["redone"] == redone
    assert got["created"] == len(seq.created) > 0 and got["continued"] == seq.num_continued > 0
    assert (redone > 0) or transitivity == 1
    for pid in seq.created:
        assert got["tracks"][pid] == seq.rec.points3D[pid].track
