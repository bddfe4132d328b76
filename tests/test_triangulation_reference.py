"""The 50-digit triangulation reference (tests/triangulation_reference.py) and its golden file, checked on the CPU: the file holds the sets it is meant to
hold, the oracle (oracle/triangulation.h, in double, Jacobi on the Gram matrix) equals it in success flag, trial count and inlier mask on EVERY decided
track - no share left out - and the reference, run again, reproduces the file.  That the margin rule separates what two correct double implementations
agree on is shown here, before the device is held to the same numbers (tests/test_gpu_triangulation_exact.py)."""
import numpy as np
import pytest

import triangulation_reference as ref

SETS = ("grid", "models", "options", "degenerate")


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


def _undecided_share(s):
    return float(np.mean(np.concatenate([~r["decided"] for r in s["runs"]])))


def test_golden_sets_are_the_ones_described(golden):
    assert set(golden) == set(SETS)
    grid = golden["grid"]
    lens = np.diff(grid["scenes"][0]["track_start"])
    assert len(lens) == 129 and len(grid["scenes"][0]["view_camera"]) == 10 and list(grid["scenes"][0]["camera_model"]) == [2]
    assert set(range(13)) <= set(lens.tolist()) and all(lens[t] < 3 for t in (0, 63, 64, 65, 128)) and {0, 1, 2} <= {int(lens[t]) for t in (0, 63, 64, 65, 128)}
    assert sorted(r["options"]["residual_type"] for r in grid["runs"]) == [0, 1]
    models = golden["models"]
    assert len(models["scenes"]) == 12 and len(models["runs"]) == 24
    for m, sc in enumerate(models["scenes"][:11]):
        lens = np.diff(sc["track_start"])
        assert list(sc["camera_model"]) == [m] and len(lens) == 24 and lens.min() >= 4 and lens.max() <= 8
    mixed = models["scenes"][11]
    assert set(mixed["camera_model"].tolist()) == set(range(11)) and len(set(mixed["view_camera"].tolist())) == len(mixed["view_camera"])
    opts = golden["options"]
    lens = np.diff(opts["scenes"][0]["track_start"])
    assert len(lens) == 32 and lens.min() == 3 and lens.max() == 10
    assert opts["scenes"][1]["cam_size"].tolist() == [[1, 1]] and np.array_equal(opts["scenes"][1]["lines"], opts["scenes"][0]["lines"])
    rows = [{k: v for k, v in r["options"].items() if k not in ("residual_type", "max_error")} for r in opts["runs"] if r["scene"] == 0 and r["options"]["residual_type"] == 1]
    base = dict(min_tri_angle=0.0)
    for want in (dict(), dict(confidence=1.0), dict(confidence=0.5), dict(min_inlier_ratio=0.5), dict(max_num_trials=1), dict(max_num_trials=5), dict(min_num_trials=10 ** 6),
                 dict(dyn_num_trials_multiplier=1.0), dict(min_tri_angle=0.02), dict(min_tri_angle=0.2)):
        assert dict(base, **want) in rows, want
    assert len(np.diff(golden["degenerate"]["scenes"][0]["track_start"])) == 32
    for name in ("grid", "models", "options"):                      # the cap on the undecided share, from the margins in the file
        assert _undecided_share(golden[name]) <= 0.02, (name, _undecided_share(golden[name]))
        assert abs(golden[name]["undecided_share"] - _undecided_share(golden[name])) < 1e-12
    assert _undecided_share(golden["degenerate"]) >= 0.9               # that set is there to be undecided


def test_golden_holds_both_outcomes_of_every_decision(golden):
    """the sets are no easy ones: failures, supports of three and of more, observations on both sides of the threshold, rejected projections"""
    for name in ("grid", "models", "options"):
        runs = golden[name]["runs"]
        ok = np.concatenate([r["ok"] for r in runs])
        mask = np.concatenate([r["mask"] for r in runs])
        assert 0.05 < mask.mean() < 0.95, name
        assert (np.concatenate([r["support"] for r in runs]) >= 4).any()
        if name != "models":
            assert (~ok).any() and ok.any()
    runs = golden["models"]["runs"]                                   # the two residual types do not merely repeat each other
    assert any(not np.array_equal(a["mask"], b["mask"]) for a, b in zip(runs[0::2], runs[1::2]))


def test_empty_supports_run_every_combination(golden):
    """an image of one pixel rejects every projection: zero inliers, the trial bound is "never abort", so C(n, 3) trials capped by max_num_trials"""
    s = golden["options"]
    lens = np.diff(s["scenes"][1]["track_start"])
    seen = 0
    for r in s["runs"]:
        if r["scene"] != 1:
            continue
        cap = r["options"].get("max_num_trials", 2 ** 64 - 1)
        assert r["decided"].all() and not r["ok"].any() and not r["mask"].any()
        assert r["num_trials"].tolist() == [min(ref.n_choose_3(n), cap) for n in lens]
        seen += 1
    assert seen == 4


@pytest.mark.parametrize("name", SETS)
def test_oracle_equals_golden_on_decided_tracks(oracle, golden, name):
    s = golden[name]
    for r in s["runs"]:
        sc, o = s["scenes"][r["scene"]], r["options"]
        kw = {k: v for k, v in o.items() if k not in ("min_tri_angle", "residual_type")}
        ok, xyz, mask, nt = oracle.triangulate_tracks(sc, o["min_tri_angle"], o["residual_type"], **kw)
        ts, d = sc["track_start"], r["decided"]
        assert np.array_equal(ok[d], r["ok"][d]), (name, o, np.nonzero(d & (ok != r["ok"]))[0])
        assert np.array_equal(nt[d], r["num_trials"][d]), (name, o, np.nonzero(d & (nt != r["num_trials"]))[0])
        dobs = np.repeat(d, np.diff(ts))
        assert np.array_equal(mask[dobs], r["mask"][dobs]), (name, o)
        sel = d & r["ok"]
        if sel.any():                                                # the measurement the device's bound is made of: the file's figure covers this run
            assert np.abs(xyz[sel] - r["xyz"][sel]).max() <= s["oracle_xyz_err"][str(o["residual_type"])]


def test_reference_reproduces_the_golden_file(golden):
    """the FOV camera's 24 tracks under the pixel residual, computed again"""
    s = golden["models"]
    r = next(r for r in s["runs"] if r["scene"] == 7 and r["options"]["residual_type"] == 1)
    sc = s["scenes"][7]
    assert len(sc["track_start"]) - 1 <= 30
    res = ref.triangulate_scene(sc, r["options"])
    assert [x["ok"] for x in res] == r["ok"].tolist() and [x["num_trials"] for x in res] == r["num_trials"].tolist()
    assert [m for x in res for m in x["mask"]] == r["mask"].tolist()
    assert np.array_equal(np.array([[float(c) for c in x["xyz"]] for x in res]), r["xyz"])
    assert [ref.round_margin(x["margin"]) for x in res] == r["margin"].tolist()
    assert [x["support"] for x in res] == r["support"].tolist() and [x["near"] for x in res] == r["near"].tolist()


def test_residuals_at_a_point():
    """residuals(xyz, track): zero on a line through the projection, DBL_MAX (inf) behind the camera and outside the image"""
    P = np.hstack([np.eye(3), [[0.0], [0.0], [4.0]]])
    sc = dict(P=P[None], centers=np.array([[0.0, 0.0, -4.0]]), view_camera=[0], camera_model=[0], intr=np.array([[1000.0, 640.0, 480.0] + [0.0] * 9]), cam_size=[[1280, 960]],
              track_start=[0, 2], obs_view=[0, 0], lines=np.array([[1.0, 0.0, -0.1], [1.0, 0.0, -0.101]]))
    views = ref.scene_views(sc)
    for rt in (0, 1):
        tr = ref.scene_track(sc, views, 0, rt)
        r = ref.residuals([0.4, 0.2, 0.0], tr)
        assert abs(r[0]) < 1e-30 and r[1] > 0
        want = 1.0 if rt == 1 else 1e-3 ** 2 / (1 + 0.1 ** 2 + 0.05 ** 2) / (1 + 0.101 ** 2)
        assert abs(float(r[1]) / want - 1) < (1e-12 if rt == 1 else 2e-2)
        assert ref.residuals([0.4, 0.2, -5.0], tr) == [ref.mp.inf] * 2 and ref.residuals([3.0, 0.2, 0.0], tr) == [ref.mp.inf] * 2
        rs, seps = ref.residuals([0.4, 0.2, 0.0], tr, max_residual=1.0 if rt == 1 else 1e-6)
        assert seps[0] > 0.1 and (seps[1] < 1e-12 if rt == 1 else seps[1] > 1e-3)
