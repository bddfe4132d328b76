"""The 50-digit reference of the K6 initialisation solvers (tests/init_solvers_reference.py) and its golden file, checked on the CPU: the oracle
(oracle/init_solvers.h: Gram matrix and cyclic Jacobi in double, as the kernels) passes the exact comparison the device is held to in
tests/test_gpu_init_solvers_exact.py, sample by sample and with no share left out; samples of every set recomputed from their inputs equal the file; the
reference satisfies its own defining equations at 1e-40; the file's quantiles and shares are printed (pytest -s)."""
import numpy as np
import pytest

import init_solvers_reference as ref

mp = ref.mp
ALL_SETS = ref.FOURVIEW_SETS + ref.POSE2D_SETS + ref.PLANAR_SETS + (ref.TRACK_SET,)
TINY = mp.mpf(10) ** -40


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


def _f(rows):
    return np.array([[float(v) for v in r] for r in rows])


def test_golden_sets_are_the_ones_described(golden):
    assert set(golden) == set(ALL_SETS) | {"_meta"}
    for name in ALL_SETS:
        s = golden[name]
        assert s["n"] == (16 if name == "fourview_e" else 120 if name == ref.TRACK_SET else 48), name
        assert np.mean(~s["decided"]) <= 0.02, name
    for name in ("fourview_a", "fourview_b", "fourview_e"):
        assert golden[name]["decided"].all(), name
    assert [golden[n]["samples"].shape[1] for n in ref.FOURVIEW_SETS] == [5, 10, 5, 5, 5]
    d = golden["fourview_d"]["count"]                    # both outcomes of the discriminant, each on a twentieth of the set at least
    assert np.mean(d == 0) >= 0.05 and np.mean(d == 16) >= 0.05 and set(d.tolist()) == {0, 16}
    for name in ("fourview_a", "fourview_b", "fourview_c", "fourview_e"):
        assert (golden[name]["count"] == 16).all(), name
    # both branches of `beta > 0`: the sign of beta belongs to the scene and its frames (sets a, b and e: all positive), so sets c and d carry the other one -
    # an oracle forced into the `beta > 0` branch passes a, b and e and fails c and d (tried on a scratch copy)
    assert golden["fourview_a"]["beta_positive"].all() and not golden["fourview_c"]["beta_positive"].any()
    bd = golden["fourview_d"]["beta_positive"][d == 16]
    assert bd.any() and not bd.all()
    assert np.array_equal(golden["fourview_a"]["samples"], golden["fourview_c"]["samples"]) and golden["fourview_a"]["x"] is not None
    assert not np.array_equal(golden["fourview_a"]["frames"], golden["fourview_c"]["frames"])
    e, a = golden["fourview_e"], golden["fourview_a"]   # the hard set: every sample worse conditioned than set a's ninth decile
    assert e["K"].max(axis=1).min() > np.quantile(a["K"].max(axis=1), 0.9)
    for name in ref.FOURVIEW_SETS + ref.POSE2D_SETS:    # every bearing is a fixed point of the constructors' x / |x|
        x = golden[name]["x"]
        assert np.array_equal(x / np.sqrt(x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1])[..., None], x), name


def test_quantiles_and_shares_are_printed(golden):
    """the figures INTEGRATION.md section 1 quotes: per set the oracle's normalised error and the share of samples whose null vector the Gram route
    (2^-52 K) and a decomposition of A itself (2^-52 sqrt K) leave uncertain beyond 1e-7, the inlier threshold of the reference's own four-view test"""
    for name in ALL_SETS:
        s = golden[name]
        r = np.sort(s["oracle_rho"][s["decided"]])
        K = s["K"].max(axis=1) if s["K"].ndim == 2 else s["K"]
        print("%-18s oracle rho median %.3g, 0.9 quantile (floor) %.3g, max %.3g; K median %.3g max %.3g; share 2^-52 K > 1e-7: %.3f, with sqrt K: %.3f" % (
            name, r[len(r) // 2], s["oracle_floor"], r[-1], np.median(K), K.max(), s["share_K"], s["share_sqrtK"]))
        assert s["share_K"] == float(np.mean(ref.EPS * K > 1e-7)) and s["share_sqrtK"] == float(np.mean(ref.EPS * np.sqrt(K) > 1e-7))
        seen = sorted(s["oracle_rho"][i] for i in range(s["n"]) if s["decided"][i] and (name not in ref.FOURVIEW_SETS or s["count"][i]))
        assert s["oracle_floor"] == ref.quantile(seen, 0.9), name
    assert golden["fourview_e"]["share_K"] == 1.0 and all(golden[n]["share_sqrtK"] == 0.0 for n in ALL_SETS)


@pytest.mark.parametrize("name", ref.FOURVIEW_SETS)
def test_oracle_passes_the_fourview_comparison(oracle, golden, name):
    s = golden[name]
    cams, cnt = oracle.fourview2d_minimal(s["x"], s["samples"], s["frames"])
    worst = ref.check_fourview_decided(s, cams, cnt)
    print("%s: oracle max rho / bound = %.3g" % (name, worst))
    for i in range(s["n"]):                             # and over the draws its error is what the file says
        if s["decided"][i]:
            e = dict(count=s["count"][i], cams=s["cams"][i], K=s["K"][i])
            r = ref.oracle_fourview_rho(oracle, name, i, s["x"], s["samples"][i], s["frames"], e)
            assert r is not None and r <= s["oracle_rho"][i], (name, i, r, s["oracle_rho"][i])


@pytest.mark.parametrize("name", ref.POSE2D_SETS + ref.PLANAR_SETS)
def test_oracle_passes_the_pose_and_offset_comparison(oracle, golden, name):
    s = golden[name]
    if name in ref.POSE2D_SETS:
        got = np.array([oracle.abspose2d_nonminimal(s["x"], s["X"], smp) for smp in s["samples"]])
        worst = ref.check_rows_decided(s, got, "pose")
    else:
        worst = ref.check_rows_decided(s, oracle.planar_minimal(s["scene"], s["samples"]), "offsets")
    print("%s: oracle max rho / bound = %.3g" % (name, worst))
    for i in range(0, s["n"], 5):
        if name in ref.POSE2D_SETS:
            r = ref.oracle_pose2d_rho(oracle, name, i, s["x"], s["X"], s["samples"][i], dict(pose=s["pose"][i], K=s["K"][i]))
        else:
            r = ref.oracle_planar_rho(oracle, name, i, s["scene"], s["samples"][i], dict(offsets=s["offsets"][i], K=s["K"][i]))
        assert not s["decided"][i] or r <= s["oracle_rho"][i], (name, i, r, s["oracle_rho"][i])


def test_oracle_passes_the_track_comparison(oracle, golden):
    s = golden[ref.TRACK_SET]
    _, _, err, X = oracle.fourview2d_score(s["cams"], s["x"], 1.0)
    print("track: oracle max rho / bound = %.3g" % ref.check_track_decided(s, X, err))


def test_a_wrong_order_or_branch_fails_the_comparison(golden):
    """what the nearest-candidate matching of test_gpu_init_solvers.py let through: two flips exchanged, the roots exchanged (the other branch of
    `beta > 0`), one candidate replaced by its neighbour - each fails on every sample; the one allowed exchange passes"""
    s = golden["fourview_a"]
    cnt = s["count"]
    allowed = s["cams"][:, [k ^ 1 for k in range(16)]]
    assert ref.check_fourview_decided(s, allowed, cnt) == 0.0
    half = s["cams"].copy()
    half[:, :8] = allowed[:, :8]                         # the exchange in one root and not in the other: allowed too (one sign per null vector)
    assert ref.check_fourview_decided(s, half, cnt) == 0.0
    wrong = [s["cams"][:, [(k & 8) | ((k & 4) >> 1) | ((k & 2) << 1) | (k & 1) for k in range(16)]],     # flip1 <-> flip2
             s["cams"][:, [k ^ 8 for k in range(16)]],                                                     # root 0 <-> root 1
             s["cams"][:, [1, 1] + list(range(2, 16))]]                                                    # candidate 0 lost, candidate 1 twice
    for cams in wrong:
        for i in range(s["n"]):
            one = dict(s, n=1, decided=s["decided"][i:i + 1], count=cnt[i:i + 1], cams=s["cams"][i:i + 1], K=s["K"][i:i + 1], oracle_rho=s["oracle_rho"][i:i + 1])
            with pytest.raises(AssertionError):
                ref.check_fourview_decided(one, cams[i:i + 1], cnt[i:i + 1])
    moved = s["cams"].copy()
    median = int(np.argsort(s["K"].max(axis=1))[s["n"] // 2])
    moved[median, 5, 3, 0, 2] += 1e-6                    # one entry of one fourth camera of the median sample off by 1e-6: orders beyond its bound
    with pytest.raises(AssertionError):
        ref.check_fourview_decided(s, moved, cnt)


@pytest.mark.parametrize("name", ALL_SETS)
def test_reference_reproduces_the_golden_file(golden, name):
    """three samples per set, recomputed from the inputs the file holds"""
    s = golden[name]
    for i in (0, s["n"] // 2, s["n"] - 1):
        if name in ref.FOURVIEW_SETS:
            e = ref.fourview2d_minimal(s["x"], s["samples"][i], s["frames"])
            assert e["count"] == s["count"][i] and bool(e["decided"]) == bool(s["decided"][i])
            assert [float("%.4g" % k) for k in e["K"]] == s["K"][i].tolist()
            if e["count"]:
                want = np.array([[_f(P) for P in c] for c in e["cams"]])
                assert np.array_equal(want, s["cams"][i]), (name, i)
        elif name in ref.POSE2D_SETS:
            e = ref.pose2d(s["x"], s["X"], s["samples"][i])
            assert np.array_equal(_f(e["pose"]), s["pose"][i]) and float("%.4g" % e["K"]) == s["K"][i] and bool(e["decided"]) == bool(s["decided"][i])
        elif name in ref.PLANAR_SETS:
            e = ref.planar_offsets(s["scene"], s["samples"][i])
            assert np.array_equal(np.array([float(v) for v in e["offsets"]]), s["offsets"][i]) and float("%.4g" % e["K"]) == s["K"][i]
            assert [float("%.4g" % e["cond_final"]), float("%.4g" % e["cond_track"])] == s["cond"][i].tolist()
        else:
            e = ref.fourview2d_track(s["cams"], s["x"], i)
            assert [float(v) for v in e["X"]] == s["X"][i].tolist() and float(e["err"]) == s["err"][i] and float("%.4g" % e["K"]) == s["K"][i]
            stored, scale, _ = ref.fourview2d_errors_at(s["cams"], s["x"], s["X"][i], i)
            assert float(stored) == s["err_stored"][i] and float("%.4g" % scale) == s["scale"][i]


def test_reference_satisfies_its_defining_equations(golden):
    """at 1e-40: every null vector is an eigenvector of its Gram matrix (for a minimal sample: A v = 0), cameras 2 and 3 of a minimal sample are calibrated,
    the four candidates that share a root and flip1 have one fourth camera (all inside `residual`); the offsets satisfy their (normal) equations"""
    a, b, d = golden["fourview_a"], golden["fourview_b"], golden["fourview_d"]
    full = int(np.argmax(d["count"] == 16))
    for s, i in ((a, 0), (a, 17), (b, 3), (d, full), (golden["fourview_c"], 5)):
        e = ref.fourview2d_minimal(s["x"], s["samples"][i], s["frames"])
        assert e["count"] == 16 and e["residual"] < TINY, (s["name"], i, e["residual"])
        for root in range(2):                           # and directly: rotation blocks, unit baseline
            P2, P3 = e["pre"][root]
            for P in (P2, P3):
                assert abs(P[0][0] ** 2 + P[1][0] ** 2 - 1) < TINY
                if s["samples"].shape[1] == 5:
                    assert abs(P[0][0] - P[1][1]) < TINY and abs(P[0][1] + P[1][0]) < TINY
            assert abs(P2[0][2] ** 2 + P2[1][2] ** 2 - 1) < TINY
    # a minimal sample's incidences hold in all sixteen candidates' first three cameras: the triangulated sample points project onto the bearings
    e = ref.fourview2d_minimal(a["x"], a["samples"][0], a["frames"])
    for c in e["cams"]:
        for t in a["samples"][0]:
            xs = [[mp.mpf(float(a["x"][j, t, 0])), mp.mpf(float(a["x"][j, t, 1]))] for j in range(4)]
            X, _ = ref.triangulate3(c[:3], xs[:3])
            for j in range(3):
                z0, z1 = c[j][0][0] * X[0] + c[j][0][1] * X[1] + c[j][0][2], c[j][1][0] * X[0] + c[j][1][1] * X[1] + c[j][1][2]
                assert abs(z0 * xs[j][1] - z1 * xs[j][0]) < TINY * 1000, (j, t)
    for name in ref.POSE2D_SETS[::2]:
        s = golden[name]
        assert ref.pose2d(s["x"], s["X"], s["samples"][1])["residual"] < TINY
    for name in ref.PLANAR_SETS:
        s = golden[name]
        assert ref.planar_offsets(s["scene"], s["samples"][2])["residual"] < TINY
