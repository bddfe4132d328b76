"""The exact reference of re3q3 and P6L (tests/p6l_reference.py) and its golden file, checked on the CPU: the file holds the sets it is meant to hold, the
reference run again reproduces it, the oracle (oracle/absolute_pose.h: the same elimination as the kernel, companion-matrix QR for the roots) returns
exactly the exact number of real roots on EVERY decided system and each of its roots or poses matches a distinct exact one within the recorded
oracle_rho / oracle_pose_rho - the yardstick the device is held to in tests/test_gpu_p6l_exact.py."""
import numpy as np
import pytest

import p6l_reference as ref

SETS = ref.QUADRIC_SETS + ref.P6L_SETS
ALL_SETS = SETS + (ref.SPECIAL_SET,)


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


def test_golden_sets_are_the_ones_described(golden):
    assert set(golden) == set(ALL_SETS)
    assert [e["decided"] for e in golden[ref.SPECIAL_SET]["systems"]] == [True, True, False, False]
    for name in SETS:
        assert 64 <= len(golden[name]["systems"]) <= 128, name
    elim = golden["quadrics_elim"]["systems"]
    for e in (0, 1, 2):
        assert sum(1 for s in elim if s["elim"] == e and not s["near_tie"]) >= 8
        assert sum(1 for s in elim if s["elim"] == e and s["near_tie"]) >= 4
    deg = golden["quadrics_degenerate"]["systems"]
    assert sorted({s["kind"] for s in deg}) == [0, 1, 2, 3, 4] and all(sum(1 for s in deg if s["kind"] == k) == 16 for k in range(4))
    scaled = golden["quadrics_scaled"]["systems"]
    assert sum(1 for s in scaled if np.abs(s["c"]).max() < 1e-59) == 1
    lines = golden["p6l_degenerate_lines"]["systems"]
    assert {tuple(s["groups"]) for s in lines if "groups" in s} == {(0,), (1,), (0, 1)} and sum(1 for s in lines if "groups" in s) == 40
    assert {int(s["aligned"].sum()) for s in lines} == {0, 1, 2, 3, 4, 5, 6}
    for s in lines:                                   # lines through one image point: the determinant the kernel tests is below its 1e-10
        for g in s.get("groups", ()):
            assert abs(np.linalg.det(s["lines"][3 * g: 3 * g + 3])) < 1e-14
    # both outcomes: systems with no real root, with many; roots at infinity are the exception, not the rule
    counts = [e["num_real"] for e in golden["quadrics_random"]["systems"]]
    assert min(counts) == 0 and max(counts) >= 6 and all(n % 2 == 0 for n in counts)


def test_undecided_shares_respect_the_cap(golden):
    """2 % at most, from the separations in the file; the near-tie half of quadrics_elim is not capped"""
    for name in SETS:
        systems = [e for e in golden[name]["systems"] if not e.get("near_tie", False)]
        share = float(np.mean([not e["decided"] for e in systems]))
        assert abs(golden[name]["undecided_share"] - share) < 1e-12, name
        assert share <= 0.02, (name, share)


def test_cube_has_its_eight_exact_roots(golden):
    cube = next(e for e in golden["quadrics_degenerate"]["systems"] if e["kind"] == 4)
    assert cube["num_real"] == 8 and cube["num_finite"] == 8 and cube["decided"]
    assert sorted(map(tuple, cube["real"].tolist())) == sorted((float(a), float(b), float(d)) for a in (-1, 1) for b in (-1, 1) for d in (-1, 1))
    res = ref.solve_quadrics(cube["c"])               # and again from the inputs: x alone does not separate the roots, the separator is another
    assert res["separator"] != (0, 0) and res["num_real"] == 8
    assert all(abs(abs(v) - 1) < ref.mp.mpf(10) ** -55 for s in res["roots"] for v in s)


def test_scaled_systems_have_their_parents_roots_bit_for_bit(golden):
    """rows scaled by powers of two: the same rational system up to units, so the same roots to the last bit in the reference.  The file holds a scaled
    system as its parent's index and three exponents (the generator asserts the identity for all 64); two of them are solved again here."""
    parents, scaled = golden["quadrics_random"]["systems"], golden["quadrics_scaled"]["systems"]
    assert sorted({tuple(e["exp"]) for e in scaled[:63]}) == sorted((a, b, d) for a in (-40, 40) for b in (-40, 40) for d in (-40, 40)) and scaled[63]["exp"] == [-200] * 3
    for e in scaled:
        assert np.array_equal(e["c"], parents[e["parent"]]["c"] * (2.0 ** np.array(e["exp"], dtype=np.float64))[:, None])
    for i in (next(i for i, e in enumerate(scaled) if len(set(e["exp"])) > 1 and e["num_real"]), 63):
        j = ref.system_json(ref.solve_quadrics(scaled[i]["c"]))
        p = parents[scaled[i]["parent"]]
        assert j["num_real"] == p["num_real"] and j["num_finite"] == p["num_finite"] and j["sep"] == p["sep"]
        assert np.array(j["real"]).reshape(-1, 3).tobytes() == p["real"].tobytes()
        assert np.array_equal(scaled[i]["kappa"], p["kappa"])          # the parent's: the conditioning of a root does not depend on a row's scale


@pytest.mark.parametrize("name", SETS)
def test_reference_reproduces_the_golden_file(golden, name):
    """a sample of each set, solved again"""
    systems = golden[name]["systems"]
    for i in (0, len(systems) - 1) if name in ref.QUADRIC_SETS else (len(systems) // 2,):
        e = systems[i]
        res = ref.solve_quadrics(e["c"]) if "c" in e else ref.solve_p6l(e["lines"], e["points"])
        j = ref.system_json(res)
        assert j["num_real"] == e["num_real"] and j["num_finite"] == e["num_finite"] and res["sturm"] == e["num_real"]
        assert np.array_equal(np.array(j["real"]).reshape(-1, 3), e["real"])
        assert j["sep"] == e["sep"] and ("parent" in e or np.array_equal(np.array(j["kappa"]), e["kappa"]))
        if "poses" in e:                              # the poses evaluated from the file's rounded roots against the 60-digit ones
            want = np.array([[float(v.real) for v in P] for P in res["poses"][: res["num_real"]]]).reshape(-1, 3, 4)
            assert np.abs(e["poses"] - want).max() <= 2.0 ** -50 * max(1.0, np.abs(want).max())


def test_reference_roots_solve_the_system():
    """the residual of every root in 60-digit arithmetic, on a system with roots at infinity too (no x^2 term anywhere: seven finite roots at most)"""
    rng = np.random.default_rng(5)
    c = rng.uniform(-1, 1, (3, 10))
    for drop in (False, True):
        if drop:
            c[:, 0] = 0.0
        res = ref.solve_quadrics(c)
        assert res["num_finite"] < 8 if drop else res["num_finite"] == 8
        for s in res["roots"]:
            m = ref.monomials(s)
            assert max(abs(sum(ref.mp.mpf(float(c[r, j])) * m[j] for j in range(10))) for r in range(3)) < ref.mp.mpf(10) ** -45


def test_p6l_clean_holds_the_ground_truth(golden):
    """every pose of the file is a rotation and satisfies its six incidences; solve_p6l on a six-tuple of a known pose returns that pose"""
    from privacy_preserving_sfm_amd import synthetic
    for name in ref.P6L_SETS:
        for e in golden[name]["systems"]:
            for P in e["poses"]:
                R = P[:, :3]
                assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and np.linalg.det(R) > 0
                Xc = e["points"] @ R.T + P[:, 3]
                assert np.abs(np.sum(e["lines"] * Xc, axis=1)).max() < 1e-13 * max(1.0, np.abs(Xc).max()) * max(1.0, np.abs(e["lines"]).max())
    sc = synthetic.make_ransac_scene(6, outlier_ratio=0.0, noise_px=0.0, seed=77)
    res = ref.solve_p6l(sc["lines"], sc["points"])
    assert min(np.abs(np.array([float(v.real) for v in P]).reshape(3, 4) - sc["gt_pose"]).max() for P in res["poses"][: res["num_real"]]) < 1e-12


@pytest.mark.parametrize("name", ALL_SETS)
def test_oracle_matches_reference_root_by_root(oracle, golden, name):
    """the oracle returns the exact number of real roots on every decided system, matches them one to one, and its error, system by system (the
    largest over the system and 32 copies moved by one unit in the last place), is what the file says: the device's bound is made of these"""
    s = golden[name]
    seen = []
    for i, e in enumerate(s["systems"]):
        if not e["decided"]:
            continue
        if "aligned" in e and e["aligned"].all():
            assert len(oracle.p6l(e["lines"], e["points"], e["aligned"])) == 0, (name, i)
            continue
        m = ref.oracle_error(oracle, name, i, e)
        assert m is not None, (name, i, "count or one-to-one match")
        assert m[0] <= e["oracle_rho"], (name, i, m[0], e["oracle_rho"])
        if e["num_real"]:
            seen.append(e["oracle_rho"])
    seen.sort()
    print("%s: oracle rho median %.4g, floor %.4g, max %.4g" % (name, seen[len(seen) // 2], s["oracle_floor"], seen[-1]))
    assert seen[-1] == s["oracle_max"]
    if name != ref.SPECIAL_SET:
        assert s["oracle_floor"] == seen[int(0.9 * len(seen))]
    else:
        assert s["oracle_floor"] == golden["quadrics_random"]["oracle_floor"]


def test_undecided_systems_hold_their_complex_roots(golden):
    """the two undecided systems of quadrics_special: eight real roots in close pairs, all held by the file"""
    for e, d in zip(golden[ref.SPECIAL_SET]["systems"][2:], (2.0 ** -12, 2.0 ** -16)):
        assert e["num_real"] == 8 and e["num_finite"] == 8 and e["roots"].shape == (8, 3) and not e["decided"]
        x = np.sort(e["real"][:, 0])
        assert np.allclose(x[:4], 0.5, atol=1e-15) and np.allclose(x[4:], 0.5 + d, atol=1e-15) and e["sep"] < d
