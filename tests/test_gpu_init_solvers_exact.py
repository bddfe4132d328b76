"""K6's solvers - k_fourview2d_minimal<1> and <16>, k_pose2d_solve, k_planar_solve, k_fourview2d_evaluate, k_fourview2d_errors_stored - held sample by
sample to the 50-digit reference (tests/init_solvers_reference.py, tests/golden/init_solvers_golden.json).

On every DECIDED sample (no branch of the function within 1e-6 of its threshold, 2^-52 K <= 1e-3: see the reference module) the count is the reference's, the
sixteen candidates equal the reference's IN ORDER - root (0, 1) x flip1, flip2, flip3, up to the exchange k <-> k ^ 1 of all eight candidates of a root that
the sign of the third camera's null vector decides - and each is within 4 * max(oracle_rho of the SAMPLE, oracle_floor of the set) in the normalised measure
rho = max|got - want| / (max(1, max|want|) 2^-52 K).  K comes from the reference alone; oracle_rho is the error the CPU oracle (the same Gram matrix and
cyclic Jacobi in double) made on that sample and on 32 copies of it moved by one unit in the last place, oracle_floor the nine-tenths quantile of those over
the set.  No share of samples is left out.  tests/test_init_solvers_reference.py shows on the CPU that the oracle passes the same comparison and that an
exchanged pair of flips, exchanged roots or a candidate 1e-6 off fail it.

Largest rho / bound on the MI355X (printed by each test):
  fourview_a 0.243   fourview_b 0.149   fourview_c 0.196   fourview_d 0.140   fourview_e 0.195
  pose2d exact m = 3, 6, 21: 0.131, 0.170, 0.199   noise: 0.182, 0.190, 0.182
  planar exact m = 3, 10: 0.113, 0.128             noise: 0.137, 0.143
  track 0.833 (the device's 2x2 normal equations against the oracle's QR); errors at stored points 0.40 of 2^-52 scale (bound 16)
With the normal equations k_planar_solve had for more than three tracks, planar_exact_m10 and planar_noise_m10 FAILED this comparison (first sample over
the bound: rho 0.302 against 0.298, and 0.245 against 0.242; a double-precision restatement of that arithmetic on the CPU reaches 10 and 2.6 times the
bound): the offsets of a ten-track sample were further from the exact least-squares solution than four times the oracle's QR ever is.  The kernel now
rotates each equation into a triangular factor (Givens), and holds the bound with the margin above."""
import numpy as np
import pytest

import init_solvers_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


def _minimal(s, samples, chunk):
    """the minimal solver on `samples` in calls of `chunk` samples: more than 16 in a call run k_fourview2d_minimal<1> (a lane per sample), up to 16
    k_fourview2d_minimal<16> (a lane per candidate)"""
    from privacy_preserving_sfm_amd.device import FourView2dProblem
    fv = FourView2dProblem(s["x"])
    cams, cnt = [], []
    for at in range(0, len(samples), chunk):
        c, n = fv.minimal_batch(samples[at: at + chunk], frames=s["frames"])
        cams.append(c); cnt.append(n)
    fv.close()
    return np.concatenate(cams), np.concatenate(cnt)


def test_default_frames_are_the_files(golden):
    from privacy_preserving_sfm_amd.device import fourview2d_default_frames
    assert fourview2d_default_frames().tobytes() == golden["_meta"]["default_frames"].tobytes()
    assert golden["fourview_a"]["frames"].tobytes() == golden["_meta"]["default_frames"].tobytes()


@pytest.mark.parametrize("name", ref.FOURVIEW_SETS)
def test_fourview_minimal_equals_reference_candidate_by_candidate(golden, name):
    s = golden[name]
    n = s["n"]
    # one call of all samples on the lane-per-sample kernel (the sixteen samples of the hard set twice over, to be more than 16), calls of 16, calls of 1
    whole = s["samples"] if n > 16 else np.concatenate([s["samples"], s["samples"]])
    cams, cnt = _minimal(s, whole, len(whole))
    assert len(whole) > 16 and cams[:n].tobytes() == cams[len(whole) - n:].tobytes()
    cams, cnt = cams[:n], cnt[:n]
    for chunk in (16, 1):
        c, k = _minimal(s, s["samples"], chunk)
        assert np.array_equal(k, cnt) and c.tobytes() == cams.tobytes(), (name, chunk)
    worst = ref.check_fourview_decided(s, cams, cnt)
    print("%s: max rho / bound = %.3g (bound: %g x max(the sample's oracle rho, %.4g))" % (name, worst, ref.FACTOR, s["oracle_floor"]))
    # every sample, decided or not
    assert set(cnt.tolist()) <= {0, 16}
    for i in range(n):
        if cnt[i] != 16:
            assert np.isnan(cams[i]).all(), (name, i)
            continue
        assert np.isfinite(cams[i]).all(), (name, i)
        assert np.array_equal(cams[i, :, 0], np.tile([[1.0, 0, 0], [0, 1.0, 0]], (16, 1, 1)))
        for k in range(16):
            for v in (1, 2):
                R = cams[i, k, v, :, :2]
                assert np.abs(R.T @ R - np.eye(2)).max() <= 64 * ref.EPS * s["K"][i, k >> 3], (name, i, k, v)
            assert abs(np.linalg.norm(cams[i, k, 1, :, 2]) - 1.0) <= 1e-12, (name, i, k)
            a, b = cams[i, k, 3, 0, 0], cams[i, k, 3, 1, 0]                # the fourth camera is [a -b; b a], a^2 + b^2 = 1, by construction
            assert cams[i, k, 3, 1, 1] == a and cams[i, k, 3, 0, 1] == -b and abs(a * a + b * b - 1.0) <= 1e-12


@pytest.mark.parametrize("name", ref.POSE2D_SETS)
def test_pose2d_equals_reference(golden, name):
    from privacy_preserving_sfm_amd.device import Pose2dProblem
    s = golden[name]
    pp = Pose2dProblem(s["x"], s["X"])
    poses = pp.solve_batch(s["samples"])
    one = np.concatenate([pp.solve_batch(s["samples"][i: i + 1]) for i in range(3)])
    pp.close()
    assert one.tobytes() == poses[:3].tobytes()
    worst = ref.check_rows_decided(s, poses, "pose")
    print("%s: max rho / bound = %.3g (bound: %g x max(the sample's oracle rho, %.4g))" % (name, worst, ref.FACTOR, s["oracle_floor"]))
    assert np.isfinite(poses).all() and np.abs(poses[:, 0, 0] ** 2 + poses[:, 1, 0] ** 2 - 1.0).max() <= 1e-12
    assert np.array_equal(poses[:, 0, 0], poses[:, 1, 1]) and np.array_equal(poses[:, 0, 1], -poses[:, 1, 0])
    first = s["X"][s["samples"][:, 0]]                                       # the first sample point in front
    assert (poses[:, 1, 0] * first[:, 0] + poses[:, 1, 1] * first[:, 1] + poses[:, 1, 2] >= 0).all()


@pytest.mark.parametrize("name", ref.PLANAR_SETS)
def test_planar_offsets_equal_reference(golden, name):
    from privacy_preserving_sfm_amd.device import PlanarOffsetProblem
    s = golden[name]
    pp = PlanarOffsetProblem(s["scene"]["poses"], s["scene"]["lines"], s["scene"]["Rg"])
    off = pp.solve_batch(s["samples"])
    one = np.concatenate([pp.solve_batch(s["samples"][i: i + 1]) for i in range(3)])
    pp.close()
    assert one.tobytes() == off[:3].tobytes() and np.isfinite(off).all()
    worst = ref.check_rows_decided(s, off, "offsets")
    print("%s: max rho / bound = %.3g (bound: %g x max(the sample's oracle rho, %.4g))" % (name, worst, ref.FACTOR, s["oracle_floor"]))


def test_track_points_and_errors_equal_reference(golden):
    """k_fourview2d_evaluate: the three-view point and the error of every track of one set-b model, K the condition of the track's 2x2 normal matrix;
    k_fourview2d_errors_stored at the reference's points (rounded to double): the error is a difference of ratios, each rounded at its own size, and is
    held to 16 * 2^-52 of `scale` = |x_a / x_b| + (|P_0| |X~| + |z_0 / z_1| |P_1| |X~|) / |z_1|, the size of the terms it is rounded in, worst view"""
    from privacy_preserving_sfm_amd.device import FourView2dProblem
    s = golden[ref.TRACK_SET]
    fv = FourView2dProblem(s["x"])
    err, X = fv.evaluate(s["cams"])
    stored = fv.evaluate_points(s["cams"], s["X"])
    fv.close()
    worst = ref.check_track_decided(s, X, err)
    print("track: max rho / bound = %.3g (bound: %g x max(the track's oracle rho, %.4g))" % (worst, ref.FACTOR, s["oracle_floor"]))
    assert s["decided"].all() and (s["err"] < 1e3).all()                      # every track in front of the four views
    d = np.abs(stored - s["err_stored"]) / (ref.EPS * s["scale"])
    print("track: errors at stored points, max |got - want| / (2^-52 scale) = %.3g (bound 16)" % d.max())
    assert d.max() <= 16.0, (int(np.argmax(d)), d.max())
