"""IterativeGlobalRefinement (reference src/controllers/incremental_mapper.cc:102-124) on the device against the same loop run with the oracle
(tests/refinement_oracle.py), on noisy cfg-1 and cfg-2 scenes: 0.5 px line noise, 5 % outlier observations, float32-stored lines.

Asserted: the same number of rounds; per round the identical sets of deleted observations and deleted points and the same `changed`; final
parameters within 1e-5 relative after Normalize; at least 90 % of the planted outliers removed by the end; and - so that a tie cannot hide -
that no observation's pixel error lies within 1e-6 relative of the 4 px threshold in the oracle's run.

Seeds: chosen on the CPU so that the ORACLE's own loop is reproducible (its input points perturbed by 1e-12 relative, three perturbations: the
same deleted sets, final parameters within 1e-6) - round 1's solve runs the global preset's 50 iterations under the TRIVIAL loss with the outliers
(338 px rms) still in and stops unconverged, at a point that on many seeds depends on rounding.  Measured with the oracle loop:
  20 images, seed 0x260: two rounds, 1796 of 2000 observations filtered in round 1 (a point with one observation over 4 px loses its whole
  4-track), 96 % of the planted outliers removed, smallest threshold margin 2.2e-3, movement under the perturbation 3.1e-9.
  100 images, seed 0x2c0: three rounds, 36243 / 3 / 0 filtered, 99.6 % removed, margin 2.2e-5, movement 3.7e-10.
The oracle alone removes more than 90 %, so the bound stays at 90 %.
In those two cases round 1 deletes nine observations in ten, inliers included: with 5 % gross outliers under the TRIVIAL loss the solve is wrecked, so the
90 % says little about selectivity.  A third case, beside the issue's, has 0.2 % outliers (100 images, seed 0x320; oracle loop: 34 iterations to
CONVERGENCE, 2645 of 40000 filtered, every planted outlier among them, movement under the perturbation 5.6e-13, margin 2.2e-5): there the inliers
survive, which the test asserts (at least 90 % of them).

"1e-5 relative" is the project's array-norm bound (tests/test_gpu_baseline_sizes.py `_rel`): |a - b| of every parameter over the largest magnitude of its
array - the poses (quaternions and translations together, largest entry about 4) and the points (about 1) - so a small parameter is held to about
1e-5 absolute, not to 1e-5 of itself.
"""
import time

import numpy as np
import pytest

import refinement_oracle
from privacy_preserving_sfm_amd import synthetic

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("cams,points,track,seed,outlier_obs", [(20, 500, 4, 0x260, 0.05), (100, 5000, 8, 0x2C0, 0.05), (100, 5000, 8, 0x320, 0.002)])
def test_iterative_global_refinement_matches_the_oracle_loop(oracle, cams, points, track, seed, outlier_obs):
    from privacy_preserving_sfm_amd.bundle_adjustment import IncrementalMapperOptions, IterativeGlobalRefinement, Reconstruction
    sc = synthetic.make_ba_scene(cams, points, track, seed=seed, model=2, **dict(refinement_oracle.NOISY, outlier_obs=outlier_obs))
    options = IncrementalMapperOptions()
    options.print_summary = False
    ref_rec = Reconstruction.from_scene(sc)
    ref = refinement_oracle.iterative_global_refinement(ref_rec, options)
    assert ref["margin"] > 1e-6, ref["margin"]                                   # no observation sits on the 4 px threshold in the oracle's run
    rec = Reconstruction.from_scene(sc)
    t0 = time.time()
    rep = IterativeGlobalRefinement(rec, options)
    wall = time.time() - t0
    print("%d images: %d rounds in %.2f s; filtered %s, changed %s, iterations %s (oracle %s)" % (
        cams, rep.num_rounds, wall, rep.num_filtered, rep.changed, [s.num_iterations for s in rep.summaries], [s.num_iterations for s in ref["summaries"]]))
    assert rep.num_rounds == ref["num_rounds"]
    for k in range(rep.num_rounds):
        assert rep.obs_deleted[k] == ref["obs_deleted"][k], k
        assert rep.point_deleted[k] == ref["point_deleted"][k], k
        assert rep.num_filtered[k] == ref["num_filtered"][k] and rep.changed[k] == ref["changed"][k], k
    poses, pts, ids = refinement_oracle.parameters(rec)
    rposes, rpts, rids = refinement_oracle.parameters(ref_rec)
    assert ids == rids
    assert _rel(poses, rposes) <= 1e-5 and _rel(pts, rpts) <= 1e-5
    # the planted outliers are gone
    count, planted = {}, set()
    for o, c in enumerate(sc["obs_pose"]):
        k = count.get(int(c), 0)
        count[int(c)] = k + 1
        if sc["outlier_mask"][o]:
            planted.add((int(c), k))
    left = refinement_oracle.observations(rec)
    removed = 1.0 - len(planted & left) / float(len(planted))
    print("%d images: %.1f %% of the %d planted outliers removed, %d observations left" % (cams, 100 * removed, len(planted), len(left)))
    assert removed >= 0.9
    if outlier_obs < 0.05:      # the selective case: the filter takes the outliers and leaves the inliers
        assert len(left - planted) >= 0.9 * (len(sc["obs_pose"]) - len(planted))
