"""The global refinement loop WITH CompleteAndMergeTracks, the CPU oracles doing the arithmetic - TEST INFRASTRUCTURE: tests/refinement_oracle.py's
bundle adjustment and filter around tests/tracks_reference.py's Complete / Merge, composed as the reference's loop is
(src/controllers/incremental_mapper.cc:102-124, 160-172).  The device never runs here."""
import numpy as np

import refinement_oracle as ro
import tracks_reference as tr
from privacy_preserving_sfm_amd.bundle_adjustment import GlobalBundleAdjustmentOptions, IncrementalMapperOptions


def complete_and_merge(oracle, tri_options):
    c0, m0 = len(oracle.completed), len(oracle.merged)
    nc = oracle.CompleteAllTracks(tri_options)
    nm = oracle.MergeAllTracks(tri_options)
    return nc, nm, oracle.completed[c0:], oracle.merged[m0:]


def iterative_global_refinement(rec, graph, mapper_options=None, tri_options=None):
    """-> dict(num_rounds, initial, num_completed, num_merged, completed, merged, num_filtered, changed, obs_deleted, point_deleted (per round),
    margin = the smallest threshold margin (completion, merge, filter) over everything the loop tested)"""
    options = mapper_options or IncrementalMapperOptions()
    tri_options = tri_options or tr.Options()
    oracle = tr.TracksOracle(graph, rec)
    rep = dict(num_rounds=0, num_completed=[], num_merged=[], completed=[], merged=[], num_filtered=[], changed=[], obs_deleted=[], point_deleted=[],
               margin=np.inf)
    rep["initial"] = complete_and_merge(oracle, tri_options)
    for _ in range(options.ba_global_max_refinements):
        num_observations = rec.ComputeNumObservations()
        ro.adjust_global_bundle(rec, GlobalBundleAdjustmentOptions(len(rec.RegImageIds()), options))
        nc, nm, completed, merged = complete_and_merge(oracle, tri_options)
        obs_before, points_before = ro.observations(rec), set(rec.points3D)
        nf, fmargin = ro.filter_all_points(rec, options.filter_max_reproj_error, options.filter_min_tri_angle)
        changed = float(nc + nm + nf) / num_observations
        rep["num_rounds"] += 1
        rep["num_completed"].append(nc); rep["num_merged"].append(nm); rep["completed"].append(completed); rep["merged"].append(merged)
        rep["num_filtered"].append(nf); rep["changed"].append(changed)
        rep["obs_deleted"].append(sorted(obs_before - ro.observations(rec)))
        rep["point_deleted"].append(sorted(points_before - set(rec.points3D)))
        # the filter's margin is on the unsquared error, the oracle's on the squared one: |e^2 - t^2| / t^2 >= |e - t| / t, so the minimum is a lower bound
        rep["margin"] = min(rep["margin"], fmargin, oracle.margin)
        if changed < options.ba_global_max_refinement_change:
            break
    return rep


def decisions(rep):
    return (rep["num_rounds"], rep["initial"], rep["completed"], rep["merged"], rep["obs_deleted"], rep["point_deleted"])
