// Host replay of IncrementalTriangulator::TriangulateImage / CompleteImage (reference src/sfm/incremental_triangulator.cc:63-235 with Find :426-466,
// Continue :563-604, Create :468-561) over the device's speculative results - std only, no HIP.  The device answers every line of the image on
// the state at the start of the call (ImageLineResult); the host visits the lines in ascending order and applies the answers.  An answer holds
// only while no line it read - the reference line and its filtered closure - has changed line_point since the snapshot (`changed`); otherwise
// the line is evaluated afresh on the current state.  tracks_image.hip drives it.
#pragma once
#include <cstdint>
#include <vector>

#include "tracks_replay.hpp"

namespace ppsfm {

// what the device answers for one reference line on one state
struct ImageLineResult {
  std::vector<int32_t> list;       // FindTransitiveCorrespondences in the reference's order, minus unregistered images and skipped cameras
  int32_t num_triangulated = 0;    // entries of `list` with a point
  int32_t continue_point = -1;     // Continue: the point the reference line joins, -1 none
  std::vector<int32_t> set;        // the observations EstimateTriangulation sees: the free entries of `list`, then the reference line if it is free
  uint64_t min_trials = 0;         // min_num_trials of the (first) RANSAC over `set`
  std::vector<int32_t> round_of;   // per element of `set`: k > 0 = inlier of the k-th point created from it, 0 = of none
  std::vector<double> xyz;         // 3 per created point
  int64_t trials = 0;
};

inline uint64_t NChooseK(uint64_t n, uint64_t k) {
  if (k > n) return 0;
  uint64_t r = 1;
  for (uint64_t i = 1; i <= k; ++i) r = r * (n - k + i) / i;
  return r;
}
constexpr uint64_t kExhaustiveSamplingThreshold = 15;
// Create builds its options afresh per call (:517-531): exhaustive sampling for short sets, else the default 0
inline uint64_t CreateMinTrials(uint64_t n) { return n <= kExhaustiveSamplingThreshold ? NChooseK(n, 3) : 0; }
// CompleteImage keeps ONE options object over its loop (:142-149, :205-209): a long set runs with the value the last short one left behind
inline uint64_t CompleteMinTrials(uint64_t n, uint64_t carried) { return n <= kExhaustiveSamplingThreshold ? NChooseK(n, 2) : carried; }

// CorrespondenceGraph::IsTwoViewObservation (base/correspondence_graph.cc:252-263)
inline bool IsTwoViewObservation(const TrackState& st, int32_t l) {
  if (st.corr_start[(size_t)l + 1] - st.corr_start[(size_t)l] != 1) return false;
  const int32_t o = st.corr_line[(size_t)st.corr_start[(size_t)l]];
  return st.corr_start[(size_t)o + 1] - st.corr_start[(size_t)o] == 1;
}

struct ImageCounters {
  int64_t num_tris = 0, trials = 0;
  int32_t points_created = 0, lines_continued = 0, lines_redone = 0;
  int error = 0;      // 1: an answer claims a line that is not free (the device and the host disagree about the state)
};

struct ImageReplayState {
  TrackState& st;
  std::vector<uint8_t> changed;      // per line: line_point changed in this call
  std::vector<uint8_t> touched;      // per point: track changed (or created) in this call
  ImageCounters cnt;
  explicit ImageReplayState(TrackState& s) : st(s), changed((size_t)s.L, 0), touched((size_t)s.NumPoints(), 0) {}

  bool Holds(int32_t ref, const ImageLineResult& r) const {
    if (changed[(size_t)ref]) return false;
    for (const int32_t l : r.list) if (changed[(size_t)l]) return false;
    return true;
  }
  template <typename EmitFn>
  void AddObservation(int p, int32_t l, EmitFn& emit) {      // Reconstruction::AddObservation
    if (st.line_point[(size_t)l] != -1) { cnt.error = 1; return; }
    st.line_point[(size_t)l] = p;
    st.tracks[(size_t)p].push_back(l);
    changed[(size_t)l] = 1; touched[(size_t)p] = 1;
    emit(p, l);
    ++cnt.num_tris;
  }
  // Reconstruction::AddPoint3D for every point the RANSACs over r.set created, in order; the new points take the next unused indices
  template <typename EmitFn>
  void AddPoints(const ImageLineResult& r, EmitFn& emit) {
    cnt.trials += r.trials;
    const int rounds = (int)(r.xyz.size() / 3);
    for (int k = 1; k <= rounds; ++k) {
      const int m = st.NumPoints();
      st.points.insert(st.points.end(), r.xyz.begin() + 3 * (k - 1), r.xyz.begin() + 3 * k);
      st.tracks.emplace_back();
      st.deleted.push_back(0);
      touched.push_back(1);
      ++cnt.points_created;
      for (size_t i = 0; i < r.set.size(); ++i)
        if (r.round_of[i] == k) AddObservation(m, r.set[i], emit);
    }
  }
};

// TriangulateImage over `lines` (the lines of the image, ascending).  spec(i) -> const ImageLineResult& of lines[i] on the snapshot;
// fresh(line) -> const ImageLineResult* on the current state (nullptr: failed); emit(point, line) per observation in the reference's order.
template <typename SpecFn, typename FreshFn, typename EmitFn>
inline ImageCounters ReplayTriangulateImage(TrackState& st, const std::vector<int32_t>& lines, SpecFn&& spec, FreshFn&& fresh, EmitFn&& emit) {
  ImageReplayState rs(st);
  for (size_t i = 0; i < lines.size() && !rs.cnt.error; ++i) {
    const int32_t ref = lines[i];
    const ImageLineResult* r = &spec(i);
    if (!rs.Holds(ref, *r)) {
      ++rs.cnt.lines_redone;
      r = fresh(ref);
      if (!r) { rs.cnt.error = 2; break; }
    }
    if (r->list.empty()) continue;                                   // :98
    if (r->continue_point >= 0) { rs.AddObservation(r->continue_point, ref, emit); ++rs.cnt.lines_continued; }
    rs.AddPoints(*r, emit);                                          // Create and its recursion
  }
  return rs.cnt;
}

// CompleteImage.  `lines`: the lines of the image, ascending; has_spec(i) / spec(i): the snapshot's answer for a line that was free and passed the
// two-view rule then; fresh(line, carried_min_trials) as above; complete_spec(p) -> SpecList of a point that had a line of the image at the
// snapshot; fresh_complete(p, &list) -> 0 / error: K10a for p on the current state.
template <typename HasFn, typename SpecFn, typename FreshFn, typename CSpecFn, typename CFreshFn, typename EmitFn>
inline ImageCounters ReplayCompleteImage(TrackState& st, const std::vector<int32_t>& lines, bool ignore_two_view_tracks, int complete_max_transitivity,
                                         HasFn&& has_spec, SpecFn&& spec, FreshFn&& fresh, CSpecFn&& complete_spec, CFreshFn&& fresh_complete, EmitFn&& emit) {
  ImageReplayState rs(st);
  const int P0 = st.NumPoints();
  uint64_t carried = 0;
  auto claim = [&](int p, int32_t l) { rs.AddObservation(p, l, emit); };
  std::vector<int32_t> list;
  for (size_t i = 0; i < lines.size() && !rs.cnt.error; ++i) {
    const int32_t ref = lines[i];
    const int p = st.line_point[(size_t)ref];
    if (p >= 0) {                                                    // Complete(point) (:165-169)
      if (p < P0 && !rs.touched[(size_t)p]) {
        ReplayCompletePoint(st, p, complete_spec(p), complete_max_transitivity, claim);
      } else {                                                       // a new point, or a track that grew since the snapshot: the device's list is not its closure
        ++rs.cnt.lines_redone;
        if (fresh_complete(p, &list)) { rs.cnt.error = 2; break; }
        for (const int32_t l : list) claim(p, l);
      }
      continue;
    }
    if (ignore_two_view_tracks && IsTwoViewObservation(st, ref)) continue;
    const ImageLineResult* r = has_spec(i) ? &spec(i) : nullptr;
    // the answer also depends on the min_num_trials the loop carries: known only once the lines before this one are settled
    if (r && rs.Holds(ref, *r) && (r->num_triangulated || r->list.empty() || r->min_trials == CompleteMinTrials(r->set.size(), carried))) {
    } else {
      ++rs.cnt.lines_redone;
      r = fresh(ref, carried);
      if (!r) { rs.cnt.error = 2; break; }
    }
    if (r->num_triangulated || r->list.empty()) continue;            // :179
    carried = CompleteMinTrials(r->set.size(), carried);
    rs.AddPoints(*r, emit);
  }
  return rs.cnt;
}

}  // namespace ppsfm
