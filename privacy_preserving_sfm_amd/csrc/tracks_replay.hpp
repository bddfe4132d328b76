// Host replay of IncrementalTriangulator::Complete / Merge (reference src/sfm/incremental_triangulator.cc:606-765) over the device's
// speculative results - std only, no HIP: the sequential decisions (which line is still free, which pair was tried, the recursion into a
// merged point) in ascending point order, with every number taken from the device.  tracks.hip drives it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <unordered_set>
#include <vector>

namespace ppsfm {

// the evolving state of a pp_tracks_handle (host side, authoritative between calls)
struct TrackState {
  int64_t L = 0;
  std::vector<int32_t> line_image, corr_start, corr_line;     // static
  std::vector<uint8_t> image_registered;                      // per image
  std::vector<int32_t> line_point;                            // L, -1 free
  std::vector<double> points;                                 // 3 per point
  std::vector<uint8_t> deleted;
  std::vector<std::vector<int32_t>> tracks;
  int NumPoints() const { return (int)tracks.size(); }
  bool Exists(int p) const { return p >= 0 && p < NumPoints() && !deleted[(size_t)p] && !tracks[(size_t)p].empty(); }
};

// the speculative closure of one point: the free lines that pass the error test, in (frontier, correspondence) order
struct SpecList { const int32_t* line; int64_t count; };

struct CompleteCounters { int64_t num_completed = 0; int32_t conflict_replays = 0; };

// Complete for ONE existing point p whose track is as the speculation saw it: `s` = the device's list of p; claim(p, line) per observation added.
// -> true if the host had to redo the walk.
template <typename ClaimFn>
inline bool ReplayCompletePoint(TrackState& st, int p, const SpecList s, int max_transitivity, ClaimFn&& claim) {
  bool conflict = false;
  for (int64_t i = 0; i < s.count && !conflict; ++i) conflict = st.line_point[(size_t)s.line[i]] != -1;
  if (!conflict) {      // nothing this point can reach was taken: its list is what the sequential loop appends
    for (int64_t i = 0; i < s.count; ++i) claim(p, s.line[i]);
    return false;
  }
  // an earlier point took one of its lines: redo the breadth-first walk with "free now and in the device's pass set" as the test
  // (the pass / fail of a (position, line) pair does not depend on the state, and what a point reaches only shrinks with fewer free lines)
  std::unordered_set<int32_t> pass(s.line, s.line + s.count);
  std::vector<int32_t> queue = st.tracks[(size_t)p], prev;
  for (int t = 0; t < max_transitivity && !queue.empty(); ++t) {
    prev.swap(queue);
    queue.clear();
    for (const int32_t fl : prev)
      for (int32_t e = st.corr_start[(size_t)fl]; e < st.corr_start[(size_t)fl + 1]; ++e) {
        const int32_t l = st.corr_line[(size_t)e];
        if (st.line_point[(size_t)l] != -1 || !pass.count(l)) continue;
        claim(p, l);
        if (t < max_transitivity - 1) queue.push_back(l);
      }
  }
  return true;
}

// Complete for the points of `subset` (nullptr = all) in ascending order.  spec(p) = the device's list of p; emit(p, line) per observation added.
template <typename SpecFn, typename EmitFn>
inline CompleteCounters ReplayComplete(TrackState& st, const uint8_t* subset, int max_transitivity, SpecFn&& spec, EmitFn&& emit) {
  CompleteCounters cnt;
  const int P = st.NumPoints();
  auto claim = [&](int p, int32_t l) {
    st.line_point[(size_t)l] = p;
    st.tracks[(size_t)p].push_back(l);
    emit(p, l);
    ++cnt.num_completed;
  };
  for (int p = 0; p < P; ++p) {
    if ((subset && !subset[p]) || !st.Exists(p)) continue;
    if (ReplayCompletePoint(st, p, spec(p), max_transitivity, claim)) ++cnt.conflict_replays;
  }
  return cnt;
}

struct MergeCounters { int64_t num_merged = 0; int64_t num_merges = 0; };

// Merge for the points of `subset` in ascending order.  eval(a, q) -> 1 / 0 / negative error: whether every element of both tracks passes at the
// merged position (the device's speculative flag, or a launch of its own for a fresh pair); emit(a, q, new_index) per merge.
template <typename EvalFn, typename EmitFn>
struct MergeReplay {
  TrackState& st;
  EvalFn& eval;
  EmitFn& emit;
  std::unordered_set<uint64_t> trials;      // merge_trials_, both orders of a pair
  MergeCounters cnt;
  int error = 0;

  static uint64_t Key(int a, int b) { return ((uint64_t)(uint32_t)a << 32) | (uint32_t)b; }

  int MergePoints(int a, int q) {      // Reconstruction::MergePoints3D (base/reconstruction.cc:206-232)
    const double la = (double)st.tracks[(size_t)a].size(), lb = (double)st.tracks[(size_t)q].size();
    const int m = st.NumPoints();
    for (int i = 0; i < 3; ++i) st.points.push_back((la * st.points[3 * (size_t)a + i] + lb * st.points[3 * (size_t)q + i]) / (la + lb));
    std::vector<int32_t> track = st.tracks[(size_t)a];
    track.insert(track.end(), st.tracks[(size_t)q].begin(), st.tracks[(size_t)q].end());
    for (const int32_t l : track) st.line_point[(size_t)l] = m;
    st.tracks[(size_t)a].clear(); st.tracks[(size_t)q].clear();
    st.deleted[(size_t)a] = st.deleted[(size_t)q] = 1;
    st.tracks.push_back(std::move(track));
    st.deleted.push_back(0);
    return m;
  }

  int64_t Merge(int a) {
    if (!st.Exists(a)) return 0;
    // (st.tracks is indexed afresh at every use: MergePoints appends to it, and a reference held across that call would dangle.  The track of `a`
    // itself does not change until a merge succeeds, after which the walk ends.)
    for (size_t ti = 0; ti < st.tracks[(size_t)a].size(); ++ti) {
      const int32_t fl = st.tracks[(size_t)a][ti];
      for (int32_t e = st.corr_start[(size_t)fl]; e < st.corr_start[(size_t)fl + 1]; ++e) {
        const int32_t l = st.corr_line[(size_t)e];
        if (!st.image_registered[(size_t)st.line_image[(size_t)l]]) continue;
        const int q = st.line_point[(size_t)l];
        if (q < 0 || q == a || trials.count(Key(a, q))) continue;
        trials.insert(Key(a, q)); trials.insert(Key(q, a));
        const int ok = eval(a, q);
        if (ok < 0) { error = ok; return 0; }
        if (!ok) continue;
        const int64_t num_merged = (int64_t)(st.tracks[(size_t)a].size() + st.tracks[(size_t)q].size());
        const int m = MergePoints(a, q);
        emit(a, q, m);
        ++cnt.num_merges;
        const int64_t rec = Merge(m);      // the original points are gone: go on with the merged one and return (:683-689)
        return rec > 0 ? rec : num_merged;
      }
    }
    return 0;
  }

  void Run(const uint8_t* subset) {
    const int P0 = st.NumPoints();
    for (int p = 0; p < P0 && !error; ++p) {
      if (subset && !subset[p]) continue;
      cnt.num_merged += Merge(p);
    }
  }
};

}  // namespace ppsfm
