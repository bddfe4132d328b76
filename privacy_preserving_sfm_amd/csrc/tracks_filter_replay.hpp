// Host replay of the deletions on a pp_tracks_handle - std only, no HIP: the three filters of the mapper and the de-registration of an image
//   Reconstruction::DeletePoint3D / DeleteObservation       reference src/base/reconstruction.cc:234-275
//   Reconstruction::DeRegisterImage                                                              :285-300
//   Reconstruction::FilterObservationsWithNegativeDepth                                          :442-460
//   Reconstruction::FilterImages                                                                 :462-484
//   Reconstruction::FilterPoints3D (the two point filters)                                       :425-439, 594-719
// The device gives the verdicts (tracks_filter.hip: K14a per point and per track element, K14b per line); the sequential part - a track that falls to three
// elements takes its point with it, a line whose point an earlier deletion removed is not counted - is replayed here.  tracks_filter.hip drives it.
// EVENTS, in the order the reference's Reconstruction sees them: emit(p, l) for a DeleteObservation that removed one element, emit(p, -1) for a DeletePoint3D.
// DeRegisterImage and FilterImages need no kernel: one pass over the L lines on the host.
#pragma once
#include <cstdint>
#include <vector>

#include "tracks_replay.hpp"

namespace ppsfm {

enum : uint8_t { kFilterNotTested = 0, kFilterKept = 1, kFilterDeletedByTrack = 2, kFilterDeletedByAngle = 3 };      // K14a's verdict per point

struct FilterCounts {
  int64_t num_filtered = 0;                 // the reference's return value
  int64_t num_points_deleted = 0;
  int64_t num_observations_deleted = 0;     // track elements removed, those of deleted points included
  int32_t points_tested = 0, images_filtered = 0;
};

// DeletePoint3D -> the number of track elements that went with the point
inline int64_t DeletePoint(TrackState& st, int p) {
  std::vector<int32_t>& track = st.tracks[(size_t)p];
  const int64_t n = (int64_t)track.size();
  for (const int32_t l : track) st.line_point[(size_t)l] = -1;
  track.clear();
  st.deleted[(size_t)p] = 1;
  return n;
}

// DeleteObservation of a line that has a point -> true when the whole point went (a track of at most three elements, :264-267)
inline bool DeleteObservation(TrackState& st, int32_t l, int64_t* elements_removed) {
  const int p = st.line_point[(size_t)l];
  std::vector<int32_t>& track = st.tracks[(size_t)p];
  if (track.size() <= 3) { *elements_removed = DeletePoint(st, p); return true; }
  for (size_t i = 0; i < track.size(); ++i)
    if (track[i] == l) { track.erase(track.begin() + (std::ptrdiff_t)i); break; }      // Track::DeleteElement: the order of the others stays
  st.line_point[(size_t)l] = -1;
  *elements_removed = 1;
  return false;
}

template <typename EmitFn>
inline void DeleteObservationEvent(TrackState& st, int32_t l, FilterCounts& cnt, EmitFn&& emit) {
  const int p = st.line_point[(size_t)l];
  int64_t removed = 0;
  if (DeleteObservation(st, l, &removed)) { emit(p, -1); ++cnt.num_points_deleted; }
  else emit(p, l);
  cnt.num_observations_deleted += removed;
}

// The point filters.  verdict / ndel / error: P each; elem_flag: aligned with the track CSR `start` the device saw (the tracks of st are still those).
// Ascending point index, within a point in track order.  point_error (P, may be null): -1 where the filter did not set Point3D::Error.
template <typename EmitFn>
inline FilterCounts ApplyPointFilter(TrackState& st, const int32_t* start, const uint8_t* verdict, const int32_t* ndel, const double* error, const uint8_t* elem_flag,
                                     double* point_error, EmitFn&& emit) {
  FilterCounts cnt;
  const int P = st.NumPoints();
  std::vector<int32_t> gone;
  for (int p = 0; p < P; ++p) {
    if (point_error) point_error[p] = -1.0;
    const uint8_t v = verdict[p];
    if (v == kFilterNotTested) continue;
    ++cnt.points_tested;
    const int64_t len = (int64_t)st.tracks[(size_t)p].size();
    if (v == kFilterDeletedByTrack || v == kFilterDeletedByAngle) {
      // :673-689, :705-707 count the track; :649-652 counts the point once, after the observations :709-713 removed
      cnt.num_filtered += v == kFilterDeletedByTrack ? len : (int64_t)ndel[p] + 1;
      emit(p, -1);
      cnt.num_observations_deleted += DeletePoint(st, p);
      ++cnt.num_points_deleted;
      continue;
    }
    gone.clear();
    for (int64_t i = 0; i < len; ++i) if (elem_flag[start[p] + i]) gone.push_back(st.tracks[(size_t)p][(size_t)i]);
    for (const int32_t l : gone) DeleteObservationEvent(st, l, cnt, emit);      // (more than three stay: the point never goes here)
    cnt.num_filtered += (int64_t)gone.size();
    if (point_error) point_error[p] = error[p];
  }
  return cnt;
}

// true when image_order lists exactly the registered images, each once
inline bool IsRegistrationOrder(const TrackState& st, const int32_t* image_order, int32_t n) {
  const int32_t C = (int32_t)st.image_registered.size();
  if (n < 0 || (n > 0 && !image_order)) return false;
  std::vector<uint8_t> seen((size_t)C, 0);
  for (int32_t i = 0; i < n; ++i) {
    const int32_t c = image_order[i];
    if (c < 0 || c >= C || !st.image_registered[(size_t)c] || seen[(size_t)c]) return false;
    seen[(size_t)c] = 1;
  }
  int32_t reg = 0;
  for (int32_t c = 0; c < C; ++c) reg += st.image_registered[(size_t)c] != 0;
  return reg == n;
}

// the lines of every image in ascending line index, as a CSR over the images
struct ImageLines {
  std::vector<int32_t> start, line;
  explicit ImageLines(const TrackState& st) {
    const size_t C = st.image_registered.size();
    start.assign(C + 1, 0);
    for (int64_t l = 0; l < st.L; ++l) ++start[(size_t)st.line_image[(size_t)l] + 1];
    for (size_t c = 0; c < C; ++c) start[c + 1] += start[c];
    line.resize((size_t)st.L);
    std::vector<int32_t> at(start.begin(), start.end() - 1);
    for (int64_t l = 0; l < st.L; ++l) line[(size_t)at[(size_t)st.line_image[(size_t)l]]++] = (int32_t)l;
  }
};

// FilterObservationsWithNegativeDepth: the images in registration order, the lines of each in ascending index; line_flag = K14b's verdict on the state at
// the start.  A flagged line whose point an earlier deletion took is not counted: the reference finds it without a point.
template <typename EmitFn>
inline FilterCounts ReplayNegativeDepth(TrackState& st, const int32_t* image_order, int32_t n, const uint8_t* line_flag, EmitFn&& emit) {
  FilterCounts cnt;
  const ImageLines il(st);
  for (int32_t i = 0; i < n; ++i) {
    const size_t c = (size_t)image_order[i];
    for (int32_t e = il.start[c]; e < il.start[c + 1]; ++e) {
      const int32_t l = il.line[(size_t)e];
      if (st.line_point[(size_t)l] < 0 || !line_flag[(size_t)l]) continue;
      DeleteObservationEvent(st, l, cnt, emit);
      ++cnt.num_filtered;
    }
  }
  return cnt;
}

template <typename EmitFn>
inline void DeRegisterImage(TrackState& st, const ImageLines& il, int32_t image, FilterCounts& cnt, EmitFn&& emit) {
  for (int32_t e = il.start[(size_t)image]; e < il.start[(size_t)image + 1]; ++e) {
    const int32_t l = il.line[(size_t)e];
    if (st.line_point[(size_t)l] >= 0) DeleteObservationEvent(st, l, cnt, emit);
  }
  st.image_registered[(size_t)image] = 0;
}

// FilterImages: the registered images without a point or with a flagged camera (image_skip, per image), collected first, then de-registered in list order.
// filtered (room for every image) receives them; cnt.images_filtered counts them; num_filtered is the same number (the mapper's return value).
template <typename EmitFn>
inline FilterCounts ReplayFilterImages(TrackState& st, const uint8_t* image_skip, const int32_t* image_order, int32_t n, int32_t* filtered, EmitFn&& emit) {
  FilterCounts cnt;
  const ImageLines il(st);
  for (int32_t i = 0; i < n; ++i) {
    const size_t c = (size_t)image_order[i];
    bool has_point = false;
    for (int32_t e = il.start[c]; e < il.start[c + 1] && !has_point; ++e) has_point = st.line_point[(size_t)il.line[(size_t)e]] >= 0;
    if (!has_point || image_skip[c]) filtered[cnt.images_filtered++] = (int32_t)c;
  }
  for (int32_t i = 0; i < cnt.images_filtered; ++i) DeRegisterImage(st, il, filtered[i], cnt, emit);
  cnt.num_filtered = cnt.images_filtered;
  return cnt;
}

}  // namespace ppsfm
