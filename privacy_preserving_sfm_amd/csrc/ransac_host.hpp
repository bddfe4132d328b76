// Host-side pieces of the RANSAC driver that must stay sequential and bit-compatible with the
// reference: the sampler, the trial-count rule and the replay of RANSAC<P6LEstimator>::Estimate.
// std + the plain-C header only, no HIP: tests/pose_ransac_replay_host_driver.cpp runs it on the CPU.
//
//   RandomSampler::{Initialize, Sample}  reference src/optim/random_sampler.cc:43-62
//   Shuffle / RandomInteger              src/util/random.h:88-128 (thread-local std::mt19937,
//                                        std::uniform_int_distribution<uint32_t>(i, last))
//   RANSAC::ComputeNumTrials             src/optim/ransac.h:158-176
//   RANSAC ctor, RANSAC::Estimate        src/optim/ransac.h:143-156, 178-278 (PoseRansacReplay)
// The sampler uses the host toolchain's own <random>, exactly like the reference does, so the
// index stream is the reference's stream on the same libstdc++ by construction.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <vector>

#include "../../include/ppsfm_hip.h"      // pp_ransac_options, pp_ransac_report (plain C)

namespace ppsfm {

class RandomSampler {
 public:
  RandomSampler(int num_samples, uint32_t seed) : k_(num_samples), prng_(seed) {}
  void Initialize(uint32_t total) {
    idx_.resize(total);
    std::iota(idx_.begin(), idx_.end(), 0u);
  }
  // partial Fisher-Yates on the PERSISTENT permutation: sample t depends on all earlier samples
  void Sample(uint32_t* out) {
    const uint32_t last = static_cast<uint32_t>(idx_.size() - 1);
    for (uint32_t i = 0; i < static_cast<uint32_t>(k_); ++i) {
      std::uniform_int_distribution<uint32_t> dist(i, last);
      const uint32_t j = dist(prng_);
      std::swap(idx_[i], idx_[j]);
    }
    for (int i = 0; i < k_; ++i) out[i] = idx_[i];
  }
  // the next `count` samples, one after the other: out count x k
  void Fill(uint64_t count, uint32_t* out) {
    for (uint64_t i = 0; i < count; ++i) Sample(out + static_cast<size_t>(k_) * i);
  }

 private:
  int k_;
  std::mt19937 prng_;
  std::vector<uint32_t> idx_;
};

inline uint64_t ComputeNumTrials(uint64_t num_inliers, uint64_t num_samples, double confidence, double multiplier,
                                 int min_num_samples) {
  const double inlier_ratio = num_inliers / static_cast<double>(num_samples);
  const double nom = 1 - confidence;
  if (nom <= 0) return std::numeric_limits<uint64_t>::max();
  const double denom = 1 - std::pow(inlier_ratio, min_num_samples);
  if (denom <= 0) return 1;
  return static_cast<uint64_t>(std::ceil(std::log(nom) / std::log(denom) * multiplier));
}

// One chunk of trials as a backend solved and scored it (host pointers): the models of trial i are models[(i * 8 + m) * 12 ..], m < num_models[i],
// inliers[i * 8 + m] their inlier counts.  A slot is i * 8 + m.
struct PoseChunk {
  const int32_t* num_models;   // width
  const uint32_t* inliers;     // width x 8
  const double* models;        // width x 8 x 12
};

// RANSAC<P6LEstimator, InlierSupportMeasurer, RandomSampler>::Estimate (optim/ransac.h:143-278) over a backend that solves and scores whole chunks
// of trials ahead of the loop (speculation): everything sequential - the trial cap, the sampler, the chunk width, accept and tie-break in trial order,
// the adaptive termination, num_trials - lives here, the arithmetic in the backend.  The result does not depend on the chunk width.
//
//   PoseRansacReplay replay(options, n);
//   while (!replay.Done()) {
//     width = replay.Draw(samples);                       -> the backend solves and scores the `width` six-tuples: a PoseChunk
//     replay.Candidates(width, chunk, &slots);            -> the backend sums the inlier residuals of these models in index order
//     replay.Consume(width, chunk, slots, exact_sums);    (support_measurement.cc:40-47): exact_sums[k] belongs to slots[k]
//   }
//   report = replay.Finish();
//
// Steps, not a callback: several replays can advance over one batched launch.  pp_pose_ransac (abs_pose.hip) is the device backend,
// tests/pose_ransac_replay_host_driver.cpp one on the CPU.
class PoseRansacReplay {
 public:
  static constexpr int kMinNumSamples = 6;
  uint64_t num_ties = 0, num_ties_won = 0;      // trace: models that tied with the best on the count / of them, accepted on the smaller sum

  PoseRansacReplay(const pp_ransac_options& o, int n) : o_(o), n_(n), sampler_(kMinNumSamples, o.seed) {
    std::memset(&rep_, 0, sizeof(rep_));
    rep_.best_trial = -1; rep_.best_model_index = -1;
    rep_.residual_sum = DBL_MAX;      // with num_inliers = 0: InlierSupportMeasurer::Support's default (support_measurement.h:44-50)
    if (n < kMinNumSamples) return;   // ransac.h:192-194: max_num_trials_ stays 0, Done() at once
    // ctor: a-priori cap of max_num_trials (ransac.h:149-155)
    const uint64_t kNumSamples = 100000;
    max_num_trials_ = std::min<uint64_t>(o.max_num_trials, ComputeNumTrials(static_cast<uint64_t>(o.min_inlier_ratio * kNumSamples), kNumSamples, o.confidence,
                                                                            o.dyn_num_trials_multiplier, kMinNumSamples));
    dyn_max_num_trials_ = max_num_trials_;
    sampler_.Initialize(static_cast<uint32_t>(n));
  }

  uint64_t MaxWidth() const { return o_.chunk_trials ? o_.chunk_trials : 1024; }      // no Draw() returns more
  bool Done() const { return !(trial_ < max_num_trials_ && !abort_); }

  // the next chunk: its width, its six-tuples in samples[width x 6]
  uint64_t Draw(uint32_t* samples) {
    // speculate: never beyond the static cap; shrink towards the dynamic bound once it is known
    uint64_t want = std::min<uint64_t>(MaxWidth(), max_num_trials_ - trial_);
    if (dyn_max_num_trials_ < max_num_trials_) {
      const uint64_t floor_trials = std::max<uint64_t>(dyn_max_num_trials_, o_.min_num_trials);
      if (floor_trials > trial_) want = std::min<uint64_t>(want, floor_trials - trial_ + 1);
      else want = std::min<uint64_t>(want, 64);
    }
    want = std::max<uint64_t>(want, 1);
    sampler_.Fill(want, samples);      // (draws past an early exit are harmless: nothing after it samples)
    rep_.hypotheses_evaluated += want;
    return want;
  }

  // The models whose exact (sequential-order) residual sum Consume() can ask for: a model can only become the best or tie with it if its inlier
  // count reaches the running maximum of the counts before it, and that maximum follows from the counts alone.  Slots ascending.
  void Candidates(uint64_t width, const PoseChunk& c, std::vector<size_t>* slots) const {
    slots->clear();
    uint64_t run = rep_.num_inliers;
    for (uint64_t i = 0; i < width; ++i)
      for (int m = 0; m < c.num_models[i]; ++m) {
        const uint64_t count = c.inliers[i * 8 + m];
        if (count < run) continue;
        slots->push_back(static_cast<size_t>(i * 8 + m));
        run = count;
      }
  }

  // replay of ransac.h:213-249 in trial order.  InlierSupportMeasurer::Compare (support_measurement.cc:49-60): more inliers, or as many and a smaller
  // sequential sum - the first model meets the default Support{0, DBL_MAX} like any other.
  void Consume(uint64_t width, const PoseChunk& c, const std::vector<size_t>& slots, const double* exact_sums) {
    size_t k = 0;      // slots[k] is the first candidate at or after the current slot
    for (uint64_t i = 0; i < width && !Done(); ++i, ++trial_) {
      for (int m = 0; m < c.num_models[i]; ++m) {
        rep_.models_scored += 1;
        const size_t slot = static_cast<size_t>(i * 8 + m);
        const uint64_t count = c.inliers[slot];
        if (count >= rep_.num_inliers) {      // a candidate
          while (slots[k] < slot) ++k;
          const bool tie = count == rep_.num_inliers, better = !tie || exact_sums[k] < rep_.residual_sum;
          num_ties += tie; num_ties_won += tie && better;
          if (better) {
            rep_.num_inliers = count; rep_.residual_sum = exact_sums[k];
            std::memcpy(rep_.model, c.models + slot * 12, sizeof(rep_.model));
            rep_.best_trial = static_cast<int64_t>(trial_); rep_.best_model_index = m;
            dyn_max_num_trials_ = ComputeNumTrials(count, static_cast<uint64_t>(n_), o_.confidence, o_.dyn_num_trials_multiplier, kMinNumSamples);
          }
        }
        if (trial_ >= dyn_max_num_trials_ && trial_ >= o_.min_num_trials) { abort_ = true; break; }
      }
    }
  }

  // the report, but for the two times: final once Done(), the preset before the first chunk
  pp_ransac_report Finish() const {
    pp_ransac_report r = rep_;
    // num_trials bookkeeping of the reference loop (ransac.h:213-218): an abort raised in trial t ends the run with num_trials = t + 2 (for-increment,
    // then the `if (abort) num_trials += 1`), or t + 1 when t + 1 already equals max_num_trials; Consume() leaves trial_ == t + 1 behind
    r.num_trials = (abort_ && trial_ < max_num_trials_) ? trial_ + 1 : trial_;
    r.success = r.num_inliers >= static_cast<uint64_t>(kMinNumSamples);
    return r;
  }

 private:
  pp_ransac_options o_;
  int n_;
  RandomSampler sampler_;
  pp_ransac_report rep_;      // num_inliers, residual_sum, model, best_*: the best support so far
  uint64_t max_num_trials_ = 0, dyn_max_num_trials_ = 0, trial_ = 0;
  bool abort_ = false;
};

}  // namespace ppsfm
