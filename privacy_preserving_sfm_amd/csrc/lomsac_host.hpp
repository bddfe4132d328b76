// Host replay of ransac_lib::LocallyOptimizedMSAC (reference lib/RansacLib/RansacLib/ransac.h:127-271, 337-406; sampling.h:46-135;
// utils.h:48-58, 110-132) - std only, no HIP: every accept, every local optimisation and every termination of pp_planar_lomsac, pp_pose2d_lomsac and
// pp_fourview2d_lomsac, in iteration order, over a Backend that solves and scores.  The minimal solves + scores of a CHUNK of iterations come from the
// backend in one batch (the sampler stream does not depend on results); the bookkeeping is replayed here.  RNG = this toolchain's <random>, exactly as
// the reference uses it.  init_solvers.hip drives it with its three device backends; tests/lomsac_host_driver.cpp with a toy one, on the CPU.
//
// Backend:
//   static constexpr int kDim, kMinSample, kNonMinSample          doubles per model; min_sample_size(); non_minimal_sample_size()
//   static constexpr bool kDeferredScores                         the scores inside a local optimisation are asked for by ticket (below)
//   int n() const                                                 num_data()
//   int rc                                                        != 0 once an evaluation failed; LoMsacRun returns it
//   int BatchSolveScore(uint32_t want, const int32_t* samples /*want x kMinSample*/, std::vector<double>* models /*want x kDim*/,
//                       std::vector<double>* scores, double* device_seconds)
//                                                                 MinimalSolver + ScoreModel of `want` samples, the best of each sample's candidates;
//                                                                 a model with a non-finite entry = "no model"; != 0 ends the run with that code
//   double ScoreModel(double* model)                              ransac.h:291-299
//   int GetInliers(double* model, double thr, std::vector<int>*)  error < thr, ascending; -> their number
//   bool Solve(const std::vector<int>& sample, double* model)     NonMinimalSolver
//   void LeastSquares(const std::vector<int>& sample, double* model)
//   kDeferredScores only:
//   int ScoreModelDeferred(double* model)                         -> ticket
//   void ResolveScores(std::vector<Cand>*)                        fills Cand::score (and may refresh Cand::m) of every candidate from Cand::ticket
#pragma once
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <vector>

#include "../../include/ppsfm_hip.h"      // pp_lomsac_options, pp_lomsac_report, PP_OK (plain C)

namespace ppsfm {

// the MSAC sum in WaveMsac's order (init_solvers.hip), so that a model scored on the host (ScoreModel, from downloaded errors) and in a batch
// on the device gets the same bits
inline double TreeMsacScore(const double* err, int n, double thr) {
  double acc[64];
  for (int l = 0; l < 64; ++l) acc[l] = 0.0;
  for (int i = 0; i < n; ++i) acc[i & 63] += std::min(err[i], thr);   // ransac.h:296 (a NaN error poisons the score)
  for (int off = 32; off > 0; off >>= 1) {
    double nxt[64];
    for (int l = 0; l < 64; ++l) nxt[l] = acc[l] + acc[l ^ off];
    for (int l = 0; l < 64; ++l) acc[l] = nxt[l];
  }
  return acc[0];
}

inline uint32_t NumRequiredIterations(double inlier_ratio, double prob_missing, int sample_size, uint32_t min_it, uint32_t max_it) {
  if (inlier_ratio <= 0.0) return max_it;        // utils.h:110-132
  if (inlier_ratio >= 1.0) return min_it;
  const double p = 1.0 - std::pow(inlier_ratio, static_cast<double>(sample_size));
  const double it = std::ceil(std::log(prob_missing) / std::log(p) + 0.5);
  return std::max(min_it, std::min(static_cast<uint32_t>(it), max_it));
}
inline void RandomShuffle(std::mt19937* rng, std::vector<int>* v) {   // utils.h:48-58
  const int n = static_cast<int>(v->size());
  for (int i = 0; i < n - 1; ++i) { std::uniform_int_distribution<int> d(i, n - 1); std::swap((*v)[i], (*v)[d(*rng)]); }
}

class UniformSampling {   // sampling.h:46-135
 public:
  UniformSampling(unsigned seed, int num_data, int sample_size) : n_(num_data), k_(sample_size) {
    rng_.seed(seed);
    draw_ = static_cast<double>(num_data) / static_cast<double>(num_data - sample_size) < M_E;
    dist_.param(std::uniform_int_distribution<int>::param_type(0, n_ - 1));
  }
  void Sample(int* out) {
    if (draw_) {
      for (int i = 0; i < k_; ++i) {
        bool found = true;
        while (found) { found = false; out[i] = dist_(rng_); for (int j = 0; j < i; ++j) if (out[j] == out[i]) { found = true; break; } }
      }
    } else {
      std::vector<int> v(n_);
      std::iota(v.begin(), v.end(), 0);
      if (k_ != n_) RandomShuffle(&rng_, &v);
      for (int i = 0; i < k_; ++i) out[i] = v[i];
    }
  }
 private:
  std::mt19937 rng_; std::uniform_int_distribution<int> dist_; int n_, k_; bool draw_;
};

// LocalOptimization (ransac.h:337-406)
template <class Backend>
inline void LocalOptimization(const pp_lomsac_options& o, Backend& be, std::array<double, Backend::kDim>* best_min, double* score_best) {
  typedef std::array<double, Backend::kDim> Model;
  const int kN = be.n(), kMinNonMin = Backend::kNonMinSample, kMin = Backend::kMinSample;
  if (kMinNonMin > kN) return;
  const double thr = o.squared_inlier_threshold, mult = o.threshold_multiplier;
  std::mt19937 rng; rng.seed(o.random_seed);
  // ScoreModel + UpdateBestModel (ransac.h:399-404).  Nothing inside a local optimisation READS the best score or model - the loop's control flow depends on
  // inlier lists and on whether the non-minimal solver found a model -, so a backend whose models live on the device (kDeferredScores) only enqueues the
  // score here and the candidates are compared, in the order they were produced and with the same strict <, when the local optimisation is over.
  struct Cand { double score; Model m; int ticket; };
  std::vector<Cand> cand;
  auto consider = [&](Model& m) {
    if constexpr (Backend::kDeferredScores) { const int t = be.ScoreModelDeferred(m.data()); cand.push_back(Cand{0.0, m, t}); }
    else { const double sc = be.ScoreModel(m.data()); if (sc < *score_best) { *score_best = sc; *best_min = m; } }
  };
  auto lsq_fit = [&](double thresh, Model* m) {   // LeastSquaresFit: the rng draws happen even where LeastSquares is a no-op
    const int kSize = o.min_sample_multiplicator * kMin;
    std::vector<int> inl;
    const int ni = be.GetInliers(m->data(), thresh, &inl);
    if (ni < kMin) return;
    RandomShuffle(&rng, &inl);
    inl.resize(std::min(kSize, ni));
    be.LeastSquares(inl, m->data());
  };
  Model m_init = *best_min;
  lsq_fit(thr * mult, &m_init);
  consider(m_init);
  std::vector<int> base;
  be.GetInliers(m_init.data(), thr, &base);
  const int kNonMin = std::max(kMinNonMin, std::min(kMin * o.non_min_sample_multiplier, static_cast<int>(base.size()) / 2));
  for (int r = 0; r < o.num_lo_steps; ++r) {
    std::vector<int> sample = base;
    RandomShuffle(&rng, &sample);
    sample.resize(kNonMin);     // vector::resize value-initialises missing entries, as RandomShuffleAndResize does
    Model m_non_min;
    if (!be.Solve(sample, m_non_min.data())) continue;
    consider(m_non_min);
    lsq_fit(thr, &m_non_min);
    double thresh = mult * thr;
    const double upd = (mult - 1.0) * thr / static_cast<int>(o.num_lsq_iterations - 1);
    for (int i = 0; i < o.num_lsq_iterations; ++i) {
      lsq_fit(thresh, &m_non_min);
      consider(m_non_min);
      thresh -= upd;
    }
  }
  if constexpr (Backend::kDeferredScores) {
    be.ResolveScores(&cand);
    for (const Cand& c : cand) if (c.score < *score_best) { *score_best = c.score; *best_min = c.m; }
  }
}

// LocallyOptimizedMSAC::EstimateModel (ransac.h:127-271): the minimal solves + scores of a chunk of iterations come from the backend in one batch,
// the bookkeeping is replayed in iteration order.  -> PP_OK, or the backend's code (BatchSolveScore's, or its rc).
template <class Backend>
inline int LoMsacRun(const pp_lomsac_options* o, Backend& be, pp_lomsac_report* rep, std::array<double, Backend::kDim>* best_out, std::vector<int>* inliers_out) {
  typedef std::array<double, Backend::kDim> Model;
  const auto t0 = std::chrono::steady_clock::now();
  std::memset(rep, 0, sizeof(*rep));
  rep->best_model_score = std::numeric_limits<double>::max();
  const int kMin = Backend::kMinSample, kN = be.n();
  Model best_model; best_model.fill(0.0);
  Model best_min = best_model;
  std::vector<int>& inliers = *inliers_out;
  inliers.clear();
  if (kMin > kN) { *best_out = best_model; return PP_OK; }
  const double thr = o->squared_inlier_threshold;
  const double kMax = std::numeric_limits<double>::max();
  UniformSampling sampler(o->random_seed, kN, kMin);
  uint32_t max_it = std::max(o->max_num_iterations, o->min_num_iterations);
  double best_min_score = kMax;
  auto refresh = [&]() {
    rep->best_num_inliers = be.GetInliers(best_model.data(), thr, &inliers);
    rep->inlier_ratio = static_cast<double>(rep->best_num_inliers) / static_cast<double>(kN);
    max_it = NumRequiredIterations(rep->inlier_ratio, 1.0 - o->success_probability, kMin, o->min_num_iterations, o->max_num_iterations);
  };
  auto update_best = [&](double sc, const Model& m) { if (sc < rep->best_model_score) { rep->best_model_score = sc; best_model = m; } };
  const uint32_t chunk = o->chunk_iterations ? o->chunk_iterations : 1024;
  std::vector<int32_t> hs; std::vector<double> models, sc;
  uint32_t it = 0;
  double dev_s = 0;
  while (it < max_it) {
    const uint32_t want = std::min<uint32_t>(chunk, max_it - it);
    hs.resize((size_t)want * kMin);
    for (uint32_t i = 0; i < want; ++i) sampler.Sample(&hs[(size_t)kMin * i]);
    const int rc = be.BatchSolveScore(want, hs.data(), &models, &sc, &dev_s);
    if (rc) return rc;
    rep->hypotheses_evaluated += want;
    // replay of ransac.h:155-237 in iteration order; the sampler has already been advanced for the whole
    // chunk, which is harmless because nothing after an early exit draws from it
    for (uint32_t i = 0; i < want && it < max_it; ++i, ++it) {
      if (it == o->lo_starting_iterations && best_min_score < kMax) {
        ++rep->number_lo_iterations;
        LocalOptimization(*o, be, &best_model, &rep->best_model_score);
        refresh();
      }
      Model m;
      bool finite = true;
      for (int k = 0; k < Backend::kDim; ++k) { m[k] = models[(size_t)Backend::kDim * i + k]; finite = finite && std::isfinite(m[k]); }
      if (!finite) continue;   // MinimalSolver returned 0 models
      const double best_local = sc[i];
      if (best_local < best_min_score || it == o->lo_starting_iterations) {
        const bool kBestMin = best_local < best_min_score;
        if (kBestMin) { best_min_score = best_local; best_min = m; update_best(best_min_score, best_min); }
        const bool kRunLO = it >= o->lo_starting_iterations && best_min_score < kMax;
        if (!kBestMin && !kRunLO) continue;
        if (kRunLO) {
          ++rep->number_lo_iterations;
          double score = best_min_score;
          LocalOptimization(*o, be, &best_min, &score);
          update_best(score, best_min);
        }
        refresh();
      }
    }
    if (be.rc) return be.rc;
  }
  rep->num_iterations = it;
  if (it <= o->lo_starting_iterations && rep->best_model_score < kMax) {
    ++rep->number_lo_iterations;
    LocalOptimization(*o, be, &best_model, &rep->best_model_score);
    rep->best_num_inliers = be.GetInliers(best_model.data(), thr, &inliers);
    rep->inlier_ratio = static_cast<double>(rep->best_num_inliers) / static_cast<double>(kN);
  }
  if (o->final_least_squares) {   // ransac.h:253-268
    Model refined = best_model;
    be.LeastSquares(inliers, refined.data());
    const double score = be.ScoreModel(refined.data());
    if (score < rep->best_model_score) {
      rep->best_model_score = score; best_model = refined;
      rep->best_num_inliers = be.GetInliers(best_model.data(), thr, &inliers);
      rep->inlier_ratio = static_cast<double>(rep->best_num_inliers) / static_cast<double>(kN);
    }
  }
  if (be.rc) return be.rc;
  *best_out = best_model;
  rep->num_inlier_indices = (int32_t)inliers.size();
  rep->device_time_s = dev_s;
  rep->total_time_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return PP_OK;
}

}  // namespace ppsfm
