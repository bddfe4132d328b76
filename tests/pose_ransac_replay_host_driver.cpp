// Driver of tests/test_pose_ransac_replay_host.py: ppsfm::PoseRansacReplay (csrc/ransac_host.hpp) - the product's replay of RANSAC<P6LEstimator>::Estimate -
// compiled with plain g++, no device and no library.  The backend is the oracle's own arithmetic: oracle::P6LEstimate for a sample,
// oracle::SquaredLineReprojectionError + oracle::EvaluateSupport for the counts of every model and for the sequential sums of the candidate slots only.
//
//   sweep | subsweep   the replay against oracle::P6LRansac (oracle/ransac.h) on the same data and seed over a grid, report and model compared with == and
//                      memcmp; prints the first mismatches and exits 1, else `cases=... mismatches=0` and how often each rule was exercised.
//                      subsweep: seed 1 and chunk widths {1, 7, 0} only (the sanitized build's share)
//   sampler            1000 draws of ppsfm::RandomSampler against oracle::RandomSampler for several sizes and seeds
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../oracle/ransac.h"
#include "../privacy_preserving_sfm_amd/csrc/ransac_host.hpp"

struct Scene { int n; std::vector<double> lines, points; std::vector<uint8_t> aligned; };

// points in a unit cube seen by one fixed pose, a line through each noisy projection, uniform outliers; an aligned line is vertical
static Scene MakeScene(int n, double outlier_ratio, double aligned_ratio, unsigned seed) {
  std::mt19937 g(seed);
  std::uniform_real_distribution<double> u(-1, 1);
  auto u01 = [&]() { return 0.5 * u(g) + 0.5; };
  Scene s;
  s.n = n; s.lines.resize(3 * n); s.points.resize(3 * n); s.aligned.resize(n);
  const double a = 0.3, R[9] = {std::cos(a), 0, std::sin(a), 0, 1, 0, -std::sin(a), 0, std::cos(a)}, t[3] = {0.1, -0.2, 4.0};
  for (int i = 0; i < n; ++i) {
    double X[3] = {u(g), u(g), u(g)}, p[3];
    for (int r = 0; r < 3; ++r) p[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
    double x = p[0] / p[2] + 1e-4 * u(g), y = p[1] / p[2] + 1e-4 * u(g);
    if (u01() < outlier_ratio) { x = u(g); y = u(g); }
    s.aligned[i] = u01() < aligned_ratio;
    const double th = s.aligned[i] ? 0.0 : 3.14159 * u(g);
    const double la = std::cos(th), lb = std::sin(th);
    s.lines[3 * i] = la; s.lines[3 * i + 1] = lb; s.lines[3 * i + 2] = -(la * x + lb * y);
    for (int r = 0; r < 3; ++r) s.points[3 * i + r] = X[r];
  }
  return s;
}

static pp_ransac_options Options(int set, unsigned seed) {
  pp_ransac_options o;
  std::memset(&o, 0, sizeof(o));
  // 0: the mapper's (sfm/incremental_mapper.cc:673-681, a lower cap)
  o.max_error = 2e-3; o.min_inlier_ratio = 0.25; o.confidence = 0.99999; o.dyn_num_trials_multiplier = 3.0; o.min_num_trials = 100; o.max_num_trials = 2000;
  o.seed = seed;
  if (set == 1) { o.min_num_trials = 0; o.confidence = 0.99; o.min_inlier_ratio = 0.1; }      // the defaults of ransac.h:47-66
  if (set == 2) o.max_num_trials = 1;
  if (set == 3) { o.confidence = 1.0; o.max_num_trials = 300; }      // ComputeNumTrials = max: never ends early
  if (set == 4) o.min_inlier_ratio = 1.0;      // a-priori cap of 1
  if (set == 5) { o.min_inlier_ratio = 0.0; o.min_num_trials = o.max_num_trials = 150; }
  return o;
}

static oracle::RansacReport RunOracle(const Scene& s, const pp_ransac_options& o) {
  oracle::RansacOptions r;
  r.max_error = o.max_error; r.min_inlier_ratio = o.min_inlier_ratio; r.confidence = o.confidence; r.dyn_num_trials_multiplier = o.dyn_num_trials_multiplier;
  r.min_num_trials = o.min_num_trials; r.max_num_trials = o.max_num_trials;
  return oracle::P6LRansac(r, s.n, s.lines.data(), s.points.data(), s.aligned.data(), o.seed);
}

struct Run { pp_ransac_report rep; uint64_t ties, ties_won; };

static Run RunReplay(const Scene& s, const pp_ransac_options& o) {
  const double max_residual = o.max_error * o.max_error;
  const double *lines = s.lines.data(), *points = s.points.data();
  ppsfm::PoseRansacReplay replay(o, s.n);
  std::vector<uint32_t> samples(6 * replay.MaxWidth()), inliers;
  std::vector<int32_t> num_models;
  std::vector<double> models, residuals(s.n), sums;
  std::vector<size_t> slots;
  auto support = [&](const double* model) {
    oracle::SquaredLineReprojectionError(s.n, lines, points, model, residuals.data());
    return oracle::EvaluateSupport(s.n, residuals.data(), max_residual);
  };
  while (!replay.Done()) {
    const uint64_t width = replay.Draw(samples.data());
    num_models.assign(width, 0); inliers.assign(width * 8, 0); models.assign(width * 96, 0.0);
    for (uint64_t i = 0; i < width; ++i) {
      double l6[18], p6[18];
      uint8_t a6[6];
      for (int k = 0; k < 6; ++k) {
        const uint32_t id = samples[6 * i + k];
        for (int c = 0; c < 3; ++c) { l6[3 * k + c] = lines[3 * id + c]; p6[3 * k + c] = points[3 * id + c]; }
        a6[k] = s.aligned[id];
      }
      num_models[i] = oracle::P6LEstimate(l6, p6, a6, &models[96 * i]);
      for (int m = 0; m < num_models[i]; ++m) inliers[8 * i + m] = (uint32_t)support(&models[96 * i + 12 * m]).num_inliers;
    }
    const ppsfm::PoseChunk chunk{num_models.data(), inliers.data(), models.data()};
    replay.Candidates(width, chunk, &slots);
    sums.resize(slots.size());
    for (size_t k = 0; k < slots.size(); ++k) sums[k] = support(&models[12 * slots[k]]).residual_sum;
    replay.Consume(width, chunk, slots, sums.data());
  }
  return Run{replay.Finish(), replay.num_ties, replay.num_ties_won};
}

static bool Same(const pp_ransac_report& r, const oracle::RansacReport& want) {
  return r.success == (int)want.success && r.num_trials == want.num_trials && r.best_trial == want.best_trial && r.best_model_index == want.best_model_idx &&
         r.num_inliers == want.support.num_inliers && r.residual_sum == want.support.residual_sum && !std::memcmp(r.model, want.model, sizeof(r.model));
}

static int Sweep(bool sub) {
  long cases = 0, mismatches = 0, oracle_trials = 0, small = 0, success = 0, early = 0, capped = 0, no_model = 0, ties = 0, ties_won = 0;
  const std::vector<unsigned> seeds = sub ? std::vector<unsigned>{1u} : std::vector<unsigned>{0u, 1u, 7u};
  const std::vector<uint32_t> chunks = sub ? std::vector<uint32_t>{1u, 7u, 0u} : std::vector<uint32_t>{1u, 2u, 7u, 64u, 0u};
  for (int n : {5, 6, 7, 12, 40, 150})
    for (double outlier_ratio : {0.0, 0.3, 0.6})
      for (double aligned_ratio : {0.0, 0.2, 1.1})
        for (unsigned seed : seeds) {
          const Scene s = MakeScene(n, outlier_ratio, aligned_ratio, 100 + seed);
          for (int set = 0; set < 6; ++set) {
            pp_ransac_options o = Options(set, seed);
            const oracle::RansacReport want = RunOracle(s, o);      // (the oracle's loop knows no chunks)
            oracle_trials += (long)want.num_trials;
            // the a-priori cap of ransac.h:149-155
            const uint64_t cap = std::min<uint64_t>(o.max_num_trials, ppsfm::ComputeNumTrials((uint64_t)(o.min_inlier_ratio * 100000), 100000, o.confidence,
                                                                                             o.dyn_num_trials_multiplier, 6));
            for (uint32_t chunk : chunks) {
              o.chunk_trials = chunk;
              const Run r = RunReplay(s, o);
              ++cases;
              small += n < 6; success += r.rep.success != 0; ties += (long)r.ties; ties_won += (long)r.ties_won;
              if (n >= 6) { early += r.rep.num_trials < cap; capped += r.rep.num_trials == cap; no_model += r.rep.best_trial < 0 && r.rep.residual_sum == DBL_MAX; }
              if (Same(r.rep, want) && r.rep.hypotheses_evaluated + 1 >= r.rep.num_trials) continue;
              if (++mismatches <= 5)
                std::printf("mismatch: n=%d outliers=%g aligned=%g seed=%u options=%d chunk=%u: trials %llu/%llu best %lld.%d/%lld.%d inliers %llu/%llu sum %.17g/%.17g\n", n,
                            outlier_ratio, aligned_ratio, seed, set, chunk, (unsigned long long)r.rep.num_trials, (unsigned long long)want.num_trials,
                            (long long)r.rep.best_trial, r.rep.best_model_index, (long long)want.best_trial, want.best_model_idx,
                            (unsigned long long)r.rep.num_inliers, (unsigned long long)want.support.num_inliers, r.rep.residual_sum, want.support.residual_sum);
            }
          }
        }
  std::printf("cases=%ld mismatches=%ld oracle_trials=%ld small=%ld success=%ld early=%ld capped=%ld no_model=%ld ties=%ld ties_won=%ld\n", cases, mismatches,
              oracle_trials, small, success, early, capped, no_model, ties, ties_won);
  return mismatches ? 1 : 0;
}

static int Sampler() {
  long draws = 0, mismatches = 0;
  for (uint32_t n : {6u, 7u, 40u, 2000u})
    for (uint32_t seed : {0u, 1u, 7u}) {
      ppsfm::RandomSampler got(6, seed);
      got.Initialize(n);
      oracle::MT19937 rng(seed);
      oracle::RandomSampler want(6, &rng);
      want.Initialize(n);
      std::vector<uint32_t> a(6 * 1000), b(6);
      got.Fill(1000, a.data());
      for (int t = 0; t < 1000; ++t, ++draws) {
        want.Sample(b.data());
        mismatches += std::memcmp(&a[6 * t], b.data(), sizeof(uint32_t) * 6) != 0;
      }
    }
  std::printf("draws=%ld mismatches=%ld\n", draws, mismatches);
  return mismatches ? 1 : 0;
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "sweep" || cmd == "subsweep") return Sweep(cmd == "subsweep");
  if (cmd == "sampler") return Sampler();
  std::fprintf(stderr, "usage: pose_ransac_replay_host_driver sweep | subsweep | sampler\n");
  return 2;
}
