// K19 - line features from keypoints: the line generation of LineFeatureWriterThread::Run (reference src/feature/extraction.cc:437-505).  Every keypoint
// is undistorted with its image's camera (ImageToWorld of camera_models.hpp) and gets a line through it: d x (u, v, 1) over the norm of its first two
// components, d the image's gravity direction for the aligned features and a random vector for the others.  What the reference leaves to chance - the
// random vectors and which features are aligned - is the counter-based generator of line_features_replay.hpp, the host half; this file is the device
// half and the C ABI.  Line index = keypoint index = descriptor row.  All arithmetic is fp64; no kernel uses an atomic or waits for another workgroup.
// K19a k_lf_select   one workgroup per image with n > 0 aligned features to choose: the n-th smallest 64-bit alignment key by a radix select over 16
//                    digits of 4 bits from the top.  A pass recomputes the keys (three multiplications each; they are never stored), every lane counts
//                    the digits of the keys that carry the prefix found so far in 16 registers, the counts are summed over the wavefront by shuffles
//                    and over the four wavefronts through LDS, and every lane picks the digit the rank falls into.  Output: one threshold key per image.
// K19b k_lf_lines    one lane per keypoint, a wavefront per tile of 64 keypoints of ONE image (the host lists the tiles), so the camera model - the
//                    switch of ImageToWorld and the trip count of its Newton loop apart - is uniform over the wavefront.  float32 (x, y) widened
//                    exactly, undistorted, the direction chosen by key <= threshold, the line written as three doubles with a flag byte per keypoint:
//                    1 aligned, 2 head norm zero or not finite (the line is written as computed: the reference divides regardless), 4 the Newton
//                    iteration ran all of its 100 iterations.  The host counts the flags.
#include <cstring>

#include "camera_models.hpp"
#include "line_features_replay.hpp"
#include "device_handle.hpp"

namespace ppsfm {

constexpr int kLfBlock = 256;
constexpr int kLfTile = kWave;                       // keypoints per wavefront of k_lf_lines
constexpr int kLfWaves = kLfBlock / kWave;

struct LfImageDev {
  uint64_t state;        // LfImageState(seed, image id)
  int64_t kp0;           // first global keypoint
  int32_t count;         // keypoints
  int32_t num_aligned;   // features to align: 0 without gravity
  int32_t camera;
  int32_t reserved_;
};

struct LfTileDev { int32_t image, first; };          // keypoints first .. first + 63 of the image

__global__ __launch_bounds__(kLfBlock) void k_lf_select(const int32_t* __restrict__ todo, const LfImageDev* __restrict__ images, uint64_t* __restrict__ threshold) {
  __shared__ int32_t part[kLfWaves][16];
  const int32_t img = todo[blockIdx.x];
  const LfImageDev q = images[img];
  const int tid = threadIdx.x;
  uint64_t prefix = 0;
  int32_t rank = q.num_aligned;                      // 1 <= rank <= count: the rank-th smallest among the keys that carry the prefix
  for (int shift = 60; shift >= 0; shift -= 4) {
    const uint64_t above = shift == 60 ? 0ull : ~0ull << (shift + 4);
    int32_t cnt[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) cnt[b] = 0;
    for (int32_t i = tid; i < q.count; i += kLfBlock) {
      const uint64_t key = LfAlignKey(q.state, i);
      const int d = (key & above) == prefix ? (int)((key >> shift) & 15) : -1;
#pragma unroll
      for (int b = 0; b < 16; ++b) cnt[b] += d == b;
    }
#pragma unroll
    for (int b = 0; b < 16; ++b) cnt[b] = WaveSumInt(cnt[b]);
    if ((tid & (kWave - 1)) == 0) {
#pragma unroll
      for (int b = 0; b < 16; ++b) part[tid / kWave][b] = cnt[b];
    }
    __syncthreads();
    int32_t below = 0;
    int chosen = -1;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      int32_t t = 0;
#pragma unroll
      for (int w = 0; w < kLfWaves; ++w) t += part[w][b];
      if (chosen < 0) {
        if (below + t >= rank) chosen = b; else below += t;
      }
    }
    if (chosen < 0) chosen = 15;                     // (rank <= the keys under the prefix: not reached)
    rank -= below;
    prefix |= (uint64_t)chosen << shift;
    __syncthreads();
  }
  if (tid == 0) threshold[img] = prefix;
}

__global__ __launch_bounds__(kLfBlock) void k_lf_lines(int32_t num_tiles, const LfTileDev* __restrict__ tiles, const LfImageDev* __restrict__ images,
                                                       const uint64_t* __restrict__ threshold, const float* __restrict__ keypoints,
                                                       const int32_t* __restrict__ camera_model, const double* __restrict__ intr,
                                                       const uint8_t* __restrict__ has_gravity, const double* __restrict__ gravity,
                                                       double* __restrict__ lines, double* __restrict__ dirs, uint8_t* __restrict__ flags) {
  const int32_t t = blockIdx.x * kLfWaves + (int32_t)(threadIdx.x / kWave);
  if (t >= num_tiles) return;
  const LfTileDev tile = tiles[t];
  const LfImageDev q = images[tile.image];
  const int32_t i = tile.first + (int32_t)(threadIdx.x & (kWave - 1));
  if (i >= q.count) return;
  const int64_t g = q.kp0 + i;
  const double x = (double)keypoints[2 * g], y = (double)keypoints[2 * g + 1];      // FeatureKeypointsToPointsVector
  double p[kCamStride];
#pragma unroll
  for (int j = 0; j < kCamStride; ++j) p[j] = intr[(int64_t)q.camera * kCamStride + j];
  double u, v;
  int ran_all = 0;
  ImageToWorld(camera_model[q.camera], p, x, y, &u, &v, &ran_all);
  const bool aligned = q.num_aligned > 0 && has_gravity[tile.image] && LfAlignKey(q.state, i) <= threshold[tile.image];
  double d0, d1, d2;
  if (aligned) {
    d0 = gravity[3 * (int64_t)tile.image]; d1 = gravity[3 * (int64_t)tile.image + 1]; d2 = gravity[3 * (int64_t)tile.image + 2];
  } else {
    d0 = LfDraw(q.state, i, 0); d1 = LfDraw(q.state, i, 1); d2 = LfDraw(q.state, i, 2);
  }
  // d x (u, v, 1)
  const double lx = d1 - d2 * v, ly = d2 * u - d0, lz = d0 * v - d1 * u;
  const double head = sqrt(lx * lx + ly * ly);
  lines[3 * g] = lx / head; lines[3 * g + 1] = ly / head; lines[3 * g + 2] = lz / head;
  if (dirs) { dirs[3 * g] = d0; dirs[3 * g + 1] = d1; dirs[3 * g + 2] = d2; }
  const bool degenerate = !(head > 0.0) || !(head <= 1.7976931348623157e308);
  flags[g] = (uint8_t)((aligned ? 1 : 0) | (degenerate ? 2 : 0) | (ran_all ? 4 : 0));
}

}  // namespace ppsfm

using namespace ppsfm;

extern "C" {

void pp_line_features_options_default(pp_line_features_options* o) {
  if (!o) return;
  o->aligned_line_ratio = 0.5;      // feature/extraction.cc:160-162 ("TODO Make aligned line ratio a parameter")
  o->seed = 0;
}

int pp_line_features_from_keypoints(const pp_line_features_desc* desc, const pp_line_features_options* options, int device, double* lines_out,
                                    uint8_t* aligned_out, double* dirs_out, pp_line_features_report* report) try {
  const char* where = "pp_line_features_from_keypoints";
  PP_REQUIRE(desc && options && report, "%s: null argument", where);
  const int32_t I = desc->num_images, K = desc->num_cameras;
  PP_REQUIRE(I >= 0 && K >= 0 && desc->kp_start, "%s: bad argument", where);
  PP_REQUIRE(I == 0 || (desc->image_ids && desc->image_camera), "%s: null image arrays", where);
  PP_REQUIRE(K == 0 || (desc->camera_model && desc->intr), "%s: null camera arrays", where);
  bool any_gravity = false;
  for (int32_t k = 0; k < I && desc->has_gravity; ++k) any_gravity = any_gravity || desc->has_gravity[k];
  PP_REQUIRE(!any_gravity || desc->gravity, "%s: has_gravity without gravity", where);
  std::vector<int> num_params((size_t)K);
  for (int32_t c = 0; c < K; ++c) num_params[(size_t)c] = CameraNumParams(desc->camera_model[c]);
  const std::string wrong = LfValidate(I, K, desc->kp_start, desc->image_camera, desc->camera_model, num_params.data(), desc->intr, kCamStride,
                                       desc->has_gravity, desc->gravity, options->aligned_line_ratio);
  PP_REQUIRE(wrong.empty(), "%s: %s", where, wrong.c_str());
  const int64_t L = desc->kp_start[I];
  PP_REQUIRE(L == 0 || (desc->keypoints && lines_out && aligned_out), "%s: null keypoints or output", where);

  std::vector<LfImageDev> images((size_t)I);
  std::vector<LfTileDev> tiles;
  std::vector<int32_t> todo;
  std::vector<uint8_t> has_gravity((size_t)I, 0);
  std::vector<double> gravity(3 * (size_t)I, 0.0);
  int64_t without_gravity = 0;
  for (int32_t k = 0; k < I; ++k) {
    const int64_t N = desc->kp_start[k + 1] - desc->kp_start[k];
    const bool hg = desc->has_gravity && desc->has_gravity[k];
    has_gravity[(size_t)k] = hg;
    if (hg) std::copy(desc->gravity + 3 * (size_t)k, desc->gravity + 3 * (size_t)k + 3, gravity.begin() + 3 * (size_t)k);
    without_gravity += !hg;
    LfImageDev& q = images[(size_t)k];
    q.state = LfImageState(options->seed, desc->image_ids[k]);
    q.kp0 = desc->kp_start[k]; q.count = (int32_t)N; q.camera = desc->image_camera[k]; q.reserved_ = 0;
    q.num_aligned = hg ? (int32_t)LfAlignedCount(N, options->aligned_line_ratio) : 0;
    if (q.num_aligned > 0) todo.push_back(k);
    for (int64_t f = 0; f < N; f += kLfTile) tiles.push_back(LfTileDev{k, (int32_t)f});
  }

  PP_TRY(UseDevice(where, device));
  DeviceHandle call;      // the pool blocks, the stream and the events of this call
  PP_TRY(call.Open(device));
  hipStream_t s = call.stream;
  LfImageDev* d_images = nullptr;
  LfTileDev* d_tiles = nullptr;
  int32_t *d_todo = nullptr, *d_model = nullptr;
  uint64_t* d_thr = nullptr;
  float* d_kp = nullptr;
  double *d_intr = nullptr, *d_gravity = nullptr, *d_lines = nullptr, *d_dirs = nullptr;
  uint8_t *d_hg = nullptr, *d_flags = nullptr;
  PP_TRY(call.blocks.Put(&d_images, images.data(), images.size(), s, 1)); PP_TRY(call.blocks.Put(&d_tiles, tiles.data(), tiles.size(), s, 1));
  PP_TRY(call.blocks.Put(&d_todo, todo.data(), todo.size(), s, 1)); PP_TRY(call.blocks.Put(&d_model, desc->camera_model, (size_t)K, s, 1));
  PP_TRY(call.blocks.Put(&d_intr, desc->intr, (size_t)K * kCamStride, s, 1)); PP_TRY(call.blocks.Put(&d_kp, desc->keypoints, 2 * (size_t)L, s, 1));
  PP_TRY(call.blocks.Put(&d_hg, has_gravity.data(), has_gravity.size(), s, 1)); PP_TRY(call.blocks.Put(&d_gravity, gravity.data(), gravity.size(), s, 1));
  PP_TRY(call.blocks.Alloc(&d_thr, (size_t)std::max(I, 1))); PP_TRY(call.blocks.Alloc(&d_lines, 3 * (size_t)std::max<int64_t>(L, 1)));
  PP_TRY(call.blocks.Alloc(&d_flags, (size_t)std::max<int64_t>(L, 1)));
  if (dirs_out) PP_TRY(call.blocks.Alloc(&d_dirs, 3 * (size_t)std::max<int64_t>(L, 1)));
  PP_HIP_TRY(hipMemsetAsync(d_thr, 0, (size_t)std::max(I, 1) * sizeof(uint64_t), s));

  StreamTimer timer(call);
  PP_TRY(timer.Begin());
  if (!todo.empty())
    hipLaunchKernelGGL(k_lf_select, dim3((unsigned)todo.size()), dim3(kLfBlock), 0, s, (const int32_t*)d_todo, (const LfImageDev*)d_images, d_thr);
  if (!tiles.empty())
    hipLaunchKernelGGL(k_lf_lines, dim3(CeilDiv((int64_t)tiles.size(), kLfWaves)), dim3(kLfBlock), 0, s, (int32_t)tiles.size(), (const LfTileDev*)d_tiles,
                       (const LfImageDev*)d_images, (const uint64_t*)d_thr, (const float*)d_kp, (const int32_t*)d_model, (const double*)d_intr,
                       (const uint8_t*)d_hg, (const double*)d_gravity, d_lines, d_dirs, d_flags);
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(timer.End());
  std::vector<uint8_t> flags((size_t)L);
  PP_TRY(Download(lines_out, d_lines, 3 * (size_t)L, s));
  if (dirs_out) PP_TRY(Download(dirs_out, d_dirs, 3 * (size_t)L, s));
  PP_TRY(Download(flags.data(), d_flags, (size_t)L, s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  PP_TRY(timer.Add());

  std::memset(report, 0, sizeof(*report));
  for (int64_t l = 0; l < L; ++l) {
    const uint8_t f = flags[(size_t)l];
    aligned_out[l] = f & 1;
    report->num_aligned += f & 1; report->num_degenerate += (f >> 1) & 1; report->num_newton_exhausted += (f >> 2) & 1;
  }
  report->num_lines = L; report->num_images_without_gravity = without_gravity; report->device_ms = timer.ms;
  return PP_OK;
} PP_API_CATCH("pp_line_features_from_keypoints")

}  // extern "C"
