// The pp_ba_handle lifecycle: pp_ba_create runs the host stages of ba_structure.hpp with the device work between them (the co-visibility graph and the pair
// lists of large problems) and one upload at the end; pp_ba_destroy, the create profile, pp_ba_covisibility, the parameter transfers.  No kernel lives here.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "ba_impl.hpp"
#include "image_ordering.hpp"
#include "device_handle.hpp"
#include "camera_models.hpp"
using namespace ppsfm;

// ---- device allocation + upload: `st` onto the device, its counts into the handle.  arrays_on_device: the by-point lists, obs_pose / obs_point and the
// constant flags are there already (the device pair-list path put them up - also when the host builder took over).
static int UploadStructure(pp_ba_impl* h, BaStructure& st, bool arrays_on_device) {
  const pp_ba_problem_desc* d = st.d;
  const int64_t C = st.C, P = st.P, K = st.K, NI = st.intr.NI, M = st.M;
  hipStream_t s = h->stream;
  DeviceBlocks& B = h->blocks;
  h->num_pairs = st.num_pairs; h->num_entries = st.total_entries; h->pairs_chunked = st.pairs_chunked; h->small_num_chunks = st.small_num_chunks;
  h->sparse_tiles = st.sparse_tiles; h->num_nz_tiles = st.num_nz_tiles; h->pairs_complete = st.pairs_complete;
  h->gen_num_groups = st.gen.num_groups; h->gen_num_pairs = (int64_t)(st.gen.pair.size() / 4); h->gen_num_chunks = (int64_t)(st.gen.chunk.size() / 3);
  h->gen_num_multi = (int64_t)st.gen.multi.size(); h->isum_num_chunks = (int64_t)(st.isum_chunk.size() / 3);
  h->num_effective_pose_point = st.num_effective_pose_point; h->host_pose_const = st.pose_const;
  PP_TRY(B.Put(&h->la, st.la.data(), M, s)); PP_TRY(B.Put(&h->lb, st.lb.data(), M, s)); PP_TRY(B.Put(&h->lc, st.lc.data(), M, s));
  if (!arrays_on_device) { PP_TRY(B.Put(&h->obs_pose, st.obs_pose(), M, s)); PP_TRY(B.Put(&h->obs_point, d->obs_point, M, s)); }
  PP_TRY(B.Put(&h->obs_cam, st.obs_cam.data(), M, s));
  PP_TRY(B.Put(&h->pose_camera, st.pose_camera(), C, s)); PP_TRY(B.Put(&h->camera_model, d->camera_model, K, s));
  if (!arrays_on_device) {
    PP_TRY(B.Put(&h->pose_const, st.pose_const.data(), C, s)); PP_TRY(B.Put(&h->point_const, st.point_const.data(), P, s));
    PP_TRY(B.Put(&h->pt_start, st.pt_start.data(), P + 1, s)); PP_TRY(B.Put(&h->pt_obs, st.pt_obs.data(), M, s));
  }
  PP_TRY(B.Put(&h->tvec_mask, st.tvec_mask.data(), C, s));
  PP_TRY(B.Put(&h->pose_start, st.pose_start.data(), C + 1, s)); PP_TRY(B.Put(&h->pose_obs, st.pose_obs.data(), M, s));
  PP_TRY(B.Put(&h->pair_start, st.pair_start.data(), st.pair_start.size(), s)); PP_TRY(B.Put(&h->pair_ij, st.pair_ij.data(), st.pair_ij.size(), s, 2));
  if (!h->pair_entries) PP_TRY(B.Put(&h->pair_entries, st.pair_entries.data(), st.pair_entries.size(), s, 2));      // (built on the device: already there, and the handle's)
  PP_TRY(B.Alloc(&h->poses, (size_t)7 * C)); PP_TRY(B.Alloc(&h->points, (size_t)3 * P)); PP_TRY(B.Alloc(&h->intr, (size_t)kCamStride * K));
  PP_TRY(B.Alloc(&h->poses_c, (size_t)7 * C)); PP_TRY(B.Alloc(&h->points_c, (size_t)3 * P)); PP_TRY(B.Alloc(&h->intr_c, (size_t)kCamStride * K));
  PP_TRY(B.Put(&h->cam_np, st.cam_np.data(), K, s)); PP_HIP_TRY(hipStreamSynchronize(s));
  PP_TRY(B.Put(&h->intr_off, st.intr.off.data(), K, s)); PP_TRY(B.Put(&h->intr_nv, st.intr.nv.data(), K, s)); PP_TRY(B.Put(&h->intr_col, st.intr.col.data(), st.intr.col.size(), s));
  if (NI > 0) {
    PP_TRY(B.Put(&h->cam_start, st.cam_start.data(), K + 1, s)); PP_TRY(B.Put(&h->cam_obs, st.cam_obs.data(), M, s));
    PP_TRY(B.Put(&h->gen_pair, st.gen.pair.data(), st.gen.pair.size(), s, 4)); PP_TRY(B.Put(&h->gen_pair_chunk, st.gen.pair_chunk.data(), st.gen.pair_chunk.size(), s));
    PP_TRY(B.Put(&h->gen_chunk, st.gen.chunk.data(), st.gen.chunk.size(), s)); PP_TRY(B.Put(&h->gen_entries, st.gen.entries.data(), st.gen.entries.size(), s, 2));
    PP_TRY(B.Put(&h->gen_multi, st.gen.multi.data(), st.gen.multi.size(), s, 1));
    if (!st.iterative) {
      const DiagLists& kk = st.kk;
      h->kk_num_groups = kk.num_groups; h->kk_num_pairs = (int64_t)(kk.pair.size() / 4); h->kk_num_chunks = (int64_t)(kk.chunk.size() / 3); h->kk_num_multi = (int64_t)kk.multi.size();
      PP_TRY(B.Put(&h->kk_entries, kk.entries.data(), kk.entries.size(), s, 1)); PP_TRY(B.Put(&h->kk_pair, kk.pair.data(), kk.pair.size(), s, 1));
      PP_TRY(B.Put(&h->kk_pair_chunk, kk.pair_chunk.data(), kk.pair_chunk.size(), s, 1)); PP_TRY(B.Put(&h->kk_chunk, kk.chunk.data(), kk.chunk.size(), s, 1));
      PP_TRY(B.Put(&h->kk_multi, kk.multi.data(), kk.multi.size(), s, 1)); PP_TRY(B.Alloc(&h->kk_partial, 144 * std::max<size_t>((size_t)h->kk_num_chunks, 1)));
      PP_TRY(B.Put(&h->gen_grp_start, st.gen_grp_start.data(), st.gen_grp_start.size(), s, 1)); PP_TRY(B.Put(&h->gen_grp_obs, st.gen_grp_obs.data(), st.gen_grp_obs.size(), s, 1));
      PP_TRY(B.Alloc(&h->gen_L, 36 * std::max<size_t>((size_t)h->gen_num_groups, 1)));
    }
    PP_TRY(B.Put(&h->isum_chunk, st.isum_chunk.data(), st.isum_chunk.size(), s)); PP_TRY(B.Put(&h->isum_cam_chunk, st.isum_cam_chunk.data(), st.isum_cam_chunk.size(), s));
    PP_TRY(B.Alloc(&h->gen_partial, (size_t)std::max<int64_t>(h->gen_num_chunks, 1) * 144)); PP_TRY(B.Alloc(&h->isum_partial, (size_t)std::max<int64_t>(h->isum_num_chunks, 1) * 24));
    PP_TRY(B.Alloc(&h->cnI, (size_t)NI)); PP_TRY(B.Alloc(&h->JkS_intr, (size_t)M * 2 * kCamStride));
    PP_HIP_TRY(hipMemsetAsync(h->JkS_intr, 0, sizeof(double) * (size_t)M * 2 * kCamStride, s));      // (k_intr_prepare only ever writes a camera's variable columns)
  }
  PP_TRY(B.Alloc(&h->r, (size_t)2 * M)); PP_TRY(B.Alloc(&h->Jpoint, (size_t)6 * M));
  h->num_partials = CeilDiv(M, 256);
  h->partials_stride = std::max(std::max(h->num_partials, 4096), CeilDiv(4 * (int64_t)P, 256));      // (k_step_points: one partial per 64 points)
  PP_TRY(B.Alloc(&h->partials, 2 * (size_t)h->partials_stride));     // K1's cost partials, then the model-cost partials
  // the int32 flag words live in the last scalar slot (+ one more double), so ONE copy of kNumScalars doubles reads back the
  // scalars and the failure flag
  PP_TRY(B.Alloc(&h->scal, kNumScalars + 1));
  h->d_flag = reinterpret_cast<int32_t*>(h->scal + kNumScalars - 1);
  PP_TRY(B.AllocPinned(reinterpret_cast<void**>(&h->h_scal), sizeof(double) * 3 * kNumScalars));   // read-back + two evaluation slots
  std::memset(h->h_scal, 0, sizeof(double) * 3 * kNumScalars);     // the ticket slot starts at 0 = "no ticket"
  if (hipHostGetDevicePointer(reinterpret_cast<void**>(&h->h_scal_dev), h->h_scal, 0) != hipSuccess) { h->h_scal_dev = nullptr; (void)hipGetLastError(); }
  PP_HIP_TRY(hipMemsetAsync(h->scal, 0, sizeof(double) * (kNumScalars + 1), s));
  PP_TRY(B.Put(&h->spos, st.spos.data(), st.spos.size(), s, 1));
  if (st.pairs_chunked) {
    PP_TRY(B.Put(&h->small_chunk, st.small_chunk.data(), st.small_chunk.size(), s, 3)); PP_TRY(B.Put(&h->small_pair_chunk, st.small_pair_chunk.data(), st.small_pair_chunk.size(), s));
    PP_TRY(B.Alloc(&h->small_partials, 36 * std::max<size_t>((size_t)h->small_num_chunks, 1)));
  }
  PP_HIP_TRY(hipStreamSynchronize(s));  // host staging vectors die with `st`
  h->spos_host.swap(st.spos); h->tile_nz.swap(st.tile_nz);      // (what the handle keeps on the host)
  return PP_OK;
}

extern "C" {
int pp_ba_create(const pp_ba_problem_desc* d, int device, pp_ba_handle* out) try {
  PP_REQUIRE(d && out, "pp_ba_create: null argument");
  *out = nullptr;
  PP_REQUIRE(d->num_poses > 0 && d->num_points > 0 && d->num_cameras > 0 && d->num_obs > 0,
             "pp_ba_create: empty problem (poses %d, points %d, cameras %d, obs %lld)", d->num_poses, d->num_points,
             d->num_cameras, (long long)d->num_obs);
  PP_REQUIRE(d->lines && d->obs_pose && d->obs_point && d->pose_camera && d->camera_model, "pp_ba_create: null array");
  PP_REQUIRE(d->loss_type >= 0 && d->loss_type <= 2 && d->loss_scale >= 0, "pp_ba_create: bad loss");
  PP_REQUIRE(d->num_obs < (int64_t)1 << 31, "pp_ba_create: more than 2^31 observations");
  PP_REQUIRE(d->ordering >= PP_ORDERING_DEFAULT && d->ordering <= PP_ORDERING_AUTO, "pp_ba_create: unknown ordering %d", d->ordering);      // (every check of the descriptor comes before the device is touched)
  const int C = d->num_poses, P = d->num_points, K = d->num_cameras;
  const int64_t M = d->num_obs;
  PP_REQUIRE(K < (1 << 26), "pp_ba_create: too many intrinsics blocks");
  for (int k = 0; k < K; ++k) PP_REQUIRE(CameraNumParams(d->camera_model[k]) > 0, "pp_ba_create: unknown camera model %d", d->camera_model[k]);
  for (int c = 0; c < C; ++c) PP_REQUIRE(d->pose_camera[c] >= 0 && d->pose_camera[c] < K, "pp_ba_create: pose_camera[%d] out of range", c);
  for (int64_t o = 0; o < M; ++o) {
    PP_REQUIRE(d->obs_pose[o] >= 0 && d->obs_pose[o] < C && d->obs_point[o] >= 0 && d->obs_point[o] < P,
               "pp_ba_create: observation %lld indexes out of range", (long long)o);
    const double nrm = std::sqrt(d->lines[3 * o] * d->lines[3 * o] + d->lines[3 * o + 1] * d->lines[3 * o + 1]);
    // CHECK_NEAR(norm, 1.0, 1e-6) of the reference (cost_functions.h:51-52, bundle_adjustment.cc:373)
    PP_REQUIRE(std::fabs(nrm - 1.0) <= 1e-6, "pp_ba_create: line %lld is not normalised (|(a,b)| = %.9g)", (long long)o, nrm);
  }
  BaStructure st;
  st.d = d; st.C = C; st.P = P; st.K = K; st.M = M;
  for (int k = 0; k < K; ++k) st.cam_np.push_back(CameraNumParams(d->camera_model[k]));
  st.intr = LayOutIntrinsics(C, K, d->pose_camera, st.cam_np.data(), d->camera_const_mask);
  const int NI = st.intr.NI; st.n_red = 6 * C + NI;
  PP_TRY(UseDevice("pp_ba_create", device));

  const auto t_create0 = std::chrono::steady_clock::now();
  const ppsfm::Switches sw = ppsfm::ReadSwitches();      // (the handle's snapshot: nothing reads the environment after this)
  const bool create_dbg = sw.create_debug;      // (stderr: where the host time of this create goes)
  auto lap = [&, last = t_create0](const char* what) mutable {
    if (!create_dbg) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "ppsfm: create %-34s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
  };
  UnderConstruction<pp_ba_impl, pp_ba_destroy> guard{new pp_ba_impl()};      // (an error return or a std::bad_alloc of the host builders below: the handle's device memory goes back)
  pp_ba_impl* const h = guard.h;
  // (a handle whose order and tile structure come from the caller's co-visibility - the union over the shards of a point-sharded group - lays out the
  // exchanged system like every other rank that was given the same matrix: it may join a group renumbered and block-sparse)
  h->sw = sw;
  h->chol = CholeskyCreate(sw);
  h->structure_from_covisibility = d->covisibility != nullptr;
  h->device = device; h->C = C; h->P = P; h->K = K; h->M = M;
  h->loss_type = d->loss_type; h->loss_scale = d->loss_scale;
  h->NI = NI; h->n_red = st.n_red; h->intrinsics_variable = NI > 0;
  h->jcam_stride = std::max(2, (st.intr.nv_widest + 1) & ~1);
  // linear solver of the reduced camera system, chosen before the structure is built as BundleAdjuster::Solve does
  // (bundle_adjustment.cc:273-286): ITERATIVE_SCHUR above 1000 images.  PPSFM_BA_LINEAR_SOLVER=direct|iterative overrides (tools / tests).
  // Variable intrinsics ride along: their columns follow the pose columns in the conjugate-gradient vectors, their part of the operator is applied
  // from the per-observation intrinsics Jacobians, their diagonal blocks (the preconditioner's) are assembled from the (k, k) pair lists alone.
  const bool iterative = h->iterative = st.iterative = ppsfm::WillIterate(d, sw.ba_linear_solver);
  const int nv_private = iterative ? 0 : ppsfm::PrivateIntrinsicsColumns(d, st.cam_np.data(), sw.ba_intr_layout);
  st.sw = sw;
  PP_TRY(PoolStreamAcquire(&h->stream));
  PP_TRY(PoolEventAcquire(&h->ev0, true));
  PP_TRY(PoolEventAcquire(&h->ev1, true));
  hipStream_t s = h->stream;
  DeviceBlocks& B = h->blocks;
  lap("handle, stream, events");
  BuildByPointLists(&st);
  lap("CSR by point");
  // On the device when the problem is large enough to pay for the launches (pair_lists.hip): the by-point lists go up first - the co-visibility graph the
  // image order is chosen on comes from them (in the caller's numbering), then the Schur pair lists (in the order chosen).
  bool lists_on_device = !iterative && PairListsOnDeviceEligible(C, M, sw.ba_pair_lists);
  std::vector<uint64_t> graph_bits;
  double graph_ms = 0;
  if (lists_on_device) {
    PP_TRY(B.Alloc(&h->obs_pose, M)); PP_TRY(B.Put(&h->obs_point, d->obs_point, M, s)); PP_TRY(B.Alloc(&h->pose_const, C)); PP_TRY(B.Put(&h->point_const, st.point_const.data(), P, s));
    PP_TRY(B.Put(&h->pt_start, st.pt_start.data(), P + 1, s)); PP_TRY(B.Put(&h->pt_obs, st.pt_obs.data(), M, s));
    if (ppsfm::OrderingReadsObservations(d, NI, st.cam_np.data(), sw)) {
      const auto tg = std::chrono::steady_clock::now();
      std::vector<uint8_t> fixed(C, 0);
      for (int c = 0; c < C; ++c) fixed[c] = ppsfm::ImageIsFixed(nv_private, d->pose_const, c) ? 1 : 0;
      PP_TRY(Upload(h->obs_pose, d->obs_pose, M, s)); PP_TRY(Upload(h->pose_const, fixed.data(), C, s));
      PP_TRY(CoVisibilityOnDevice(C, M, h->pt_start, h->pt_obs, h->obs_pose, h->obs_point, h->pose_const, h->point_const, s, &graph_bits));
      graph_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tg).count();
      lap("co-visibility graph (device)");
    }
  }

  // the image order (ba_structure.hpp ApplyImageOrder says what it is) and the problem in it
  ppsfm::ImageOrdering ord = ppsfm::ChooseImageOrdering(d, NI, st.cam_np.data(), sw, graph_bits.empty() ? nullptr : graph_bits.data());
  const double ordering_ms = graph_ms + ord.plan_ms;
  st.old_of_new.swap(ord.old_of_new); st.new_of_old.swap(ord.new_of_old);
  lap("image order");
  h->pose_old_of_new = st.old_of_new; h->pose_new_of_old = st.new_of_old;
  h->nnz_tiles_natural = ord.nnz_natural; h->nnz_tiles_ordered = ord.nnz_ordered;
  ApplyImageOrder(&st, nv_private);
  h->spos_identity = st.nv_private == 0;
  h->intr_private_nv = st.nv_private;
  h->intr_wide_nv = st.intr_wide_nv;
  lap("line streams, CSR by image");

  // block-pair entry lists of the reduced camera matrix (lower triangle, variable poses/points only): for every pair of variable images (ci >= cj) that
  // share a variable point, the (observation of ci, observation of cj) pairs, lists in (ci, cj) order, a list's entries in (oi, oj) order.
  // Built per problem structure, i.e. once per BA call of an incremental mapper (src/sfm/incremental_mapper.cc:893-936): ROW BY ROW (round 5; rounds 1-4
  // walked the points twice through a C x C table of counters and sorted 16-byte entries - 7.6 ms of an 11 ms create at 500 images / 200k observations) -
  // image ci's observations in order, each with the other observers of its point: the row's counters are C ints (cache resident), the rows are independent
  // (a few host threads share them), and the entries come out in list order without a sort.
  const int64_t bound = iterative ? 0 : PairEntryBound(P, st.pt_start.data(), st.pt_obs.data(), st.obs_pose(), st.list_const.data(), st.point_const.data());
  if (bound >= ((int64_t)1 << 31) - 1) {
    SetLastError("pp_ba_create: %lld Schur pair entries (sum over points of track^2 / 2) exceed the 32-bit pair lists", (long long)bound);
    return PP_ERR_INVALID;
  }
  // The pair lists on the device (the by-point lists are there): the lists' 3 ints per list come back, the entries never leave the device.  A structure with a list too long for the device's per-list sort takes the host builder below.
  const bool arrays_on_device = lists_on_device;      // (the by-point lists, obs_pose / obs_point and the constant flags are on the device already - also when the host builder takes over below)
  if (lists_on_device) {
    PP_TRY(Upload(h->obs_pose, st.obs_pose(), M, s)); PP_TRY(Upload(h->pose_const, st.list_const.data(), C, s));      // (the order chosen)
    bool fallback = false;
    const int rc = BuildPairListsOnDevice(C, M, h->pt_start, h->pt_obs, h->obs_pose, h->obs_point, h->pose_const, h->point_const, s, &B, &h->pair_entries, &st.total_entries, &st.pair_start, &st.pair_ij, &fallback);
    if (rc && !fallback) return rc;
    if (fallback) { lists_on_device = false; st.total_entries = 0; st.pair_start.clear(); st.pair_ij.clear(); }
    if (st.nv_private > 0) PP_TRY(Upload(h->pose_const, st.pose_const.data(), C, s));      // (the handle's array says which POSES are constant)
  }
  if (!iterative && !lists_on_device) {      // (an iterative handle applies S from the records: no pair lists)
    // (pair_lists.hip BuildPairListsOnHost: buckets per row image + a counting sort per row, on a few host threads)
    BuildPairListsOnHost(C, P, M, st.pt_start.data(), st.pt_obs.data(), st.obs_pose(), st.list_const.data(), st.point_const.data(), 0, [&](const char* what) { lap(what); },
                         &st.total_entries, &st.pair_start, &st.pair_ij, &st.pair_entries);
  } else if (iterative) {
    st.pair_start.assign(1, 0);
  }
  lap("pair lists");
  st.num_pairs = (int64_t)st.pair_start.size() - 1;
  const auto t_create2 = std::chrono::steady_clock::now();
  const std::string refusal = BuildTileMap(&st);
  if (!refusal.empty()) { SetLastError("%s", refusal.c_str()); return PP_ERR_INVALID; }
  lap("tile map");
  CompletePairLists(&st);
  lap("empty lists of a complete system");
  OrderPairLists(&st);
  lap("lists by length and strip");
  ChunkPairLists(&st);
  BuildIntrinsicsLists(&st);
  lap("chunks, intrinsics lists");
  const auto t_create3 = std::chrono::steady_clock::now();
  PP_TRY(UploadStructure(h, st, arrays_on_device));
  {
    const auto t_create4 = std::chrono::steady_clock::now();
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    // (the image order: the graph's pass on the device + ChooseImageOrdering; the handle, the by-point lists and their upload count with the pair lists)
    h->create_ms[0] = ordering_ms; h->create_ms[1] = ms(t_create0, t_create2) - ordering_ms; h->create_ms[2] = ms(t_create2, t_create3);
    h->create_ms[3] = ms(t_create3, t_create4); h->create_ms[4] = 0; h->create_ms[5] = ms(t_create0, t_create4);
  }
  *out = guard.release();
  return PP_OK;
} PP_API_CATCH("pp_ba_create")

int pp_ba_destroy(pp_ba_handle h) try {
  if (!h) return PP_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);      // nothing of this handle is in flight when its blocks go back to the pool (resource_pool.hpp)
  CholeskyDestroy(h->chol);
  h->blocks.Release();
  h->mirrors.Release();
  for (int i = 0; i < 8; ++i) if (h->tev[i]) PoolEventRelease(h->tev[i], true);
  for (int i = 0; i < 2; ++i) if (h->tev_eval[i]) PoolEventRelease(h->tev_eval[i], true);
  if (h->ev_readback) PoolEventRelease(h->ev_readback, false);
  if (h->ev0) PoolEventRelease(h->ev0, true);
  if (h->ev1) PoolEventRelease(h->ev1, true);
  if (h->stream) PoolStreamRelease(h->stream);
  delete h;
  return PP_OK;
} PP_API_CATCH("pp_ba_destroy")

int pp_ba_get_create_profile(pp_ba_handle h, double* ms) try {
  PP_REQUIRE(h && ms, "pp_ba_get_create_profile: null argument");
  for (int i = 0; i < 6; ++i) ms[i] = h->create_ms[i];
  ms[4] = CholeskyPlanMs(h->chol);      // (the task plan is made with the solver buffers, at the first solve or attach)
  return PP_OK;
} PP_API_CATCH("pp_ba_get_create_profile")

int pp_ba_covisibility(const pp_ba_problem_desc* d, uint8_t* out) try {
  PP_REQUIRE(d && out && d->obs_pose && d->obs_point, "pp_ba_covisibility: null argument");
  const int C = d->num_poses, P = d->num_points;
  const int64_t M = d->num_obs;
  PP_REQUIRE(C > 0 && P > 0 && M >= 0, "pp_ba_covisibility: empty problem");
  std::vector<int32_t> cam_np;
  if (d->camera_const_mask) {      // (PrivateIntrinsicsColumns walks the cameras of the images: the same checks as pp_ba_create / pp_ba_plan_ordering)
    PP_REQUIRE(d->pose_camera && d->camera_model && d->num_cameras > 0, "pp_ba_covisibility: camera_const_mask without pose_camera / camera_model");
    for (int k = 0; k < d->num_cameras; ++k) { cam_np.push_back(CameraNumParams(d->camera_model[k])); PP_REQUIRE(cam_np[k] > 0, "pp_ba_covisibility: unknown camera model %d", d->camera_model[k]); }
    for (int c = 0; c < C; ++c) PP_REQUIRE(d->pose_camera[c] >= 0 && d->pose_camera[c] < d->num_cameras, "pp_ba_covisibility: pose_camera[%d] out of range", c);
  }
  for (int64_t o = 0; o < M; ++o)
    PP_REQUIRE(d->obs_pose[o] >= 0 && d->obs_pose[o] < C && d->obs_point[o] >= 0 && d->obs_point[o] < P, "pp_ba_covisibility: observation %lld indexes out of range", (long long)o);
  std::memset(out, 0, (size_t)C * C);
  // (intrinsics of its own beside the pose: every image has columns)
  const int nv_private = d->camera_const_mask ? ppsfm::PrivateIntrinsicsColumns(d, cam_np.data(), ppsfm::ReadSwitches().ba_intr_layout) : 0;
  std::vector<uint64_t> bits((size_t)C * ppsfm::BitWords(C), 0);
  ppsfm::FillFromObservations(d, nv_private, 0, bits.data());
  const ppsfm::Adjacency adj = ppsfm::AdjacencyOf(C, bits.data());
  for (int i = 0; i < C; ++i) for (int j : adj[i]) out[(size_t)i * C + j] = 1;
  return PP_OK;
} PP_API_CATCH("pp_ba_covisibility")

int pp_ba_set_parameters(pp_ba_handle h, const double* poses, const double* points, const double* intr) try {
  PP_REQUIRE(h, "pp_ba_set_parameters: null handle");
  PP_HIP_TRY(hipSetDevice(h->device));
  std::vector<double> staged;      // (the caller's image order -> the handle's)
  if (poses && !h->pose_new_of_old.empty()) {
    staged.resize((size_t)7 * h->C);
    for (int c = 0; c < h->C; ++c) std::memcpy(&staged[(size_t)7 * h->pose_new_of_old[c]], poses + (size_t)7 * c, 7 * sizeof(double));
    poses = staged.data();
  }
  if (poses && (int)h->host_pose_const.size() == h->C)
    for (int c = 0; c < h->C; ++c) {
      // "CostFunction assumes unit quaternions" (bundle_adjustment.cc:354-355: AddImageToProblem normalises first): the Jacobian on the rotation tangent of a
      // VARIABLE pose is exact for unit q only - a caller that skipped the normalisation is told so instead of being given other steps than Ceres'
      // (a constant pose only enters through the rotate-point polynomial, as in the reference; NaN passes and fails the solve as before)
      const double* q = poses + (size_t)7 * c;
      const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
      PP_REQUIRE(h->host_pose_const[c] || !(std::fabs(n2 - 1.0) > 1e-6),
                 "pp_ba_set_parameters: the quaternion of a variable pose is not of unit length (|q|^2 = %.9g at internal image %d); normalise it as "
                 "BundleAdjuster::AddImageToProblem does (Image::NormalizeQvec)", n2, c);
    }
  if (poses) { int rc = Upload(h->poses, poses, (size_t)7 * h->C, h->stream); if (rc) return rc; }
  if (points) { int rc = Upload(h->points, points, (size_t)3 * h->P, h->stream); if (rc) return rc; }
  if (intr) { int rc = Upload(h->intr, intr, (size_t)kCamStride * h->K, h->stream); if (rc) return rc; }
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  return PP_OK;
} PP_API_CATCH("pp_ba_set_parameters")

int pp_ba_get_parameters(pp_ba_handle h, double* poses, double* points, double* intr) try {
  PP_REQUIRE(h, "pp_ba_get_parameters: null handle");
  PP_HIP_TRY(hipSetDevice(h->device));
  std::vector<double> staged;
  const bool perm = poses && !h->pose_new_of_old.empty();
  if (perm) staged.resize((size_t)7 * h->C);
  if (poses) { int rc = Download(perm ? staged.data() : poses, h->poses, (size_t)7 * h->C, h->stream); if (rc) return rc; }
  if (points) { int rc = Download(points, h->points, (size_t)3 * h->P, h->stream); if (rc) return rc; }
  if (intr) { int rc = Download(intr, h->intr, (size_t)kCamStride * h->K, h->stream); if (rc) return rc; }
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  if (perm) for (int c = 0; c < h->C; ++c) std::memcpy(poses + (size_t)7 * c, &staged[(size_t)7 * h->pose_new_of_old[c]], 7 * sizeof(double));
  return PP_OK;
} PP_API_CATCH("pp_ba_get_parameters")

}  // extern "C"
