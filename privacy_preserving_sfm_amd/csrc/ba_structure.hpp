// The host stages of pp_ba_create (ba_create.hip) - everything that decides what the Schur and intrinsics kernels walk - as free functions over one plain
// record, BaStructure.  No device API: g++ -std=c++17 compiles it alone, tests/ba_structure_host_driver.cpp runs it under ASan/UBSan.  In pp_ba_create's order:
// LayOutIntrinsics | (device, handle) BuildByPointLists | (image order) ApplyImageOrder, PairEntryBound | (pair lists) BuildTileMap, CompletePairLists,
// OrderPairLists, ChunkPairLists | BuildIntrinsicsLists.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ppsfm_hip.h"
#include "chol_plan.hpp"
#include "switches.hpp"

namespace ppsfm {
constexpr int kCamStride = 12;     // doubles per intrinsics block (max kNumParams of the 11 models)
constexpr int kGenChunk = 32;      // list entries per chunk of a generic block pair (256: twelve lanes walked a chunk for ~200 us with one wavefront per CU)
constexpr int kIsumChunk = 2048;   // observations per chunk of a per-camera sum

// CSR of n items by key(i) in [0, nkeys): start[nkeys + 1], items[n] (a counting sort: keeps the items' order inside a group)
template <class Key>
inline void GroupByKey(int64_t n, int nkeys, Key key, std::vector<int32_t>* start, std::vector<int32_t>* items) {
  start->assign((size_t)nkeys + 1, 0); items->resize((size_t)n);
  int32_t *s = start->data(), *it = items->data();
  for (int64_t i = 0; i < n; ++i) s[key(i) + 1]++;
  for (int k = 0; k < nkeys; ++k) s[k + 1] += s[k];
  std::vector<int32_t> fill(start->begin(), start->end() - 1);
  for (int64_t i = 0; i < n; ++i) it[fill[(size_t)key(i)]++] = (int32_t)i;
}
// Eight runs src[start[x], start[x + 1]) dealt to the eight XCDs: run x is handled by the workgroups that land on XCD x (workgroups are dealt round-robin by
// blockIdx, the first of them lands on first_xcd; 40 items per workgroup), and a workgroup whose XCD's run is used up takes from the next run that is not.
// emit(item) in the order the workgroups take them.
template <class Emit>
inline void DealRunsToXcds(const int32_t* src, const int32_t* start, int first_xcd, Emit emit) {
  int32_t at[8];
  for (int x = 0; x < 8; ++x) at[x] = start[x];
  int64_t left = start[8] - start[0];
  for (size_t wg = 0; left > 0; ++wg) {
    int x = (int)((first_xcd + wg) & 7);
    for (int tries = 0; tries < 8 && at[x] >= start[x + 1]; ++tries) x = (x + 1) & 7;
    for (int k2 = 0; k2 < 40 && at[x] < start[x + 1]; ++k2, --left) emit(src[at[x]++]);
  }
}
// variable intrinsics: compact columns, block k at off[k] (oracle/bundle_adjustment.h BuildLayout; reference bundle_adjustment.cc:490-528: constant camera unless a refine flag is set,
// SubsetParameterization otherwise); col: K x kCamStride, -1 if constant; nv_widest: the most variable parameters any camera has (the row width of the solver's compact camera Jacobians)
struct IntrinsicsLayout { std::vector<int32_t> off, nv, col; int NI = 0, nv_widest = 0; };
inline IntrinsicsLayout LayOutIntrinsics(int C, int K, const int32_t* pose_camera, const int32_t* cam_np, const uint16_t* camera_const_mask) {
  IntrinsicsLayout L;
  L.off.assign((size_t)K, -1); L.nv.assign((size_t)K, 0); L.col.assign((size_t)K * kCamStride, -1);
  if (!camera_const_mask) return L;
  // a block is part of the problem if an image references it (the same on every rank of a point-sharded group,
  // whose shards hold different observations)
  std::vector<char> cam_used((size_t)K, 0);
  for (int c = 0; c < C; ++c) cam_used[(size_t)pose_camera[c]] = 1;
  for (int k = 0; k < K; ++k) {
    if (!cam_used[(size_t)k]) continue;
    int nv = 0;
    for (int j = 0; j < cam_np[k]; ++j) if (!((camera_const_mask[k] >> j) & 1)) L.col[(size_t)k * kCamStride + j] = nv++;
    if (nv > 0) { L.off[(size_t)k] = L.NI; L.nv[(size_t)k] = nv; L.NI += nv; }
    L.nv_widest = std::max(L.nv_widest, nv);
  }
  return L;
}
// the 32-bit bound on the Schur pair entries: the entry count grows with the SQUARE of the track lengths (a track of L variable observers gives L (L - 1) / 2
// entries, up to L (L - 1) when images repeat) while every offset into the lists is 32-bit: count in 64 bits first and refuse what does not fit
inline int64_t PairEntryBound(int P, const int32_t* pt_start, const int32_t* pt_obs, const int32_t* obs_pose, const uint8_t* list_const, const uint8_t* point_const) {
  int64_t bound = 0;
  for (int p = 0; p < P; ++p) {
    if (point_const[p]) continue;
    int64_t nv = 0;
    for (int e = pt_start[p]; e < pt_start[p + 1]; ++e) nv += list_const[obs_pose[pt_obs[e]]] ? 0 : 1;
    bound += nv * (nv - 1);               // (a track that sees ONE image nv times lists both orders of every pair)
  }
  return bound;
}
// block-pair lists of the intrinsics: of the diagonal blocks S_kk (BuildDiagonalLists: kk of a direct handle, gen of an iterative one) or the factored ones
struct DiagLists { std::vector<int32_t> entries, pair, pair_chunk, chunk, multi; int64_t num_groups = 0; };
struct BaStructure {
  // what the stages read: the caller's problem, the handle's switches and solver, the parameters per camera (CameraNumParams of camera_model)
  const pp_ba_problem_desc* d = nullptr;
  Switches sw;
  bool iterative = false, sparse_tiles = false, pairs_complete = false, pairs_chunked = false;
  int C = 0, P = 0, K = 0, n_red = 0;      // n_red: order of the reduced system = 6C + NI (= index of the rhs row)
  int64_t M = 0, total_entries = 0, num_pairs = 0;
  IntrinsicsLayout intr;
  // the internal image order (both empty = the caller's) and the problem in it (views of the caller's arrays when nothing moved)
  std::vector<int32_t> cam_np, pt_start, pt_obs, old_of_new, new_of_old, obs_pose_perm, pose_camera_perm;
  bool reordered() const { return !old_of_new.empty(); }
  const int32_t* obs_pose() const { return reordered() ? obs_pose_perm.data() : d->obs_pose; }
  const int32_t* pose_camera() const { return reordered() ? pose_camera_perm.data() : d->pose_camera; }
  int nv_private = 0, W6 = 6, intr_wide_nv = 0, num_effective_pose_point = 0;      // PrivateIntrinsicsColumns (0 on an iterative handle); columns per image; as pp_ba_impl's
  std::vector<double> la, lb, lc;
  std::vector<uint8_t> point_const, pose_const, tvec_mask, list_const, tile_nz;
  // the Schur pair lists: as the device or the host builder left them, then completed, ordered, cut into chunks
  std::vector<int32_t> spos, obs_cam, pose_start, pose_obs, pair_start, pair_ij, pair_entries, small_chunk, small_pair_chunk;
  int num_nz_tiles = 0, small_num_chunks = 0, chunk_len = 16;
  std::vector<int32_t> cam_start, cam_obs, isum_chunk, isum_cam_chunk, gen_grp_start, gen_grp_obs;      // variable intrinsics
  DiagLists gen, kk;      // gen_* of the handle; kk: the diagonal blocks' lists of a direct handle
};
// ---- the by-point lists (no image order in them) ---------------------------------------------------------------------------------------------------
inline void BuildByPointLists(BaStructure* st) {
  st->point_const.assign((size_t)st->P, 0);
  if (st->d->point_const) std::memcpy(st->point_const.data(), st->d->point_const, (size_t)st->P);
  GroupByKey(st->M, st->P, [obs_point = st->d->obs_point](int64_t o) { return obs_point[o]; }, &st->pt_start, &st->pt_obs);      // CSR by point
}

// ---- camera ordering of the reduced system (what Ceres' SPARSE_SCHUR does before it factorises, bundle_adjustment.cc:279-282) -------
// The images are renumbered INTERNALLY (pose index = position of its six columns in the reduced system) when that makes the tile
// structure of the factor sparser; every per-image input / output of the C ABI (pp_ba_set/get_parameters, pp_ba_reduced_system) is
// in the caller's order.  old_of_new empty = the caller's order.  nv_private: PrivateIntrinsicsColumns of the problem (0 on an iterative handle).
inline void ApplyImageOrder(BaStructure* st, int nv_private) {
  const pp_ba_problem_desc* d = st->d;
  const int C = st->C, M = (int)st->M;
  const int32_t* new_of_old = st->new_of_old.data();
  const bool reordered = st->reordered();
  auto to_internal = [&](const uint8_t* in, std::vector<uint8_t>* out) {      // a per-image flag array of the caller (may be null: zeros)
    out->assign((size_t)C, 0);
    for (int c = 0; in && c < C; ++c) (*out)[(size_t)(reordered ? new_of_old[c] : c)] = in[c];
  };
  if (reordered) {
    st->obs_pose_perm.resize((size_t)M); st->pose_camera_perm.resize((size_t)C);
    for (int o = 0; o < M; ++o) st->obs_pose_perm[(size_t)o] = new_of_old[d->obs_pose[o]];
    for (int c = 0; c < C; ++c) st->pose_camera_perm[(size_t)new_of_old[c]] = d->pose_camera[c];
  }
  const int32_t *in_obs_pose = st->obs_pose(), *in_pose_camera = st->pose_camera();
  // columns of the reduced system: the vectors' order (pose c at 6c, intrinsics block k at 6C + intr_off[k]) unless every image carries its own variable
  // intrinsics, which then sit beside its pose columns (image_ordering.hpp PrivateIntrinsicsColumns; internal image order)
  const int W6 = st->W6 = 6 + (st->nv_private = nv_private);
  // (PPSFM_BA_INTR_WIDE=0: the general block-pair lists (ba_intr.hip) also for per-image intrinsics - tests / comparisons)
  st->intr_wide_nv = (nv_private >= 2 && nv_private <= 8 && st->sw.ba_intr_wide) ? nv_private : 0;
  st->spos.resize((size_t)st->n_red);
  for (int v = 0; v < st->n_red; ++v) st->spos[(size_t)v] = v;
  if (nv_private)
    for (int i = 0; i < C; ++i) {
      const int k = in_pose_camera[i];
      for (int j = 0; j < 6; ++j) st->spos[(size_t)(6 * i + j)] = W6 * i + j;
      for (int j = 0; j < nv_private; ++j) st->spos[(size_t)(6 * C + st->intr.off[(size_t)k] + j)] = W6 * i + 6 + j;
    }
  st->la.resize((size_t)M); st->lb.resize((size_t)M); st->lc.resize((size_t)M);
  for (int o = 0; o < M; ++o) { st->la[(size_t)o] = d->lines[3 * o]; st->lb[(size_t)o] = d->lines[3 * o + 1]; st->lc[(size_t)o] = d->lines[3 * o + 2]; }
  st->obs_cam.resize((size_t)M);
  for (int o = 0; o < M; ++o) { const int k = in_pose_camera[in_obs_pose[o]]; st->obs_cam[(size_t)o] = (k << 4) | d->camera_model[k]; }
  to_internal(d->pose_const, &st->pose_const); to_internal(d->tvec_const_mask, &st->tvec_mask);
  // which images have columns in the reduced system at all: those with a variable pose - and every image when each carries variable intrinsics of its own
  // beside its pose columns (its block pairs with the images it shares points with exist whatever its pose is; the pose rows of a constant pose are zeros)
  st->list_const = nv_private > 0 ? std::vector<uint8_t>((size_t)C, 0) : st->pose_const;
  GroupByKey(M, C, [in_obs_pose](int64_t o) { return in_obs_pose[o]; }, &st->pose_start, &st->pose_obs);      // CSR by image
  // effective parameters (tangent dimensions of the variable blocks): fixed with the masks, reported by every solve
  int& neff = st->num_effective_pose_point = 0;
  for (int c = 0; c < C; ++c) if (!st->pose_const[(size_t)c]) neff += 6 - __builtin_popcount(st->tvec_mask[(size_t)c] & 7);
  for (int p = 0; p < st->P; ++p) if (!st->point_const[(size_t)p]) neff += 3;
}

// ---- the columns of the reduced camera system and its 64x64 tiles: the one place that knows ------------------------------------------------------
// W6 columns per image - its pose and, when every image carries nv_private variable intrinsics of its own (image_ordering.hpp PrivateIntrinsicsColumns),
// those beside it, coupled with the same images as the pose -, image at position p at W6 p; behind the images (tail0) the NI_tail columns of the shared
// intrinsics blocks, which couple with every image; then the right-hand side's row n_red.  Tt: tiles per side.
struct ReducedColumns {
  int nv_private, W6, tail0, NI_tail, n_red, Tt;
  ReducedColumns(int C, int NI, int nv) : nv_private(nv), W6(6 + nv), tail0(W6 * C), NI_tail(NI - nv * C), n_red(6 * C + NI), Tt((n_red + 1 + 63) / 64) {}
};
// an image whose pose is constant has no part in the reduced system - no node of the co-visibility graph, no pair lists - unless every image carries variable
// intrinsics of its own beside its pose columns (its block pairs with the images it shares points with exist whatever its pose is)
inline bool ImageIsFixed(int nv_private, const uint8_t* pose_const, int c) { return nv_private == 0 && pose_const && pose_const[c]; }
// the tiles (lower triangle of the Tt x Tt map nz) of the block pair of the images at positions pi and pj (pi == pj: the diagonal block); returns how many were new
inline int MarkImagePair(const ReducedColumns& rc, int pi, int pj, uint8_t* nz) {
  const int r0 = rc.W6 * std::max(pi, pj), c0 = rc.W6 * std::min(pi, pj);
  int marked = 0;
  for (int ti = r0 / 64; ti <= (r0 + rc.W6 - 1) / 64; ++ti)
    for (int tj = c0 / 64; tj <= (c0 + rc.W6 - 1) / 64; ++tj) if (tj <= ti && !nz[(size_t)ti * rc.Tt + tj]) { nz[(size_t)ti * rc.Tt + tj] = 1; ++marked; }
  return marked;
}
// the rows of the shared intrinsics (they couple with every image) and the right-hand side's row (without a tail: the row of n_red alone)
inline void MarkTailAndRhs(const ReducedColumns& rc, uint8_t* nz) {
  for (int ti = rc.tail0 / 64; ti <= rc.n_red / 64; ++ti) for (int tj = 0; tj <= ti; ++tj) nz[(size_t)ti * rc.Tt + tj] = 1;
}
// the block-sparse path takes a closed tile map when at most 0.7 of the lower triangle is in it (variable intrinsics: dense rows, the pose part keeps its structure - an arrow)
inline bool BlockSparsePays(int Tt, int nnz) { return (int64_t)nnz * 10 <= (int64_t)Tt * (Tt + 1) / 2 * 7; }

// Tile structure of the reduced camera system (64x64 tiles of its lower triangle): which tiles the co-visibility puts an
// entry in, closed under the fill-in of the factorisation.  When a good part of them stays empty (a sequence: images only
// share points with their neighbours) the assembly, the factorisation and the back substitution skip them - what the
// reference gets from Ceres' SPARSE_SCHUR above 50 images (src/optim/bundle_adjustment.cc:275-286).  PPSFM_BA_SPARSE=0 disables.
// Reads the pair lists as the builder left them; returns the refusal (pp_last_error's text) of a co-visibility matrix that is not the group's union, or "".
inline std::string BuildTileMap(BaStructure* st) {
  const pp_ba_problem_desc* d = st->d;
  const int C = st->C, nv_private = st->nv_private, reordered = st->reordered();
  const std::vector<int32_t>&pair_ij = st->pair_ij, &old_of_new = st->old_of_new, &new_of_old = st->new_of_old;
  const ReducedColumns rc(C, st->intr.NI, nv_private);
  std::vector<uint8_t> nz((size_t)rc.Tt * rc.Tt, 0);
  int64_t marked = 0;
  const int64_t image_rows = (rc.W6 * C - 1) / 64 + 1, all_tiles = image_rows * (image_rows + 1) / 2;      // the tiles the images' columns can reach
  for (int c = 0; c < C; ++c) marked += MarkImagePair(rc, c, c, nz.data());
  // (a dense co-visibility has every tile after a fraction of its 125 000 pairs: the walk stops there)
  for (size_t i = 0; i + 1 < pair_ij.size() && marked < all_tiles; i += 2) marked += MarkImagePair(rc, pair_ij[i], pair_ij[i + 1], nz.data());
  if (d->covisibility) {
    // a pair of THIS shard that the given matrix lacks: the matrix is not the group's union (stale, partial, another scene's) and the other ranks - who
    // only have the matrix - would lay out another tile map than this one: refuse here instead of exchanging differently sized systems later
    for (size_t i = 0; i + 1 < pair_ij.size(); i += 2) {
      const int oi = reordered ? old_of_new[(size_t)pair_ij[i]] : pair_ij[i], oj = reordered ? old_of_new[(size_t)pair_ij[i + 1]] : pair_ij[i + 1];
      if (oi != oj && !d->covisibility[(size_t)oi * C + oj] && !d->covisibility[(size_t)oj * C + oi]) {
        char msg[512];
        std::snprintf(msg, sizeof(msg), "pp_ba_create: images %d and %d share a point of this shard but pp_ba_problem_desc::covisibility has no entry for them - the matrix must be "
                      "the union over the group's shards (pp_ba_covisibility of every rank, element-wise MAX)", oi, oj);
        return msg;
      }
    }
    // (the union over a group's shards: tiles other ranks' points fill, in the internal order)
    for (int i = 1; i < C; ++i) {
      if (ImageIsFixed(nv_private, d->pose_const, i)) continue;
      const int ni = reordered ? new_of_old[(size_t)i] : i;
      for (int j = 0; j < i; ++j)
        if ((d->covisibility[(size_t)i * C + j] || d->covisibility[(size_t)j * C + i]) && !ImageIsFixed(nv_private, d->pose_const, j))
          MarkImagePair(rc, ni, reordered ? new_of_old[(size_t)j] : j, nz.data());
    }
  }
  MarkTailAndRhs(rc, nz.data());
  const int nnz = CloseTileMap(rc.Tt, nz.data());
  st->sparse_tiles = !st->iterative && st->sw.ba_sparse && rc.Tt >= 8 && BlockSparsePays(rc.Tt, nnz);
  st->tile_nz.swap(nz); st->num_nz_tiles = nnz;
  return std::string();
}

// the factorisation overwrites S with L, fill-in included, so a block of two variable poses that share no point must be
// cleared before every assembly: give it an EMPTY list (k_schur_pairs then stores zeros).  With every such block listed
// and no same-image pair (which accumulates into a diagonal block), k_schur_pairs stores instead of read-modify-write
// and S needs no per-iteration clear.
inline void CompletePairLists(BaStructure* st) {
  std::vector<int32_t>&pair_start = st->pair_start, &pair_ij = st->pair_ij;
  bool same = false;
  for (size_t i = 0; i + 1 < pair_ij.size(); i += 2) same = same || pair_ij[i] == pair_ij[i + 1];
  st->pairs_complete = !same && !st->sparse_tiles;      // (block-sparse: no empty lists; the non-zero tiles are cleared per assembly instead)
  if (!st->pairs_complete || st->num_pairs <= 0) return;
  std::vector<int32_t> var;      // the variable images, ascending
  for (int c = 0; c < st->C; ++c) if (!st->list_const[(size_t)c]) var.push_back(c);
  const size_t V = var.size(), npairs = V * (V - 1) / 2;
  std::vector<int32_t> start2(npairs + 1), ij2(2 * npairs);
  size_t src = 0, at = 0;
  const size_t np0 = (size_t)st->num_pairs;
  for (size_t a = 1; a < V; ++a) {
    const int ci = var[a];
    for (size_t b = 0; b < a; ++b, ++at) {
      const int cj = var[b];
      const bool hit = src < np0 && pair_ij[2 * src] == ci && pair_ij[2 * src + 1] == cj;
      start2[at] = src < np0 ? pair_start[src] : (int32_t)st->total_entries;      // (an empty list starts where the next non-empty one does)
      src += hit ? 1 : 0;
      ij2[2 * at] = ci; ij2[2 * at + 1] = cj;
    }
  }
  start2[npairs] = (int32_t)st->total_entries;
  // an empty list starts where the next non-empty one does, so consecutive differences are still the lengths
  pair_start.swap(start2); pair_ij.swap(ij2);
  st->num_pairs = (int64_t)pair_start.size() - 1;
}

// k_schur_pairs walks ten lists per wavefront in lock step: order the pairs by list length (longest first) so
// that the lists sharing a wavefront have equal lengths; pair_start becomes (first, last+1) per pair
inline void OrderPairLists(BaStructure* st) {
  std::vector<int32_t>&pair_start = st->pair_start, &pair_ij = st->pair_ij;
  const size_t np = (size_t)st->num_pairs;
  std::vector<int32_t> order, start, idx;
  int32_t max_len = 0;
  for (size_t i = 0; i < np; ++i) max_len = std::max(max_len, pair_start[i + 1] - pair_start[i]);
  GroupByKey((int64_t)np, max_len + 1, [&](int64_t i) { return max_len - (pair_start[(size_t)i + 1] - pair_start[(size_t)i]); }, &start, &order);      // by list length, longest first
  // L2 locality: pairs grouped by STRIPS of 8 column images (all rows), strip t handled by the workgroups that land on XCD
  // t % 8 (workgroups are dealt round-robin by blockIdx; 40 pairs per workgroup): the records of the strip's 8 images
  // (0.6 MB) stay in that XCD's 4 MB L2 while the row side streams through once.  Measured on cfg 3 (Schur phase = the two
  // prepare kernels + the gather, us): 16x16-image tiles in row-major order 97.2, in column-major order 93.8, strips of 8
  // or 4 images 89.1, of 16 images 94.7, of 32 images 98.3.  With the tiles the gather's L2 hit rate was 56 % of 7.8 M
  // requests and 4 M 64-byte requests went to the fabric (rocprofv3 TCC_HIT/MISS, TCC_EA0_RDREQ/WRREQ).
  if (np > 0) {
    // order is by length (desc); a stable counting sort by strip keeps that inside a strip, a second one by the strip's XCD keeps both inside a run
    const int ts = 3;
    auto strip_of = [&](int32_t id) { return pair_ij[2 * (size_t)id + 1] >> ts; };
    std::vector<int32_t> by_strip(np), by_xcd(np);
    GroupByKey((int64_t)np, (st->C >> ts) + 1, [&](int64_t i) { return strip_of(order[(size_t)i]); }, &start, &idx);
    for (size_t i = 0; i < np; ++i) by_strip[i] = order[(size_t)idx[i]];
    GroupByKey((int64_t)np, 8, [&](int64_t i) { return strip_of(by_strip[(size_t)i]) & 7; }, &start, &idx);
    for (size_t i = 0; i < np; ++i) by_xcd[i] = by_strip[(size_t)idx[i]];
    size_t out = 0;
    DealRunsToXcds(by_xcd.data(), start.data(), st->C & 7, [&](int32_t id) { order[out++] = id; });      // k_schur_blocks: the pair workgroups follow C per-image workgroups
  }
  std::vector<int32_t> range(2 * np), ij(2 * np);
  for (size_t i = 0; i < np; ++i) {
    range[2 * i] = pair_start[(size_t)order[i]]; range[2 * i + 1] = pair_start[(size_t)order[i] + 1];
    ij[2 * i] = pair_ij[2 * (size_t)order[i]]; ij[2 * i + 1] = pair_ij[2 * (size_t)order[i] + 1];
  }
  if (np == 0) range.assign(2, 0);
  pair_start.swap(range); pair_ij.swap(ij);
}

// ---- the pair lists in chunks (long lists) ----------------------------------------------
// A pair list is walked entry by entry with a dependent gather each (~0.7 us): lists of more than 64 entries are always cut into chunks of 16
// (deterministic partial blocks + one reduction); a problem too small to fill the chip (the mapper's local bundle adjustment: 20 images /
// 2000 observations walk 40-entry lists for 26 us with 3 % of the lanes) cuts lists of more than 12 entries into chunks of 8.
inline void ChunkPairLists(BaStructure* st) {
  std::vector<int32_t>&pair_start = st->pair_start, &pair_ij = st->pair_ij, &small_chunk = st->small_chunk, &small_pair_chunk = st->small_pair_chunk;
  const int C = st->C;
  const size_t np = (size_t)st->num_pairs;
  int32_t chunk_len = 16;      // (32 until the sequence scenes were measured: cfg-3 size, window 40 - lists of ~35 entries - Schur phase 105 us with 32, 95 with 16, 93 with 8, 98 with 4)
  int64_t longest = 0, total = 0;
  for (size_t i = 0; i < np; ++i) { const int64_t len = pair_start[2 * i + 1] - pair_start[2 * i]; longest = std::max(longest, len); total += len; }
  const bool latency_bound = total <= 65536 && longest > 12;
  st->pairs_chunked = !st->iterative && st->intr.NI == 0 && (longest > 64 || latency_bound) && st->sw.ba_chunked_pairs;
  if (latency_bound) chunk_len = 8;
  st->chunk_len = chunk_len;
  if (!st->pairs_chunked) return;
  small_pair_chunk.assign(np + 1, 0);
  size_t count = 0;
  for (size_t i = 0; i < np; ++i) count += (size_t)((pair_start[2 * i + 1] - pair_start[2 * i] + chunk_len - 1) / chunk_len);
  small_chunk.reserve(3 * count);
  for (size_t i = 0; i < np; ++i) {
    small_pair_chunk[i] = (int32_t)(small_chunk.size() / 3);
    for (int32_t e = pair_start[2 * i]; e < pair_start[2 * i + 1]; e += chunk_len) {
      small_chunk.push_back((int32_t)i); small_chunk.push_back(e); small_chunk.push_back(std::min(e + chunk_len, pair_start[2 * i + 1]));
    }
  }
  small_pair_chunk[np] = (int32_t)(small_chunk.size() / 3);
  st->small_num_chunks = (int)(small_chunk.size() / 3);
  // L2 locality of the chunk kernel.  k_schur_self_chunks gives a workgroup 40 CHUNKS, so the strip order above (made for 40 PAIRS per workgroup) no longer
  // lines a strip up with an XCD: at banded cfg 3 (lists of ~35 entries, three chunks each) a strip's pairs landed on three XCDs and every XCD read most
  // records - FETCH_SIZE 172 MB per launch against 38 MB of records, L2 hit rate 45 % (profiles/r06_band_pmc.json).  A sequence's pairs lie in a band:
  // the chunks are PROCESSED in the order of their pair's column image, cut into eight equal runs, run x on the workgroups that land on XCD x (dealt 40
  // chunks at a time, as the dispatcher deals workgroups) - an XCD then works through one contiguous range of column images with their partners (the next
  // window of row images) and a record is read by at most two XCDs.  A chunk keeps its id (entry 0 of its triple): its partial block is written where
  // k_schur_chunk_reduce expects it, so the sums and their bits are unchanged.  Small problems keep the natural order (nothing to gain below a few MB).
  const size_t nch = small_chunk.size() / 3;
  const bool xcd_order = nch >= 8 * 40 * 4 && st->sw.ba_chunk_xcd;
  // (entry 0 becomes the chunk's id = where its partial block goes; until then it is the chunk's pair: the row image is the minor key, the column image the major one)
  if (!xcd_order) { for (size_t q = 0; q < nch; ++q) small_chunk[3 * q] = (int32_t)q; return; }
  // by column image, then by row image, a pair's chunks in order: two stable counting sorts, the minor key first (a comparison sort with this
  // indirect key cost 1.5 ms of a 5.5 ms create at banded cfg 3 - a third more `structure` time than the whole round-5 create spent there)
  std::vector<int32_t> by_row, by_col(nch), start, idx;
  GroupByKey((int64_t)nch, C, [&](int64_t q) { return pair_ij[2 * (size_t)small_chunk[3 * (size_t)q]]; }, &start, &by_row);
  GroupByKey((int64_t)nch, C, [&](int64_t i) { return pair_ij[2 * (size_t)small_chunk[3 * (size_t)by_row[(size_t)i]] + 1]; }, &start, &idx);
  for (size_t q = 0; q < nch; ++q) by_col[q] = by_row[(size_t)idx[q]];
  std::vector<int32_t> out(3 * nch);
  size_t w = 0;
  const size_t per = (nch + 7) / 8;
  int32_t run[9];
  for (size_t x = 0; x <= 8; ++x) run[x] = (int32_t)std::min(nch, per * x);
  DealRunsToXcds(by_col.data(), run, C & 7, [&](int32_t q) {      // (the chunk workgroups follow C per-image workgroups)
    out[w++] = q; out[w++] = small_chunk[3 * (size_t)q + 1]; out[w++] = small_chunk[3 * (size_t)q + 2];
  });
  small_chunk.swap(out);
}

// the observations of every point taken with a variable camera, GROUPED by camera - the groups (p, k) of the intrinsics lists: in point order, a point's groups
// with cameras ascending, a group's observations in the by-point list's order: group g is camera cam[g] with the observations obs[start[g] .. start[g + 1])
inline void BuildPointCameraGroups(const BaStructure& st, std::vector<int32_t>* cam, std::vector<int32_t>* start, std::vector<int32_t>* obs) {
  const int32_t *in_obs_pose = st.obs_pose(), *in_pose_camera = st.pose_camera();
  std::vector<std::pair<int32_t, int32_t>> ko;      // (camera, observation) of one track
  for (int p = 0; p < st.P; ++p) {
    ko.clear();
    for (int e = st.pt_start[(size_t)p]; e < st.pt_start[(size_t)p + 1]; ++e) {
      const int32_t o = st.pt_obs[(size_t)e]; const int k = in_pose_camera[in_obs_pose[o]];
      if (st.intr.off[(size_t)k] >= 0) ko.push_back({k, o});
    }
    std::stable_sort(ko.begin(), ko.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    for (size_t a = 0; a < ko.size(); ++a) {
      if (a == 0 || ko[a].first != ko[a - 1].first) { cam->push_back(ko[a].first); start->push_back((int32_t)obs->size()); }
      obs->push_back(ko[a].second);
    }
  }
  start->push_back((int32_t)obs->size());
}

// The DIAGONAL blocks S_kk of the intrinsics (an iterative handle assembles nothing else - they are its preconditioner, everything else is applied
// from the records; a direct handle takes them out of the entry lists below).  They factor:
//   S_kk = sum_o J_k,o^T J_k,o - sum_{(p, k)} L R,  L = sum_{o in (p,k)} J_k,o^T T_o,  R = sum_{o in (p,k)} X_o^T J_k,o
// over the GROUPS (p, k) = the observations of point p taken with camera k - linear in the observations where the pair list of a shared
// camera is quadratic in the track lengths (k_intr_kk).  Groups sorted by camera, chunks of ~320 observations (a workgroup each), one pair per variable camera.
inline void BuildDiagonalLists(const BaStructure& st, const std::vector<int32_t>& grp_cam, const std::vector<int32_t>& grp_start, const std::vector<int32_t>& grp_obs, DiagLists& dl) {
  const int C = st.C, K = st.K;
  const std::vector<int32_t>&intr_off = st.intr.off, &intr_nv = st.intr.nv;
  const size_t G = grp_cam.size();
  std::vector<int32_t> first, order;      // the groups by camera (a camera's groups in point order)
  GroupByKey((int64_t)G, K, [&](int64_t g) { return grp_cam[(size_t)g]; }, &first, &order);
  auto size_of = [&](size_t g) { return grp_start[(size_t)order[g] + 1] - grp_start[(size_t)order[g]]; };
  dl.entries.assign(G + 1 + grp_obs.size(), 0);      // [group starts | observations by group]
  for (size_t g = 0, pos = 0; g < G; ++g) { dl.entries[g] = (int32_t)pos; for (int32_t e = 0; e < size_of(g); ++e) dl.entries[G + 1 + pos++] = grp_obs[(size_t)(grp_start[(size_t)order[g]] + e)]; dl.entries[g + 1] = (int32_t)pos; }
  dl.num_groups = (int64_t)G;
  dl.pair_chunk.push_back(0);
  for (int k = 0; k < K; ++k) {
    if (intr_off[(size_t)k] < 0) continue;
    const int pair_id = (int)(dl.pair.size() / 4);
    dl.pair.push_back(6 * C + intr_off[(size_t)k]); dl.pair.push_back(intr_nv[(size_t)k]); dl.pair.push_back(6 * C + intr_off[(size_t)k]); dl.pair.push_back(intr_nv[(size_t)k] | (1 << 8));
    size_t g = (size_t)first[(size_t)k], g0 = g; int64_t nobs = 0;
    for (; g < (size_t)first[(size_t)k + 1]; ++g) {
      nobs += size_of(g);
      if (nobs >= 320) { dl.chunk.push_back(pair_id); dl.chunk.push_back((int32_t)g0); dl.chunk.push_back((int32_t)(g + 1)); g0 = g + 1; nobs = 0; }
    }
    if (g0 < g) { dl.chunk.push_back(pair_id); dl.chunk.push_back((int32_t)g0); dl.chunk.push_back((int32_t)g); }
    dl.pair_chunk.push_back((int32_t)(dl.chunk.size() / 3));
  }
}
// the pairs that are not finished by their only chunk (none or several chunks): the reduce kernels' list
inline void ListMultiChunkPairs(DiagLists& dl) {
  for (size_t pr = 0; pr < dl.pair.size() / 4; ++pr) if (dl.pair_chunk[pr + 1] - dl.pair_chunk[pr] != 1) dl.multi.push_back((int32_t)pr);
}

// FACTORED entries.  The intrinsics rows of S are  S_AB = sum_o J_A,o^T J_B,o - sum_{(oi, oj) sharing a point} J_A,oi^T T_oi X_oj^T J_B,oj  with A
// an intrinsics block; the sum over oi does not depend on B or oj:  L_(p,A) = sum_{oi in (p,A)} J_A,oi^T T_oi  (n_v x 3, k_intr_L, per trial radius)
// over the GROUP (p, A) = the observations of point p taken with camera A.  An entry is (group, oj [, oj belongs to the group: the direct term
// rides on it]): sum_p (groups of p) x (observations of p) entries - linear in the track length for a camera shared by all images, where the
// (oi, oj) lists were quadratic (500 images, tracks of 8, one camera: 3.2 M -> 0.4 M entries); a camera per image keeps its count.
// Row block = the group's camera; column block = pose of oj (kind 0) or intrinsics of oj (kind 1, lower triangle k(oj) <= k(group); the diagonal
// pair takes every oj of the group = the full block).  A CONSTANT point has T = 0: only its direct terms are listed.
inline void BuildFactoredLists(BaStructure* st) {
  const int C = st->C, K = st->K;
  const int32_t *in_obs_pose = st->obs_pose(), *in_pose_camera = st->pose_camera();
  const std::vector<int32_t>&intr_off = st->intr.off, &intr_nv = st->intr.nv, &pt_start = st->pt_start, &pt_obs = st->pt_obs;
  std::vector<int32_t>&gen_pair = st->gen.pair, &gen_pair_chunk = st->gen.pair_chunk, &gen_chunk = st->gen.chunk, &gen_entries = st->gen.entries;
  struct GEntry { int64_t key; int32_t oi, oj; };      // oi = group, oj = observation | (member of the group) << 31
  std::vector<GEntry> ge;
  std::vector<int32_t> grp_cam;
  BuildPointCameraGroups(*st, &grp_cam, &st->gen_grp_start, &st->gen_grp_obs);
  for (size_t g = 0; g < grp_cam.size(); ++g) {
    const int ka = grp_cam[g], p = st->d->obs_point[st->gen_grp_obs[(size_t)st->gen_grp_start[g]]];
    for (int f = pt_start[(size_t)p]; f < pt_start[(size_t)p + 1]; ++f) {
      const int32_t oj = pt_obs[(size_t)f]; const int cj = in_obs_pose[oj]; const int kb = in_pose_camera[cj];
      const bool same = kb == ka;
      if (st->point_const[(size_t)p] && !same) continue;
      const int32_t code = oj | (same ? (int32_t)0x80000000 : 0);
      if (!st->pose_const[(size_t)cj]) ge.push_back({((int64_t)ka * 2 + 0) * (int64_t)(C + K) + cj, (int32_t)g, code});
      if (intr_off[(size_t)kb] >= 0 && kb < ka) ge.push_back({((int64_t)ka * 2 + 1) * (int64_t)(C + K) + kb, (int32_t)g, code});      // (kb == ka: the diagonal block, k_intr_kk's)
    }
  }
  st->gen.num_groups = (int64_t)grp_cam.size();
  // (the diagonal pairs - they carry the damping, also of a block without a local observation - are k_intr_kk's: BuildDiagonalLists lists every variable block)
  BuildDiagonalLists(*st, grp_cam, st->gen_grp_start, st->gen_grp_obs, st->kk); ListMultiChunkPairs(st->kk);
  std::sort(ge.begin(), ge.end(), [](const GEntry& a, const GEntry& b) {
    if (a.key != b.key) return a.key < b.key;
    if (a.oi != b.oi) return a.oi < b.oi;
    return a.oj < b.oj;
  });
  gen_entries.resize(2 * ge.size());
  gen_pair_chunk.push_back(0);
  size_t e = 0;
  while (e < ge.size()) {
    size_t f = e;
    while (f < ge.size() && ge[f].key == ge[e].key) ++f;
    const int64_t key = ge[e].key;
    const int col = (int)(key % (C + K)), kind = (int)((key / (C + K)) & 1), ka = (int)(key / (C + K) / 2);
    const int pair_id = (int)(gen_pair.size() / 4);
    gen_pair.push_back(6 * C + intr_off[(size_t)ka]); gen_pair.push_back(intr_nv[(size_t)ka]);
    if (kind == 0) { gen_pair.push_back(6 * col); gen_pair.push_back(6); }
    else { gen_pair.push_back(6 * C + intr_off[(size_t)col]); gen_pair.push_back(intr_nv[(size_t)col] | (1 << 8)); }
    for (size_t c0 = e; c0 < f; c0 += kGenChunk) { gen_chunk.push_back(pair_id); gen_chunk.push_back((int32_t)c0); gen_chunk.push_back((int32_t)std::min(c0 + kGenChunk, f)); }
    gen_pair_chunk.push_back((int32_t)(gen_chunk.size() / 3));
    for (size_t g = e; g < f; ++g) { gen_entries[2 * g] = ge[g].oi; gen_entries[2 * g + 1] = ge[g].oj; }
    e = f;
  }
}

// ---- variable intrinsics: CSR by intrinsics block, generic block-pair lists with chunks --------------------
inline void BuildIntrinsicsLists(BaStructure* st) {
  st->cam_start.assign((size_t)st->K + 1, 0);
  if (st->intr.NI <= 0) return;
  const int32_t *in_obs_pose = st->obs_pose(), *in_pose_camera = st->pose_camera();
  GroupByKey(st->M, st->K, [=](int64_t o) { return in_pose_camera[in_obs_pose[o]]; }, &st->cam_start, &st->cam_obs);
  st->isum_cam_chunk.push_back(0);
  for (int k = 0; k < st->K; ++k) {
    if (st->intr.off[(size_t)k] >= 0)
      for (int e = st->cam_start[(size_t)k]; e < st->cam_start[(size_t)k + 1]; e += kIsumChunk) { st->isum_chunk.push_back(k); st->isum_chunk.push_back(e); st->isum_chunk.push_back(std::min(e + kIsumChunk, st->cam_start[(size_t)k + 1])); }
    st->isum_cam_chunk.push_back((int32_t)(st->isum_chunk.size() / 3));
  }
  if (st->iterative) {
    std::vector<int32_t> cam, start, obs;
    BuildPointCameraGroups(*st, &cam, &start, &obs); BuildDiagonalLists(*st, cam, start, obs, st->gen);
  } else if (st->intr_wide_nv > 0) {
    // every image carries its own intrinsics beside its pose columns: its 6 + n_v columns are ONE block, assembled by the pose blocks' own gather over the
    // pair lists with wider rows (k_schur_wide_self / k_schur_wide_pairs, ba_schur.hip) - no lists of their own
    st->gen.pair_chunk.push_back(0);
  } else {
    BuildFactoredLists(st);
  }
  ListMultiChunkPairs(st->gen);
}

}  // namespace ppsfm
