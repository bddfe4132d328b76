// csrc/ba_structure.hpp - the host stages of pp_ba_create - with no device and no library: built by tests/test_ba_structure_host.py with
// g++ -Wall -Wextra -fsanitize=address,undefined.  Reads cases from stdin, builds the Schur pair lists with a brute-force walk over the tracks (the
// definition test_host_pair_list_builder_against_a_brute_force_walk pins the library's builder to), runs the stages in pp_ba_create's order and prints
// every scalar and, for every array of BaStructure, its length and the 64-bit FNV-1a hash of its bytes.
//
// A case, as whitespace-separated tokens:
//   case NAME  C P K M  iterative nv_private  ba_sparse ba_intr_wide ba_chunked_pairs ba_chunk_xcd
//   obs_pose[M] obs_point[M] pose_camera[C] camera_model[K] cam_np[K]
//   then six optional arrays, each a 0 (absent) or a 1 followed by its values:
//   pose_const[C] tvec_const_mask[C] point_const[P] camera_const_mask[K] covisibility[C*C] new_of_old[C]
// Lines are (1, 0, (o mod 7) / 4).
#include <array>
#include <cinttypes>
#include <iostream>
#include <tuple>

#include "../privacy_preserving_sfm_amd/csrc/ba_structure.hpp"

using namespace ppsfm;

template <class T>
static void Digest(const char* name, const std::vector<T>& v) {
  uint64_t h = 1469598103934665603ull;
  const unsigned char* b = reinterpret_cast<const unsigned char*>(v.data());
  for (size_t i = 0; i < v.size() * sizeof(T); ++i) { h ^= b[i]; h *= 1099511628211ull; }
  std::printf("array %s %zu %016" PRIx64 "\n", name, v.size(), h);
}

template <class T>
static std::vector<T> ReadArray(size_t n) {
  std::vector<T> v(n);
  for (size_t i = 0; i < n; ++i) { long long x; std::cin >> x; v[i] = (T)x; }
  return v;
}
template <class T>
static bool ReadOptional(size_t n, std::vector<T>* v) {
  int present = 0;
  std::cin >> present;
  if (present) *v = ReadArray<T>(n);
  return present != 0;
}

// every pair of variable images (ci >= cj) that share a variable point: the (observation of ci, observation of cj) pairs in (oi, oj) order, lists in (ci, cj) order
static void BruteForcePairLists(BaStructure* st) {
  std::vector<std::array<int32_t, 4>> all;
  const int32_t* pose = st->obs_pose();
  for (int p = 0; p < st->P; ++p) {
    if (st->point_const[(size_t)p]) continue;
    for (int e = st->pt_start[(size_t)p]; e < st->pt_start[(size_t)p + 1]; ++e)
      for (int f = st->pt_start[(size_t)p]; f < st->pt_start[(size_t)p + 1]; ++f) {
        const int32_t oi = st->pt_obs[(size_t)e], oj = st->pt_obs[(size_t)f], ci = pose[oi], cj = pose[oj];
        if (e == f || st->list_const[(size_t)ci] || st->list_const[(size_t)cj] || cj > ci) continue;
        all.push_back({ci, cj, oi, oj});
      }
  }
  std::sort(all.begin(), all.end());
  for (size_t i = 0; i < all.size(); ++i) {
    if (i == 0 || all[i][0] != all[i - 1][0] || all[i][1] != all[i - 1][1]) { st->pair_start.push_back((int32_t)i); st->pair_ij.push_back(all[i][0]); st->pair_ij.push_back(all[i][1]); }
    st->pair_entries.push_back(all[i][2]); st->pair_entries.push_back(all[i][3]);
  }
  st->pair_start.push_back((int32_t)all.size());
  st->total_entries = (int64_t)all.size();
}

int main() {
  std::string word, name;
  while (std::cin >> word >> name) {
    if (word != "case") { std::fprintf(stderr, "expected `case`, got %s\n", word.c_str()); return 2; }
    pp_ba_problem_desc d;
    std::memset(&d, 0, sizeof(d));
    long long M = 0;
    int iterative = 0, nv_private = 0, sparse = 1, wide = 1, chunked = 1, chunk_xcd = 1;
    std::cin >> d.num_poses >> d.num_points >> d.num_cameras >> M >> iterative >> nv_private >> sparse >> wide >> chunked >> chunk_xcd;
    d.num_obs = M;
    const size_t C = (size_t)d.num_poses, P = (size_t)d.num_points, K = (size_t)d.num_cameras;
    const std::vector<int32_t> obs_pose = ReadArray<int32_t>((size_t)M), obs_point = ReadArray<int32_t>((size_t)M), pose_camera = ReadArray<int32_t>(C),
                               camera_model = ReadArray<int32_t>(K);
    BaStructure st;
    st.cam_np = ReadArray<int32_t>(K);
    std::vector<uint8_t> pose_const, tvec_mask, point_const, covis;
    std::vector<uint16_t> cam_mask;
    std::vector<double> lines(3 * (size_t)M);
    for (size_t o = 0; o < (size_t)M; ++o) { lines[3 * o] = 1.0; lines[3 * o + 1] = 0.0; lines[3 * o + 2] = 0.25 * (double)(o % 7); }
    d.lines = lines.data(); d.obs_pose = obs_pose.data(); d.obs_point = obs_point.data(); d.pose_camera = pose_camera.data(); d.camera_model = camera_model.data();
    if (ReadOptional(C, &pose_const)) d.pose_const = pose_const.data();
    if (ReadOptional(C, &tvec_mask)) d.tvec_const_mask = tvec_mask.data();
    if (ReadOptional(P, &point_const)) d.point_const = point_const.data();
    if (ReadOptional(K, &cam_mask)) d.camera_const_mask = cam_mask.data();
    if (ReadOptional(C * C, &covis)) d.covisibility = covis.data();
    if (ReadOptional(C, &st.new_of_old)) { st.old_of_new.resize(C); for (size_t c = 0; c < C; ++c) st.old_of_new[(size_t)st.new_of_old[c]] = (int32_t)c; }
    if (!std::cin) { std::fprintf(stderr, "case %s: short input\n", name.c_str()); return 2; }

    // the stages, in pp_ba_create's order
    st.d = &d; st.C = (int)C; st.P = (int)P; st.K = (int)K; st.M = M;
    st.iterative = iterative != 0;
    st.sw.ba_sparse = sparse != 0; st.sw.ba_intr_wide = wide != 0; st.sw.ba_chunked_pairs = chunked != 0; st.sw.ba_chunk_xcd = chunk_xcd != 0;
    st.intr = LayOutIntrinsics(st.C, st.K, d.pose_camera, st.cam_np.data(), d.camera_const_mask);
    st.n_red = 6 * st.C + st.intr.NI;
    BuildByPointLists(&st);
    ApplyImageOrder(&st, nv_private);
    const int64_t bound = st.iterative ? 0 : PairEntryBound(st.P, st.pt_start.data(), st.pt_obs.data(), st.obs_pose(), st.list_const.data(), st.point_const.data());
    if (st.iterative) st.pair_start.assign(1, 0);
    else BruteForcePairLists(&st);
    st.num_pairs = (int64_t)st.pair_start.size() - 1;
    const std::string refusal = BuildTileMap(&st);
    std::printf("case %s\n", name.c_str());
    if (!refusal.empty()) { std::printf("refused %s\nend\n", refusal.c_str()); continue; }
    CompletePairLists(&st);
    OrderPairLists(&st);
    ChunkPairLists(&st);
    BuildIntrinsicsLists(&st);

    const std::pair<const char*, long long> scalars[] = {
        {"iterative", st.iterative}, {"reordered", st.reordered()}, {"NI", st.intr.NI}, {"nv_widest", st.intr.nv_widest}, {"n_red", st.n_red},
        {"nv_private", st.nv_private}, {"intr_wide_nv", st.intr_wide_nv}, {"num_effective_pose_point", st.num_effective_pose_point}, {"pair_entry_bound", bound},
        {"num_entries", st.total_entries}, {"num_pairs", st.num_pairs}, {"num_nz_tiles", st.num_nz_tiles}, {"sparse_tiles", st.sparse_tiles},
        {"pairs_complete", st.pairs_complete}, {"pairs_chunked", st.pairs_chunked}, {"chunk_len", st.chunk_len}, {"small_num_chunks", st.small_num_chunks},
        {"gen_num_groups", st.gen.num_groups}, {"gen_num_pairs", (long long)(st.gen.pair.size() / 4)}, {"gen_num_chunks", (long long)(st.gen.chunk.size() / 3)}, {"gen_num_multi", (long long)st.gen.multi.size()},
        {"isum_num_chunks", (long long)(st.isum_chunk.size() / 3)}, {"kk_num_groups", st.kk.num_groups}};
    for (const auto& s : scalars) std::printf("scalar %s %lld\n", s.first, s.second);
    Digest("intr_off", st.intr.off); Digest("intr_nv", st.intr.nv); Digest("intr_col", st.intr.col);
    Digest("point_const", st.point_const); Digest("pt_start", st.pt_start); Digest("pt_obs", st.pt_obs);
    Digest("old_of_new", st.old_of_new); Digest("new_of_old", st.new_of_old);
    Digest("obs_pose", std::vector<int32_t>(st.obs_pose(), st.obs_pose() + M)); Digest("pose_camera", std::vector<int32_t>(st.pose_camera(), st.pose_camera() + C));
    Digest("spos", st.spos); Digest("la", st.la); Digest("lb", st.lb); Digest("lc", st.lc); Digest("obs_cam", st.obs_cam);
    Digest("pose_const", st.pose_const); Digest("tvec_mask", st.tvec_mask); Digest("list_const", st.list_const);
    Digest("pose_start", st.pose_start); Digest("pose_obs", st.pose_obs);
    Digest("pair_start", st.pair_start); Digest("pair_ij", st.pair_ij); Digest("pair_entries", st.pair_entries); Digest("tile_nz", st.tile_nz);
    Digest("small_chunk", st.small_chunk); Digest("small_pair_chunk", st.small_pair_chunk);
    Digest("cam_start", st.cam_start); Digest("cam_obs", st.cam_obs); Digest("isum_chunk", st.isum_chunk); Digest("isum_cam_chunk", st.isum_cam_chunk);
    Digest("gen_pair", st.gen.pair); Digest("gen_pair_chunk", st.gen.pair_chunk); Digest("gen_chunk", st.gen.chunk); Digest("gen_entries", st.gen.entries);
    Digest("gen_multi", st.gen.multi); Digest("gen_grp_start", st.gen_grp_start); Digest("gen_grp_obs", st.gen_grp_obs);
    Digest("kk_entries", st.kk.entries); Digest("kk_pair", st.kk.pair); Digest("kk_pair_chunk", st.kk.pair_chunk); Digest("kk_chunk", st.kk.chunk); Digest("kk_multi", st.kk.multi);
    std::printf("end\n");
  }
  return 0;
}
