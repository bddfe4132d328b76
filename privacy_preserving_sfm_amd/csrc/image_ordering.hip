// pp_ba_plan_ordering, and the image order of pp_ba_create bound to the library's plan cache.  The ordering itself is image_ordering.hpp (std-only).
#include "ba_impl.hpp"
#include "camera_models.hpp"
#include "image_ordering.hpp"

namespace ppsfm {

// the winner's plan, list and replay go through cholesky.hip's process-wide cache: the plan is warm when the handle's first solve asks for it (EnsureTaskList)
ImageOrdering ChooseImageOrdering(const pp_ba_problem_desc* d, int NI, const int32_t* cam_np, const Switches& sw, const uint64_t* graph_bits) {
  return ChooseImageOrdering(d, NI, cam_np, sw, graph_bits, [&sw](int Tt, const uint8_t* nz, int* chains) { return CholeskyChainSteps(Tt, nz, sw, chains); });
}

}  // namespace ppsfm

extern "C" int pp_ba_plan_ordering(const pp_ba_problem_desc* d, int32_t* old_of_new, int32_t* info) try {
  using namespace ppsfm;
  PP_REQUIRE(d && info && d->obs_pose && d->obs_point && d->pose_camera && d->camera_model, "pp_ba_plan_ordering: null argument");
  const int C = d->num_poses, P = d->num_points, K = d->num_cameras;
  PP_REQUIRE(C > 0 && P > 0 && K > 0 && d->num_obs > 0, "pp_ba_plan_ordering: empty problem (poses %d, points %d, cameras %d, obs %lld)", C, P, K, (long long)d->num_obs);      // (as pp_ba_create)
  for (int c = 0; c < C; ++c) PP_REQUIRE(d->pose_camera[c] >= 0 && d->pose_camera[c] < K, "pp_ba_plan_ordering: pose_camera[%d] out of range", c);
  for (int64_t o = 0; o < d->num_obs; ++o)
    PP_REQUIRE(d->obs_pose[o] >= 0 && d->obs_pose[o] < C && d->obs_point[o] >= 0 && d->obs_point[o] < P, "pp_ba_plan_ordering: observation %lld indexes out of range", (long long)o);
  PP_REQUIRE(d->ordering >= PP_ORDERING_DEFAULT && d->ordering <= PP_ORDERING_AUTO, "pp_ba_plan_ordering: unknown ordering %d", d->ordering);
  std::vector<int32_t> cam_np;
  for (int k = 0; k < K; ++k) cam_np.push_back(CameraNumParams(d->camera_model[k]));
  const int NI = LayOutIntrinsics(C, K, d->pose_camera, cam_np.data(), d->camera_const_mask).NI;
  const Switches sw = ReadSwitches();
  const ImageOrdering ord = ChooseImageOrdering(d, NI, cam_np.data(), sw);
  // the tile map of the order chosen -> chains and chain steps of its one-launch factorisation.  The columns are those of the descriptor's solver, whatever
  // PPSFM_BA_LINEAR_SOLVER says; the graph is the whole one (the ordering may have left early, or not looked at all): the observations' and the caller's matrix's
  const ReducedColumns cols(C, NI, WillIterate(d, LinearSolverSwitch::Descriptor) ? 0 : PrivateIntrinsicsColumns(d, cam_np.data(), sw.ba_intr_layout));
  std::vector<uint64_t> graph((size_t)C * BitWords(C), 0);
  FillFromObservations(d, cols.nv_private, 0, graph.data());
  if (d->covisibility) FillFromMatrix(d, cols.nv_private, graph.data());
  std::vector<uint8_t> nz;
  const int Tt = cols.Tt, nnz = TileMapOf(cols, AdjacencyOf(C, graph.data()), ord.new_of_old.empty() ? nullptr : ord.new_of_old.data(), &nz);
  const bool sparse_path = Tt >= 8 && BlockSparsePays(Tt, nnz);
  int chains = 1;
  const int steps = sparse_path ? CholeskyChainSteps(Tt, nz.data(), sw, &chains) : Tt;
  info[0] = ord.old_of_new.empty() ? 0 : 1; info[1] = ord.nnz_natural; info[2] = nnz; info[3] = chains; info[4] = steps; info[5] = Tt; info[6] = sparse_path ? 1 : 0; info[7] = NI;
  if (old_of_new) for (int c = 0; c < C; ++c) old_of_new[c] = ord.old_of_new.empty() ? c : ord.old_of_new[c];
  return PP_OK;
} PP_API_CATCH("pp_ba_plan_ordering")
