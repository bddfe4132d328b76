// Drives ppsfm::IterativeGlobalRefinement (ppsfm/ppsfm.hpp) once on the device: reads a flat scene from a text file (one number per line), prints the
// report and the final parameters.  Run by tests/test_gpu_cpp_global_refinement.py.
#include <cstdio>
#include <fstream>

#include "../ppsfm/ppsfm.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  auto I = [&]() { long long v; in >> v; return v; };
  auto D = [&]() { double v; in >> v; return v; };
  const int C = (int)I(), P = (int)I(), K = (int)I();
  const long long M = I();
  ppsfm::FlatReconstruction rec;
  for (long long i = 0; i < 3 * M; ++i) rec.lines.push_back(D());
  for (long long i = 0; i < M; ++i) rec.obs_pose.push_back((int32_t)I());
  for (long long i = 0; i < M; ++i) rec.obs_point.push_back((int32_t)I());
  for (int i = 0; i < C; ++i) rec.pose_camera.push_back((int32_t)I());
  for (int i = 0; i < K; ++i) rec.camera_model.push_back((int32_t)I());
  for (int i = 0; i < 7 * C; ++i) rec.poses.push_back(D());
  for (int i = 0; i < 3 * P; ++i) rec.points.push_back(D());
  for (int i = 0; i < PP_CAM_STRIDE * K; ++i) rec.intr.push_back(D());
  if (!in) return 3;
  rec.point_alive.assign(P, 1);
  rec.obs_aligned.assign((size_t)M, 0);
  for (long long i = 0; i < M; ++i) rec.obs_id.push_back(i);
  for (int k = 0; k < K; ++k) { rec.cam_size.push_back(1 << 30); rec.cam_size.push_back(1 << 30); }
  try {
    const ppsfm::GlobalRefinementReport rep = ppsfm::IterativeGlobalRefinement(&rec);
    std::printf("rounds %d\n", rep.num_rounds);
    for (int r = 0; r < rep.num_rounds; ++r) {
      std::printf("round %zu %.17g %d %d %zu\n", rep.num_filtered[r], rep.changed[r], rep.summaries[r].num_iterations, rep.summaries[r].termination, rep.point_deleted[r].size());
      std::printf("obs_deleted");
      for (long long id : rep.obs_deleted[r]) std::printf(" %lld", id);
      std::printf("\n");
    }
    std::printf("poses");
    for (double v : rec.poses) std::printf(" %.17g", v);
    std::printf("\nalive");
    for (uint8_t a : rec.point_alive) std::printf(" %d", (int)a);
    std::printf("\npoints");
    for (double v : rec.points) std::printf(" %.17g", v);
    std::printf("\nleft %zu\n", rec.ComputeNumObservations());
  } catch (const ppsfm::Error& e) {
    std::printf("error %d %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
