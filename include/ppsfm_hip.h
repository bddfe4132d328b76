/* ppsfm_hip.h — C ABI of the MI355X (gfx950) line-feature bundle adjustment + P6L RANSAC hot path.
 *
 * This is the drop-in boundary.  The reference (colmap/privacy_preserving_sfm) has no
 * C ABI: its extension surface is three compile-time C++ concepts.  Each entry point below replaces
 * the arithmetic behind one of them; the ppsfm/ C++ headers and the privacy_preserving_sfm_amd ctypes module
 * are thin host mirrors of the reference interfaces on top of these functions.
 *
 * Conventions
 *   - POD only; caller owns every host buffer; a handle owns its device memory and one HIP stream.
 *   - every function returns 0 (PP_OK) or a negative error code and never aborts/throws across the
 *     boundary: every entry point is a function-try-block (csrc/common.hpp PP_API_CATCH) that turns
 *     a failed host allocation (bad_alloc / length_error) into PP_ERR_NOMEM and anything else into PP_ERR_INTERNAL;
 *     worker threads of the host builders hand their exceptions to the calling thread.
 *     pp_last_error() gives the message of the calling thread's last failure
 *     (the reference uses glog CHECK aborts: util/logging.h:43-59).
 *   - a handle is not re-entrant (one caller thread at a time); distinct handles may run concurrently.
 *   - all floating point is IEEE binary64, as in the reference.
 *   - quaternions are (w, x, y, z) (base/image.h:219), projection matrices 3x4 ROW-major.
 *   - camera models are identified by the reference's model ids 0..10 (base/camera_models.h:189-349);
 *     every intrinsics block occupies PP_CAM_STRIDE doubles, only the first kNumParams are used.
 *   - the optional PPSFM_* environment variables are read when a handle is created
 *     (pp_ba_create) or a stand-alone entry point starts (pp_ba_plan_ordering, pp_dense_cholesky_solve, ...);
 *     changing one later does not affect an existing handle.
 */
#ifndef PPSFM_HIP_H_
#define PPSFM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_OK 0
#define PP_ERR_INVALID (-1)    /* bad argument / inconsistent problem description            */
#define PP_ERR_HIP (-2)        /* a HIP runtime call failed (no device, out of memory, ...)  */
#define PP_ERR_NUMERIC (-3)    /* linear system not positive definite / non-finite values     */
#define PP_ERR_NOMEM (-4)      /* a HOST allocation failed (C++ bad_alloc / length_error) inside the library           */
#define PP_ERR_INTERNAL (-5)   /* any other C++ exception stopped at the boundary (a system_error from a worker
                                  thread, an exception thrown by a caller's callback, ...): pp_last_error() has what()  */

#define PP_CAM_STRIDE 12
#define PP_NUM_CAMERA_MODELS 11

const char* pp_last_error(void);
int pp_device_count(int* count);
/* Test hook of the exception containment: raises a C++ exception INSIDE a guarded entry point and returns what the boundary made of
 * it - kind 0 bad_alloc, 1 runtime_error, 2 a non-standard exception, 3 bad_alloc in a worker thread of a host builder,
 * 4 length_error of an over-sized vector, 5 system_error: PP_ERR_NOMEM for 0 / 3 / 4, PP_ERR_INTERNAL otherwise.  Host only. */
int pp_debug_raise(int kind);
/* Test hook of the library's exclusive scan (csrc/scan.hpp): the host arrays in0 (and in1, or both in1 and out1 null) of n >= 0 elements of
 * elem_bytes (4: int32, 8: int64) are uploaded, scanned on `device` by the call the stages make - both arrays side by side in one call - and
 * downloaded: out[i] = in[0] + ... + in[i - 1] for i <= n, so each out holds n + 1 elements, the total last. */
int pp_debug_exclusive_scan(int device, int elem_bytes, int64_t n, const void* in0, void* out0, const void* in1, void* out1);
/* number of intrinsic parameters of a camera model id (base/camera_models.h:189-349); -1 if unknown */
int pp_camera_num_params(int model_id);
/* pixel threshold -> normalised-plane threshold: BaseCameraModel::ImageToWorldThreshold
 * (base/camera_models.h:533-543), used for RANSACOptions::max_error (sfm/incremental_mapper.cc:673-675) */
int pp_camera_image_to_world_threshold(int model_id, const double* params, double threshold_px, double* out);
/* n pixels xy (n x 2) -> normalised coordinates uv (n x 2): every model's ImageToWorld (base/camera_models.h) - closed form for the pinhole models
 * and FOV (Undistortion, :1176-1210), BaseCameraModel::IterativeUndistortion (:547-588) restated for the others.  Host only, needs no device.
 * PP_ERR_INVALID for an unknown model or a null pointer. */
int pp_camera_image_to_world(int model_id, const double* params, int64_t n, const double* xy, double* uv);
/* the other direction, uv (n x 2) -> xy (n x 2): WorldToImage, the code the device evaluates residuals with, on the host */
int pp_camera_world_to_image(int model_id, const double* params, int64_t n, const double* uv, double* xy);

/* ======================================================================================== *
 *  Bundle adjustment                                                                        *
 *  replaces: BundleAdjuster::SetUp/Solve  (optim/bundle_adjustment.cc:260-542) and the      *
 *  ceres::Problem / ceres::Solve it drives, with the residual of base/cost_functions.h:46-191 *
 * ======================================================================================== */

enum { PP_LOSS_TRIVIAL = 0, PP_LOSS_SOFT_L1 = 1, PP_LOSS_CAUCHY = 2 }; /* bundle_adjustment.h:51-52 */

/* What BundleAdjuster::SetUp builds from Reconstruction + BundleAdjustmentConfig, flattened:
 * one entry per residual block (= one line observation that has a 3D point).                  */
typedef struct pp_ba_problem_desc {
  int32_t num_poses;    /* C images in the problem (config Images() plus out-of-config observers) */
  int32_t num_points;   /* P 3D points                                                           */
  int32_t num_cameras;  /* K intrinsics blocks                                                    */
  int32_t loss_type;    /* PP_LOSS_*  (BundleAdjustmentOptions::CreateLossFunction, .cc:55-70)    */
  int64_t num_obs;      /* M residual blocks                                                      */
  double loss_scale;
  const double* lines;          /* M x 3  FeatureLine::Line(): (a,b,c), a^2+b^2 = 1 (.cc:373)     */
  const int32_t* obs_pose;      /* M      image (pose) index of each observation                  */
  const int32_t* obs_point;     /* M      3D point index                                          */
  const int32_t* pose_camera;   /* C      Image::CameraId                                          */
  const int32_t* camera_model;  /* K      Camera::ModelId                                          */
  const uint8_t* pose_const;        /* C  1: constant pose -> ConstantPose functor (.cc:361-398, :470-486) */
  const uint8_t* tvec_const_mask;   /* C  bit i: tvec[i] constant, SubsetParameterization (.cc:426-432)   */
  const uint8_t* point_const;       /* P  1: SetParameterBlockConstant (.cc:530-542)                       */
  const uint16_t* camera_const_mask;/* K  bit i: intrinsic i constant; all bits of the model set =>
                                          block constant (.cc:490-528).  NULL => all constant.             */
  /* ceres::Solver::Options::linear_solver_type as BundleAdjuster::Solve picks it from the image count before it builds the
   * problem (.cc:273-286): PP_LINEAR_SOLVER_*.  AUTO applies the reference's rule to num_poses (> 1000 images:
   * ITERATIVE_SCHUR + SCHUR_JACOBI); the host mirrors pass the choice made from BundleAdjustmentConfig::NumImages().
   * The structure built at create depends on it (an iterative handle builds no pair lists and no N x N system).
   * NOTE (zero-initialised descriptors): AUTO is 0, so a caller with more than 1000 poses gets the iterative solver without asking -
   * inexact steps (eta), and pp_ba_reduced_system refuses such a handle; PP_LINEAR_SOLVER_DIRECT (or the environment override
   * PPSFM_BA_LINEAR_SOLVER=direct) requests the direct solve.  VARIABLE intrinsics (camera_const_mask) ride along on the iterative path: their
   * columns follow the pose columns in the conjugate-gradient vectors and get one preconditioner block per intrinsics block, as Ceres lays the
   * parameter blocks out; in a point-sharded group their rows ride in the same exchanges (6 C + NI doubles per product, the compact diagonal blocks and
   * right-hand-side rows once per LM iteration). */
  int32_t linear_solver;
  /* Order of the images' columns in the reduced camera system: PP_ORDERING_*.
   * DEFAULT (0, what a zero-initialised descriptor gets) and NATURAL (1): the caller's order.
   * AUTO (2): pp_ba_create may renumber the images INTERNALLY - what Ceres' SPARSE_SCHUR ordering does for the reference between 50 and 1000 images
   * (bundle_adjustment.cc:279-282): reverse Cuthill-McKee on the co-visibility graph when that removes at least a tenth of the factor's non-zero 64x64
   * tiles (a sequence scene whose image ids are not in capture order gets its block-banded system back), and a nested dissection - of that band, or of the
   * graph itself (clusters joined by a few images) - when the independent parts, factorised side by side, shorten the critical path of the factorisation
   * (pp_ba_get_structure: info[6], info[7]).  The solve is the same to rounding, not bit for bit, as in the caller's order.  Every per-image array of
   * this interface stays in the CALLER's order.  The host mirrors of BundleAdjuster (ppsfm/ppsfm.hpp, bundle_adjustment.py) pass AUTO, as the reference's
   * solver orders without being asked.
   * Point-sharded groups (pp_ba_set_allreduce / pp_ba_set_communicator): every rank must lay out the exchanged system the same way, and a rank only sees its
   * own shard's co-visibility.  A handle of a group therefore keeps the caller's order - or, with AUTO, takes its order and its tile structure from
   * `covisibility` below, which every rank of the group passes alike (the UNION over the shards).  The attach calls refuse a handle that renumbered its
   * images from its own shard (an error on every rank that does; make the request the same on all ranks). */
  int32_t ordering;
  /* Optional (NULL: derived from this descriptor's own observations): C x C bytes, row-major, non-zero where two images share a variable point (symmetric;
   * the diagonal is ignored).  Read by PP_ORDERING_AUTO for the order and by pp_ba_create for the tile structure of the reduced system: the ranks of a
   * point-sharded group pass the element-wise MAX of their pp_ba_covisibility matrices (one all-reduce of C x C bytes at create), which lets the group keep
   * the block-sparse, several-chain factorisation a whole sequence scene gets on one GPU. */
  const uint8_t* covisibility;
} pp_ba_problem_desc;
enum { PP_LINEAR_SOLVER_AUTO = 0, PP_LINEAR_SOLVER_DIRECT = 1, PP_LINEAR_SOLVER_ITERATIVE_SCHUR = 2 };
enum { PP_ORDERING_DEFAULT = 0, PP_ORDERING_NATURAL = 1, PP_ORDERING_AUTO = 2 };
enum { PP_MAX_NUM_IMAGES_DIRECT_SOLVER = 1000 };   /* kMaxNumImagesDirectSparseSolver, bundle_adjustment.cc:276 */

/* the fields of ceres::IterationSummary the LM loop has */
typedef struct pp_ba_iteration_summary {
  int32_t iteration;           /* 0 = initial evaluation */
  int32_t step_is_successful;  /* 1 for iteration 0 */
  double cost, cost_change, gradient_max_norm, step_norm, relative_decrease, trust_region_radius;
} pp_ba_iteration_summary;
/* return values of the callback = ceres::CallbackReturnType */
enum { PP_SOLVER_CONTINUE = 0, PP_SOLVER_ABORT = 1, PP_SOLVER_TERMINATE_SUCCESSFULLY = 2 };

/* ceres::Solver::Options fields the reference sets (bundle_adjustment.h:80-93,
 * controllers/incremental_mapper.cc:196-243) + the Ceres trust-region defaults it inherits. */
typedef struct pp_ba_options {
  int32_t max_num_iterations;                /* 100 */
  int32_t max_num_consecutive_invalid_steps; /* 10  */
  double function_tolerance;                 /* 0   */
  double gradient_tolerance;                 /* 0 (1.0 global BA, 10.0 local BA) */
  double parameter_tolerance;                /* 0   */
  double initial_trust_region_radius;        /* 1e4   */
  double max_trust_region_radius;            /* 1e16  */
  double min_trust_region_radius;            /* 1e-32 */
  double min_relative_decrease;              /* 1e-3  */
  double min_lm_diagonal;                    /* 1e-6  */
  double max_lm_diagonal;                    /* 1e32  */
  int32_t jacobi_scaling;                    /* 1 */
  int32_t phase_timings;                     /* 0; 1 = record HIP events between the phases of every iteration for
                                                pp_ba_get_timings (each record costs ~5 us of stream time) */
  int32_t max_linear_solver_iterations;      /* 200 (bundle_adjustment.h:87): cap of the conjugate-gradient loop of an iterative handle */
  int32_t reserved_;
  double eta;                                /* 1e-1 (Ceres default): forcing term of the inexact step = q tolerance of the CG loop */
  /* ceres::IterationCallback (Solver::Options::callbacks).  The reference registers one callback,
   * BundleAdjustmentIterationCallback (controllers/bundle_adjustment.cc:43-61, 87-88), which blocks while the
   * controller thread is paused and returns SOLVER_TERMINATE_SUCCESSFULLY once it was stopped.  Called on the caller's thread after every
   * iteration (iteration 0 = the initial evaluation) with the iteration's summary; with a callback set
   * the solver waits for the evaluation at an accepted point before calling (one extra host round trip per
   * iteration), so `cost` / `gradient_max_norm` are the values at the point just accepted.  NULL = none. */
  int32_t (*iteration_callback)(void* ctx, const pp_ba_iteration_summary* it);
  void* iteration_callback_ctx;
} pp_ba_options;
void pp_ba_options_default(pp_ba_options* o);

/* ceres::TerminationType; USER_FAILURE (callback returned PP_SOLVER_ABORT) is NOT a usable solution in Ceres
 * (Solver::Summary::IsSolutionUsable): the host mirrors do not copy the parameters back in that case. */
enum { PP_TERM_CONVERGENCE = 0, PP_TERM_NO_CONVERGENCE = 1, PP_TERM_FAILURE = 2, PP_TERM_USER_SUCCESS = 3, PP_TERM_USER_FAILURE = 4 };

/* the part of ceres::Solver::Summary the reference prints (bundle_adjustment.cc:544-598) */
typedef struct pp_ba_summary {
  double initial_cost, final_cost;
  int32_t num_successful_steps, num_unsuccessful_steps;
  int32_t termination;        /* PP_TERM_* */
  int32_t num_iterations;     /* successful + unsuccessful */
  int32_t num_residuals;      /* 2 M */
  int32_t num_effective_parameters;
  double total_time_s;        /* wall clock of pp_ba_solve, host side */
  double device_time_s;       /* HIP-event time of the LM loop */
  /* what solved the reduced camera system in the LAST iteration of this solve (Ceres prints linear_solver_type_used,
   * bundle_adjustment.cc:585-590): PP_LINSOLVE_* */
  int32_t linear_solver;
  /* one-launch factorisations of this HANDLE (all its solves so far) that ran into a bounded wait and were repeated with
   * per-column launches; after the first one the handle stays with per-column launches */
  int32_t cholesky_fallbacks;
  int32_t linear_solver_iterations;   /* PP_LINSOLVE_PCG: conjugate-gradient iterations summed over the LM iterations; 0 otherwise */
  int32_t reserved_;
} pp_ba_summary;
enum { PP_LINSOLVE_CHOLESKY_COLUMNS = 0,   /* dense Cholesky, one launch per block column */
       PP_LINSOLVE_CHOLESKY_TASKS = 1,     /* dense Cholesky, the whole factorisation in one launch */
       PP_LINSOLVE_CHOLESKY_SPARSE = 2,    /* block-sparse Cholesky: the one-launch factorisation over the non-zero tiles, a chain workgroup per independent
                                              sub-tree of the elimination tree (per-column launches over the tile lists above 128 block columns / as the fallback) */
       PP_LINSOLVE_PCG = 3 };              /* matrix-free conjugate gradients on the implicit Schur complement (ITERATIVE_SCHUR + SCHUR_JACOBI) */

typedef struct pp_ba_impl* pp_ba_handle;

/* Upload the static structure (observations, index lists, masks).  `device` is the HIP device
 * ordinal.  One handle per sub-model / per GPU.                                                    */
int pp_ba_create(const pp_ba_problem_desc* desc, int device, pp_ba_handle* out);
int pp_ba_destroy(pp_ba_handle h);
/* pp_ba_create / pp_ba_destroy sit in the mapper's inner loop (a new BundleAdjuster per registered image, sfm/incremental_mapper.cc:813-858): the
 * device blocks, pinned blocks, stream and events of a destroyed handle are kept (by size class, at most PPSFM_POOL_MAX_MB = 1024 MB of device memory
 * per process; 0 disables) and handed to the next one.  pp_pool_trim frees everything that is cached. */
int pp_pool_trim(void);
/* What the pool holds for this process: device blocks and pinned blocks handed out and not yet returned, device bytes cached for reuse (all devices).
 * Null outputs are skipped.  The pool tracks nothing when it is disabled: with PPSFM_POOL_MAX_MB=0 all three are zero. */
int pp_pool_stats(int64_t* live_device_blocks, int64_t* live_pinned_blocks, int64_t* cached_device_bytes);

/* parameter blocks: poses C x 7 (qw,qx,qy,qz,tx,ty,tz), points P x 3, intrinsics K x PP_CAM_STRIDE.
 * PRECONDITION: unit quaternions.  BundleAdjuster::AddImageToProblem normalises every image of the configuration before it hands the block to Ceres
 * ("CostFunction assumes unit quaternions", src/optim/bundle_adjustment.cc:354-355); a binding does the same on its side of the boundary (the host
 * mirrors do: BundleAdjuster.AddImageToProblem).  The residual is the rotate-point polynomial of q as given (no re-normalisation, as Ceres'
 * UnitQuaternionRotatePoint); the Jacobian on the rotation tangent is exact for unit q only - for a quaternion of length L it differs from Ceres'
 * jets by factors of L (tools/fuzz_line_eval.py measures this; the ambient 2x4 Jacobian of pp_ba_evaluate is exact for any q).  pp_ba_set_parameters
 * therefore returns PP_ERR_INVALID for a VARIABLE pose whose |q|^2 is off 1 by more than 1e-6; a constant pose is taken as given (it enters through the
 * polynomial only, and AddPointToProblem does not normalise the out-of-configuration observers either).  pp_ba_attach (device pointers) cannot look. */
int pp_ba_set_parameters(pp_ba_handle h, const double* poses, const double* points, const double* intr);
int pp_ba_get_parameters(pp_ba_handle h, double* poses, double* points, double* intr);

/* Batched ceres::CostFunction::Evaluate for all M residual blocks at the parameters currently on the
 * device (kernel K1).  Results stay on the device; any of the *_out host pointers may be NULL.
 *   jac_mode 0: J_pose is M x (2x6) = [d r / d rotation-tangent (3) | d r / d tvec (3)]   (local
 *               parameterisation already applied: J_q (2x4) * QuaternionParameterization plus-Jacobian)
 *   jac_mode 1: J_pose is M x (2x7) = [d r / d qvec (w,x,y,z) | d r / d tvec]  (what Ceres hands to
 *               Evaluate: jacobians[0] 2x4 and jacobians[1] 2x3 side by side)
 *   J_point M x (2x3), J_cam M x (2 x PP_CAM_STRIDE) (only if want_cam), residuals 2M (NOT loss-corrected),
 *   cost = 1/2 sum rho(|r|^2).
 */
int pp_ba_eval(pp_ba_handle h, int jac_mode, int want_cam, double* residuals_out, double* jpose_out,
               double* jpoint_out, double* jcam_out, double* cost_out);

/* The same evaluation for a ceres::EvaluationCallback adaptor (ppsfm/ceres_adaptor.hpp): the results are copied by DMA into
 * PINNED host mirrors owned by the handle and the caller gets pointers to them (valid until the next call on the handle);
 * each residual block's CostFunction::Evaluate then copies its own slice - no staging copy through pageable memory, no
 * per-call allocation.  want_jacobians = 0 (Ceres evaluates residuals alone at every trial point) runs the cost-only
 * variant of K1 and moves 16 B per observation instead of 236 B+.  Layouts as pp_ba_eval.                          */
int pp_ba_eval_host_view(pp_ba_handle h, int jac_mode, int want_cam, int want_jacobians, const double** residuals,
                         const double** jpose, const double** jpoint, const double** jcam, double* cost_out);

/* device-resident variant used by benchmarks:
 * runs K1 `repeat` times on the handle's stream without copying anything back; returns the
 * HIP-event time per launch in *ms_per_launch (may be NULL).                                  */
int pp_ba_eval_device(pp_ba_handle h, int jac_mode, int want_cam, int repeat, float* ms_per_launch);

/* ceres::Solve replacement: Levenberg-Marquardt with exact point-Schur elimination, everything on the
 * device; parameters are read from / left on the device (use set/get_parameters).                  */
int pp_ba_solve(pp_ba_handle h, const pp_ba_options* options, pp_ba_summary* summary);

/* per-iteration trace of the last pp_ba_solve: rows of 7 doubles
 * {cost, cost_change, gradient_max_norm, step_norm, relative_decrease, trust_region_radius, successful} */
int pp_ba_get_trace(pp_ba_handle h, double* trace, int32_t capacity_rows, int32_t* num_rows);
/* Structure of the reduced camera system as the handle factorises it: info[0] = 64x64 tiles in the lower triangle, info[1] = non-zero
 * tiles of the factor (fill-in included) in the caller's image order, info[2] = in the order the handle uses, info[3] = 1 if the images
 * were renumbered internally (pp_ba_problem_desc::ordering), info[4] = 1 if the block-sparse path is taken (outside a group),
 * info[5] = 1 for an iterative handle (no reduced system is formed), info[6] = chain workgroups of the one-launch factorisation (more than one: the
 * internal order is a nested dissection whose independent parts are factorised side by side), info[7] = block-column steps on its longest
 * dependency path (info[0]'s block-column count for one chain). */
int pp_ba_get_structure(pp_ba_handle h, int32_t* info /* 8 */);
/* Where the handle put the variable intrinsics: info[0] = their columns in the reduced system over all referenced cameras, info[1] = n_v > 0 when every
 * image owns a camera with the same even number n_v of variable parameters and those columns sit beside its pose columns (6 + n_v columns per image, no
 * tail), 0 when they follow the 6 C pose columns, info[2] = n_v when such an image's 6 + n_v columns are assembled as one block by the pose gather with
 * wider rows (n_v = 2, 4, 6, 8), 0 when the general block pairs assemble them, info[3] = row width of the compact camera Jacobians (the widest camera). */
int pp_ba_get_intrinsics_layout(pp_ba_handle h, int32_t* info /* 4 */);
/* The image order pp_ba_create would give this problem's reduced camera system, computed on the host alone (no device is touched: what the ordering tests
 * run without a GPU).  Only the structure fields of the descriptor are read (counts, obs_pose, obs_point, pose_camera, camera_model, the const masks,
 * linear_solver, ordering).  old_of_new (num_poses ints, may be NULL): the caller's index of the image at every internal position.  info[0] = 1 if the
 * images are renumbered, info[1] = non-zero tiles of the factor in the caller's order (-1: no candidate order was looked at, or the co-visibility turned out too dense for any
 * order to pay before it was complete), info[2] = in the order chosen,
 * info[3] / info[4] = chain workgroups / chain steps of its one-launch factorisation, info[5] = block columns, info[6] = 1 if the block-sparse path applies,
 * info[7] = variable intrinsics columns. */
int pp_ba_plan_ordering(const pp_ba_problem_desc* d, int32_t* old_of_new /* num_poses or NULL */, int32_t* info /* 8 */);
/* The Schur pair lists of the problem in the CALLER's image order, built by the library's HOST builder (the builder of small problems and the one the
 * device-built lists are tested against), host only: for every pair of variable images (ci >= cj) that share a variable point the (observation of ci,
 * observation of cj) pairs - pair_start (lists + 1 offsets), pair_ij (2 per list), pair_entries (2 per entry); NULL arrays are skipped, nothing is
 * written beyond the capacities.  threads: 0 = by size, otherwise that many host threads (what the sanitizer configuration runs: tests/test_host_sanitizers.py). */
int pp_ba_pair_lists_host(const pp_ba_problem_desc* d, int32_t threads, int64_t* num_lists, int64_t* num_entries, int32_t* pair_start, int32_t* pair_ij,
                          int32_t* pair_entries, int64_t capacity_lists, int64_t capacity_entries);
/* The co-visibility matrix of a descriptor's own observations (host only): out = C x C bytes, 1 where two variable images share a variable point.
 * A point-sharded group all-reduces (MAX) these at create and passes the result as pp_ba_problem_desc::covisibility. */
int pp_ba_covisibility(const pp_ba_problem_desc* d, uint8_t* out /* num_poses x num_poses */);
/* Host wall time of the pp_ba_create that made this handle, ms: [0] image ordering (co-visibility, candidate orders, their chain plans), [1] CSR and
 * Schur pair lists, [2] tile structure + the intrinsics lists, [3] device allocation + upload, [4] the factorisation's task plan (made with the solver
 * buffers, at the handle's first solve or attach: 0 before; a process-wide cache keyed on the tile map answers repeated structures), [5] total of [0]..[3].  The mapper builds a new BundleAdjuster per global
 * bundle adjustment (src/sfm/incremental_mapper.cc:893-936): this is what that costs here. */
int pp_ba_get_create_profile(pp_ba_handle h, double* ms /* 6 */);

/* The damped Jacobi-scaled reduced camera system at the current parameters for a given radius, as the
 * solver builds it (kernels K2/K3a): S is n x n row-major (n = 6 C + variable intrinsics, constant
 * columns are identity rows), rhs n.  For parity tests and for multi-GPU reduction. */
int pp_ba_reduced_system(pp_ba_handle h, const pp_ba_options* options, double radius, int32_t* n, double* S,
                         double* rhs, int64_t capacity);

/* Covariance blocks of poses and points at the handle's current parameters, from the factorised reduced camera system (the counterpart of
 * ceres::Covariance with apply_loss_function = true; the reference has none).
 *   H = J^T J, J the LOSS-CORRECTED Jacobian in the tangent coordinates of pp_ba_eval (jac_mode 0: 3 rotation-tangent + 3 tvec coordinates per pose, in that
 *   order); no Levenberg-Marquardt damping enters and the solver's Jacobi scaling is undone.  No sigma^2 factor is applied: the caller scales, as with Ceres.
 *   With the points eliminated, S = U - W V^-1 W^T:  Cov(pose i, pose j) = (S^-1)_ij,  Cov(point p) = V_p^-1 + (V_p^-1 W_p^T) S^-1 (W_p V_p^-1).
 *   Variable intrinsics stay in S, so the pose and point blocks are the correct marginals; the intrinsics' own blocks and the cross blocks (pose-point, point-point,
 *   pose-intrinsics) come from pp_ba_covariance_blocks below.
 * pose_i / pose_j (num_pose_pairs each) and point_ids (num_points) are indices in the CALLER's image and point order whatever order the handle uses inside.
 * pose_cov: num_pose_pairs x 36, block q row-major = Cov(delta_i, delta_j) (the block of (j, i) is its transpose); point_cov: num_points x 9.
 * Constant blocks follow Ceres' convention: a constant pose has zero rows and columns, a constant tvec component a zero row and column, a constant point a
 * zero 3 x 3 block.
 * The call has no side effects on the handle: parameters, Jacobi scale, the reduced system and the factor arrays of the solver are as before, and a
 * pp_ba_solve after it is bit-identical to one without it.  It works in device buffers of its own (the inverse factor is n^2 doubles: 72 MB at 500 images),
 * returned to the pool before it returns.  What it does overwrite is the handle's per-evaluation scratch, which every pp_ba_solve / pp_ba_eval /
 * pp_ba_reduced_system recomputes before reading: residuals and Jacobians, the U and V blocks, the gradients and the scaled gather records.
 * The factorisation runs on the launch path the handle has bound (per-column launches, one launch, block-sparse), except that a system of at most two
 * block columns (n <= 128), whose one-workgroup kernel keeps the factor on chip, is factorised by per-column launches that leave it in memory.
 * Errors: PP_ERR_INVALID for an index out of range (before any device work), for an iterative handle (no reduced system exists) and for a handle attached to
 * a group (it holds one shard of the points); PP_ERR_NUMERIC when the undamped system is not positive definite (a free gauge, a point seen along one
 * direction only) - the handle solves as usual afterwards.
 * info (may be NULL): n = order of the reduced system, path = PP_LINSOLVE_* of the factorisation, device_ms = HIP-event time of the whole device path. */
typedef struct pp_ba_covariance_info { int32_t n; int32_t path; double device_ms; double reserved[2]; } pp_ba_covariance_info;
int pp_ba_covariance(pp_ba_handle h, const pp_ba_options* options,
                     int32_t num_pose_pairs, const int32_t* pose_i, const int32_t* pose_j, double* pose_cov /* pairs x 36, row-major */,
                     int32_t num_points, const int32_t* point_ids, double* point_cov /* points x 9 */,
                     pp_ba_covariance_info* info /* may be NULL */);

/* The covariance block of ANY pair of parameter blocks (what ceres::Covariance::Compute takes as its list of block pairs): poses, the intrinsics
 * blocks and points, in any of the six combinations.  The same H, the same undamped factorisation, tangent coordinates, scaling (none: no sigma^2) and
 * side effects (none beyond the per-evaluation scratch; a pp_ba_solve after it is bit-identical) as pp_ba_covariance; with x = (c, p) the camera-side
 * columns (poses, variable intrinsics) and the points, Z = L^-1 of S = L L^T and Y_p = Z (W_p V_p^-1):
 *   Cov(c_a, c_b) = Z[:, a]^T Z[:, b],   Cov(c_a, point p) = -Z[:, a]^T Y_p,   Cov(point p, point q) = Y_p^T Y_q  (+ V_p^-1 when p == q).
 * blocks[q] = (kind_a, index_a, kind_b, index_b), indices in the CALLER's order: PP_COV_POSE an image (6 rows: 3 rotation-tangent, 3 tvec),
 * PP_COV_INTRINSICS a row of pp_ba_problem_desc's intrinsics array (12 rows: the block's parameter slots in parameter order), PP_COV_POINT a point
 * (3 rows).  out: block q is row-major w(a_q) x w(b_q) and starts at the sum of w(a) w(b) over the blocks before it; capacity = doubles out can hold.
 * Constant blocks follow pp_ba_covariance (a constant pose, tvec component or point: zero rows and columns); a constant intrinsics parameter, a slot
 * beyond the camera model's parameter count and a block with nothing variable have zero rows and columns too.
 * Errors: PP_ERR_INVALID, before any device work, for a NULL handle or options, an unknown kind, an index out of range and a capacity below the total;
 * for an iterative or a group-attached handle; PP_ERR_NUMERIC when the undamped system is not positive definite - the handle solves as usual afterwards.
 * num_blocks == 0: PP_OK, nothing is computed (info, when given, is zeroed).  Device memory beyond pp_ba_covariance's: the request and the output. */
enum { PP_COV_POSE = 0, PP_COV_INTRINSICS = 1, PP_COV_POINT = 2 };      /* widths 6, 12, 3 */
typedef struct pp_cov_block { int32_t kind_a, index_a, kind_b, index_b; } pp_cov_block;
int pp_ba_covariance_blocks(pp_ba_handle h, const pp_ba_options* options, int64_t num_blocks, const pp_cov_block* blocks,
                            double* out, int64_t capacity /* doubles */, pp_ba_covariance_info* info /* may be NULL */);

/* Multi-GPU hook: one BA whose POINTS (with their observations) are sharded across the
 * ranks of a group; poses/intrinsics are replicated.  Each rank creates its handle from its own shard
 * of the observations (same pose/point/camera index spaces, points it does not own simply have no
 * observation) and registers a reduction callback: `fn(ctx, device_ptr, count, op)` reduces `count`
 * doubles in place across the group (op PP_REDUCE_SUM / PP_REDUCE_MAX) on the handle's stream
 * semantics (the solver synchronises its stream before calling and expects the result to be visible
 * to later work on any stream when fn returns).  Per LM iteration the solver reduces: the per-pose
 * normal-equation blocks (42 doubles per pose), the reduced camera system S (lower triangle is what
 * matters) + rhs, and a handful of scalars.  rank 0 of the group adds the damping/diagonal terms.
 * NULL fn => single GPU.
 * ATTACHING IS COLLECTIVE (fn != NULL, group_size > 1): the call itself runs ONE reduction through fn - three doubles,
 * PP_REDUCE_MAX: whether any rank must refuse (a handle that renumbered its images from its own shard) and a hash of the
 * layout of the reduced system (image count, variable intrinsics, internal order, block-sparse tile map), so that the ranks
 * of a group fail TOGETHER (PP_ERR_INVALID everywhere) instead of one erroring while the others enter a collective, and a
 * group whose handles would exchange differently sized systems is refused before its first exchange.  Hence: every rank of
 * the group must make the call, each from its own thread / process (attaching the group's handles one after another from ONE
 * thread deadlocks in the callback's rendezvous), and fn must be ready for traffic at attach time, not only inside
 * pp_ba_solve.  A group of one rank and a detach (fn == NULL) exchange nothing.                                          */
enum { PP_REDUCE_SUM = 0, PP_REDUCE_MAX = 1 };
typedef int (*pp_allreduce_fn)(void* ctx, void* device_ptr, int64_t count, int32_t op);
int pp_ba_set_allreduce(pp_ba_handle h, pp_allreduce_fn fn, void* ctx, int32_t group_rank, int32_t group_size);

/* The same exchange as RCCL collectives inside the library (one process per GPU).  The ranks of ONE sub-model's group create a communicator from a shared 128-byte id
 * (rank 0 of the group calls pp_comm_unique_id and sends it to the others by any means: MPI, a socket, a file), then
 * every rank hands its communicator to its handle.  Per LM iteration the solver then issues on the handle's own stream,
 * without synchronising the host: ONE grouped all-reduce of the per-pose blocks U, g_c (+ intrinsics sums), ONE all-reduce of
 * the reduced system packed as its lower triangle + rhs row ((n+1)(n+2)/2 doubles: 36 MB at 500 images instead of the
 * 72 MB square), and ONE grouped all-reduce of the handful of scalars (cost, model cost change, |step|^2, |x|^2 as sums with
 * the replicated pose part counted on rank 0 only; gradient max norm as a max).  Every rank then factorises the (identical)
 * reduced system itself.  BASELINE configs[4]: 4 sub-models over 8 GPUs = 4 communicators of 2 ranks (bench.py --submodels 4).
 * librccl is loaded with dlopen on first use: pp_comm_* return PP_ERR_HIP where it is absent.                        */
#define PP_COMM_ID_BYTES 128
typedef struct pp_comm_impl* pp_comm_handle;
int pp_comm_unique_id(uint8_t* id /* PP_COMM_ID_BYTES */);
int pp_comm_create(const uint8_t* id, int32_t num_ranks, int32_t rank, int device, pp_comm_handle* out);
int pp_comm_destroy(pp_comm_handle c);
/* in-place all-reduce of `count` device doubles on the null stream, synchronous (set-up and tests; the solver uses its own stream) */
int pp_comm_allreduce(pp_comm_handle c, double* device_ptr, int64_t count, int32_t op);
/* NULL detaches.  The communicator must outlive the handle's solves; it replaces a pp_ba_set_allreduce callback.
 * COLLECTIVE like pp_ba_set_allreduce when comm has more than one rank: every rank of the communicator calls it (one
 * ncclAllReduce of three doubles on the null stream inside the call: the common refusal + the structure hash).        */
int pp_ba_set_communicator(pp_ba_handle h, pp_comm_handle comm);

/* The dense SPD solver of the reduced camera system on its own (kernel K3b: blocked fp64 Cholesky on
 * v_mfma_f64_16x16x4_f64 + triangular solves): solves A x = b for a symmetric positive definite n x n
 * row-major A (only the lower triangle is read).  repeat > 1 re-runs the device part for timing;
 * *ms_per_solve (may be NULL) receives the HIP-event time of one factorisation + solve: the MEDIAN
 * over the `repeat` solves (an untimed one precedes them).
 * Range: b travels through the factorisation as one more row of A whose own diagonal entry is the constant 1e100,
 * so ||L^-1 b||_2^2 (L the Cholesky factor; for an A with a unit-size diagonal about b' A^-1 b) must stay below 1e100:
 * beyond it that row's pivot turns non-positive and the call reports PP_ERR_NUMERIC for a positive definite A.
 * Inside it the constant never reaches x: scaling b by 2^k, or A by 4^k, scales x exactly (no clamp, no epsilon), as
 * long as nothing overflows or becomes subnormal.  A non-positive or non-finite pivot, or a NaN / Inf anywhere in
 * the lower triangle or in b, is reported as PP_ERR_NUMERIC ("not positive definite"); x is then unspecified.      */
int pp_dense_cholesky_solve(int32_t n, const double* A, const double* b, double* x, int device, int32_t repeat,
                            float* ms_per_solve);
/* The work list of the one-launch factorisation for `block_columns` 64-wide block columns (4 .. 128), in launch order: four
 * int32 per task - type (1 PrepX, 2 PrepD, 3 solve, 4 update), step k, a, b (solve: a = block row; update: a = I,
 * b = J | part << 8 | parts << 12 | target << 16 of super-tile (I,J)).  Host-only (no device needed): lets a test check that
 * the order is topological, i.e. that no workgroup waits for one dispatched after it.  *count receives the number of tasks;
 * tasks beyond `capacity` are not written.                                                                                  */
int pp_cholesky_task_list(int32_t block_columns, int32_t* tasks, int64_t capacity, int64_t* count);
/* The same for a BLOCK-SPARSE system: tile_nz = T x T bytes, non-zero 64x64 tiles of the lower triangle of the matrix (closed under the
 * fill-in of the factorisation here).  map_out (T x T bytes, may be NULL): the tile map the one-launch mode works with (fill-in + the
 * two sub-diagonals the chain owns).  tasks: rows of SEVEN ints {type, k, a, b, w0, w1, w2} - w0 / w1: the values the task's
 * panel counters must have reached, w2: the value of the row counter of the row it solves a tile of (which depend on the tasks that
 * exist; tests/test_cholesky_task_order.py replays them). */
int pp_cholesky_task_list_sparse(int32_t block_columns, const uint8_t* tile_nz, uint8_t* map_out, int32_t* tasks, int64_t capacity, int64_t* count);
/* The plan of the one-launch factorisation of a block-sparse system with SEVERAL CHAINS (a nested-dissection order: the independent sub-trees of the
 * elimination tree are factorised side by side, chol_plan.hpp "ChainRanges").  max_chains <= 0: as many as the structure has (at most 16).
 * tasks: rows of SIXTEEN ints {type, k, a, b, w0, w1, w2, flags, cidx, sidx, zsel, mask, slot[4]}; chains_out (49 ints, may be NULL): n, then {begin, end, post} per chain;
 * time_out / rho1_out (T ints each, may be NULL): the step at which a block column is eliminated and 1 + its rank in the elimination order;
 * *verified (may be NULL): 1 when the host replay finds every wait of the list met by an earlier task (what pp_ba_solve requires of a list of
 * several chains before it uses it).  tests/test_cholesky_task_order.py replays the arithmetic side. */
int pp_cholesky_task_plan(int32_t block_columns, const uint8_t* tile_nz, int32_t max_chains, uint8_t* map_out, int32_t* tasks, int64_t capacity,
                          int64_t* count, int32_t* chains_out, int32_t* time_out, int32_t* rho1_out, int32_t* verified);

/* timing breakdown of the last solve (HIP events, ms, averaged per call): index by PP_BA_T_* */
enum { PP_BA_T_EVAL = 0, PP_BA_T_REDUCE = 1, PP_BA_T_SCHUR = 2, PP_BA_T_CHOLESKY = 3, PP_BA_T_BACKSUB = 4,
       PP_BA_T_UPDATE_COST = 5, PP_BA_T_COUNT = 6 };
int pp_ba_get_timings(pp_ba_handle h, double* ms /* PP_BA_T_COUNT */, int32_t* calls /* PP_BA_T_COUNT */);

/* ---- filters the mapper runs after every bundle adjustment (on the parameters the handle currently holds) ----
 * replaces Reconstruction::FilterPoints3D (= FilterPoints3DWithLargeReprojectionError +
 * FilterPoints3DWithSmallTriangulationAngle, base/reconstruction.cc:425-439, 594-719) and
 * FilterObservationsWithNegativeDepth (:441-460); the track of a point = its observations in problem order.
 * Deletions are returned as masks (the reference calls DeletePoint3D / DeleteObservation):
 *   obs_deleted[o] = 1: observation o is removed (its point was deleted or its pixel line error > max_reproj_error,
 *   behind the camera or outside the image, base/projection.cc:153-203); point_deleted[p] = 1; point_error[p] = mean
 *   error of the surviving track (Point3D::SetError), -1 where not set.
 * obs_aligned M (FeatureLine::IsAligned; NULL = none aligned), cam_size K x 2 (width, height), point_subset P or NULL. */
typedef struct { double max_reproj_error; double min_tri_angle_deg; } pp_filter_options;
typedef struct { int64_t num_filtered; /* the reference's return value */ int64_t num_points_deleted, num_observations_deleted; } pp_filter_report;
int pp_ba_filter_points(pp_ba_handle h, const pp_filter_options* options, const uint8_t* obs_aligned, const int32_t* cam_size,
                        const uint8_t* point_subset, uint8_t* obs_deleted, uint8_t* point_deleted, double* point_error, pp_filter_report* report);
int pp_ba_filter_negative_depth(pp_ba_handle h, uint8_t* obs_negative /* M */, int64_t* num_filtered);

/* ======================================================================================== *
 *  Absolute pose from six 2D-line / 3D-point pairs, RANSAC                                  *
 *  replaces: RANSAC<P6LEstimator>::Estimate (optim/ransac.h:178-278) with                   *
 *  P6LEstimator::Estimate/Residuals (estimators/absolute_pose.cc:79-174), re3q3              *
 *  (lib/re3q3/re3q3/re3q3.h:16-200), ComputeSquaredLineReprojectionError                     *
 *  (estimators/utils.cc:40-89), InlierSupportMeasurer (optim/support_measurement.cc:36-60). *
 * ======================================================================================== */

typedef struct pp_pose_impl* pp_pose_handle;

/* X = lines2D (n x 3, FeatureLine::Line()), Y = points3D (n x 3), aligned (n, FeatureLine::IsAligned(),
 * may be NULL) are uploaded once and stay resident (the Estimator's X/Y of optim/ransac.h:178-180).   */
int pp_pose_create(int32_t n, const double* lines2D, const double* points3D, const uint8_t* aligned,
                   int device, pp_pose_handle* out);
int pp_pose_destroy(pp_pose_handle h);

/* P6LEstimator::Residuals for `num_models` 3x4 row-major models: residuals_out num_models x n
 * (squared normalised point-to-line distance, DBL_MAX behind the camera).  Bit-identical to the
 * reference arithmetic (no FMA contraction, IEEE division).                                       */
int pp_pose_residuals(pp_pose_handle h, int32_t num_models, const double* models, double* residuals_out);

/* InlierSupportMeasurer::Evaluate for a batch of models (kernel K4, one wavefront per model):
 * num_inliers[m] = #{r <= max_residual} (exact); residual_sum[m] = sum of inlier residuals in a
 * fixed tree order (deterministic; NOT the sequential order — see pp_pose_support_sequential).       */
int pp_pose_score(pp_pose_handle h, int32_t num_models, const double* models, double max_residual,
                  uint32_t* num_inliers, double* residual_sum);
/* the exact sequential-order residual_sum of support_measurement.cc:40-47 (one lane per model) */
int pp_pose_support_sequential(pp_pose_handle h, int32_t num_models, const double* models, double max_residual,
                               uint32_t* num_inliers, double* residual_sum);

/* P6LEstimator::Estimate for H six-tuples (kernel K5, one lane per hypothesis):
 * samples H x 6 indices into X/Y; models_out H x 8 x 12 (3x4 row-major), num_models_out H.
 * Roots are returned in ascending order of the eliminated variable.                               */
int pp_pose_p6l_batch(pp_pose_handle h, int64_t num_hyp, const uint32_t* samples, double* models_out,
                      int32_t* num_models_out);
/* stand-alone three-quadrics solver, one system per lane: coeffs H x 30 (3x10 row-major),
 * solutions H x 24 (3x8 row-major), num H                                                          */
int pp_re3q3_batch(int64_t num, const double* coeffs, double* solutions, int32_t* num_solutions, int device);

/* RANSACOptions (optim/ransac.h:47-76) */
typedef struct pp_ransac_options {
  double max_error;                  /* threshold on the UNSQUARED error; residuals are squared */
  double min_inlier_ratio;           /* 0.1  */
  double confidence;                 /* 0.99 */
  double dyn_num_trials_multiplier;  /* 3.0  */
  uint64_t min_num_trials;           /* 0    */
  uint64_t max_num_trials;           /* SIZE_MAX */
  uint32_t seed;                     /* PRNG seed: util/random.h:46 kDefaultPRNGSeed = 0 */
  uint32_t chunk_trials;             /* speculation width (trials solved+scored per launch), 0 = auto */
} pp_ransac_options;
void pp_ransac_options_default(pp_ransac_options* o);

/* RANSAC::Report (optim/ransac.h:82-99) */
typedef struct pp_ransac_report {
  int32_t success;
  int32_t best_model_index;   /* index of the winner among its trial's models (trace, not in the reference) */
  uint64_t num_trials;
  uint64_t num_inliers;       /* support.num_inliers */
  double residual_sum;        /* support.residual_sum, sequential order */
  double model[12];           /* 3x4 row-major */
  int64_t best_trial;         /* trial that produced the winner (trace) */
  uint64_t hypotheses_evaluated;  /* trials actually solved+scored on the device (>= num_trials: speculation) */
  uint64_t models_scored;
  double device_time_s, total_time_s;
} pp_ransac_report;

/* RANSAC<P6LEstimator, InlierSupportMeasurer, RandomSampler>::Estimate: the host draws the samples
 * (mt19937 + persistent partial Fisher-Yates, bit-compatible with optim/random_sampler.cc:43-62 on
 * libstdc++), the device solves and scores them in speculative chunks, the host replays the
 * sequential accept / adaptive-termination logic in trial order (optim/ransac.h:213-249), so that
 * num_trials, the winner and the inlier mask equal the sequential loop's.  inlier_mask: n bytes. */
int pp_pose_ransac(pp_pose_handle h, const pp_ransac_options* options, pp_ransac_report* report,
                   uint8_t* inlier_mask);

/* throughput form (BASELINE cfg 4): solve + score `num_hyp` pre-drawn six-tuples, keep only the best
 * (num_inliers, tree residual_sum) — no adaptive termination.  samples may be NULL: drawn on the host
 * with the RANSAC sampler from `seed`.                                                             */
int pp_pose_hypotheses(pp_pose_handle h, int64_t num_hyp, const uint32_t* samples, uint32_t seed,
                       double max_residual, pp_ransac_report* report);

/* scores of EVERY model of the last pp_pose_hypotheses call (they stay on the device; this copies them out):
 * num_models num_hyp, num_inliers / residual_sum num_hyp x 8 (entries >= num_models[h] are unspecified).  For tests
 * that re-derive the winner on the host at BASELINE cfg 4's full size; any pointer may be NULL.                */
int pp_pose_last_scores(pp_pose_handle h, int64_t num_hyp, int32_t* num_models, uint32_t* num_inliers, double* residual_sum);

/* the RandomSampler stream alone (host): first `count` k-subsets for total size n */
int pp_sampler_draw(uint32_t seed, uint32_t n, int32_t k, int64_t count, uint32_t* out);
/* RANSAC::ComputeNumTrials for kMinNumSamples = 6 (optim/ransac.h:158-176) */
uint64_t pp_ransac_compute_num_trials(uint64_t num_inliers, uint64_t num_samples, double confidence,
                                      double num_trials_multiplier);


/* ---- batched robust track triangulation (one LORANSAC per track, one GPU lane per track) --------------------------
 * replaces the per-track EstimateTriangulation calls of the incremental triangulator (estimators/triangulation.cc:111-149,
 * sfm/incremental_triangulator.cc:214, 536): LORANSAC<TriangulationEstimator, ..., CombinationSampler> (optim/loransac.h,
 * deterministic: the sampler enumerates the 3-combinations), TriangulateMultiViewPoint (base/triangulation.cc:41-57), cheirality
 * and minimum-triangulation-angle checks, squared angular (residual_type 0) or squared pixel (1) line residuals.
 * Track t = observations track_start[t] .. track_start[t+1]-1: line (a,b,c) seen in view obs_view[i].  Views: proj_matrices
 * V x (3x4 row-major), proj_centers V x 3, view_camera V; cameras: model id, intr K x PP_CAM_STRIDE, cam_size K x 2.
 * Out per track: success, xyz (3), num_trials; per observation: inlier mask (0 where the track failed).               */
typedef struct pp_triangulation_options {
  double min_tri_angle;      /* radians */
  int32_t residual_type;     /* 0 ANGULAR_ERROR (EstimateTriangulationOptions default), 1 REPROJECTION_ERROR */
  int32_t reserved;
  pp_ransac_options ransac;  /* max_error: radians resp. pixels (squared internally) */
} pp_triangulation_options;
int pp_triangulate_tracks(int device, int32_t num_tracks, const int32_t* track_start, const double* lines, const int32_t* obs_view,
                          int32_t num_views, const double* proj_matrices, const double* proj_centers, const int32_t* view_camera,
                          int32_t num_cameras, const int32_t* camera_model, const double* intr, const int32_t* cam_size,
                          const pp_triangulation_options* options, uint8_t* success, double* xyz, uint8_t* inlier_mask,
                          int32_t* num_trials, float* device_ms /* may be NULL */);

/* ======================================================================================== *
 *  Track completion and merging                                                              *
 *  replaces: IncrementalTriangulator::CompleteTracks / CompleteAllTracks / MergeTracks /     *
 *  MergeAllTracks (sfm/incremental_triangulator.cc:237-293) with Complete (:697-765) and      *
 *  Merge (:606-695), on CalculateSquaredLineReprojectionError (base/projection.cc:162-203).   *
 *  The device speculates (kernels K10a k_complete_tracks, K10b k_merge_candidates: one          *
 *  wavefront per point, on the state at the start of the call), the host replays the          *
 *  sequential decisions, as pp_pose_ransac does for RANSAC.                                   *
 *  POINT ORDER: the reference iterates an unordered_set, so its order is unspecified, and     *
 *  unlike the bundle adjustment the result depends on it.  Here it is ASCENDING POINT INDEX,  *
 *  for the whole-model form (point_subset NULL) and the subset form alike.                    *
 *  EXACTNESS: the result of a call equals the strictly sequential loop in that order - the    *
 *  same pairs in the same order, the same merges, new indices and counts - whatever the       *
 *  schedule of the device work.                                                               *
 * ======================================================================================== */

/* The state the triangulator reads, flattened.  Lines are numbered 0..L-1 over all images; a point's track lists line numbers. */
typedef struct pp_tracks_desc {
  int32_t num_images;    /* C */
  int32_t num_cameras;   /* K */
  int32_t num_points;    /* P */
  int32_t reserved_;
  int64_t num_lines;     /* L */
  int64_t num_corrs;     /* E = corr_start[L] */
  const double* poses;            /* C x 7 (qw,qx,qy,qz,tx,ty,tz); normalised inside, as Image::ProjectionMatrix does */
  const int32_t* pose_camera;     /* C */
  const int32_t* camera_model;    /* K, as pp_triangulate_tracks */
  const double* intr;             /* K x PP_CAM_STRIDE */
  const int32_t* cam_size;        /* K x 2 (width, height) */
  const uint8_t* camera_skip;     /* K  1: HasCameraBogusParams, decided once per camera on the host (:767-779); NULL = none */
  const uint8_t* image_registered;/* C  Image::IsRegistered; NULL = all */
  const double* lines;            /* L x 3 FeatureLine::Line(), a^2 + b^2 = 1 (projection.cc:166) */
  const int32_t* line_image;      /* L */
  const int32_t* line_point;      /* L  point of the line, -1 = free */
  const int32_t* corr_start;      /* L + 1: CSR of the correspondence graph over lines */
  const int32_t* corr_line;       /* E: the neighbours of each line in the order FindCorrespondences returns them */
  const double* points;           /* P x 3 */
  const int32_t* track_start;     /* P + 1: tracks as CSR, in track order; an empty track = the point does not exist */
  const int32_t* track_line;      /* track_start[P] */
} pp_tracks_desc;

/* IncrementalTriangulator::Options, the fields Complete and Merge read (incremental_triangulator.h:57-64) */
typedef struct pp_tracks_options {
  double merge_max_reproj_error;       /* 4.0 */
  double complete_max_reproj_error;    /* 4.0 */
  int32_t complete_max_transitivity;   /* 5 */
  int32_t reserved_;
} pp_tracks_options;
void pp_tracks_options_default(pp_tracks_options* o);

typedef struct pp_tracks_report {
  int64_t num_changed;           /* the reference's return value: completed observations / merged observations (rule of :684-689) */
  int64_t num_entries;           /* pairs (complete) / merges (merge) of this call; those beyond `capacity` are not written */
  int64_t candidates_evaluated;  /* line errors the device computed, speculation included; a point of `overflow_points` is walked twice (its
                                    aborted first pass and the second launch), and both walks are counted */
  int32_t conflict_replays;      /* complete: points whose walk the host redid because an earlier point took one of their lines */
  int32_t overflow_points;       /* complete: points whose closure outgrew the on-chip list and were finished by the second launch;
                                    merge: points whose candidate list did (their pairs are evaluated one by one) */
  int32_t fresh_pair_launches;   /* merge: pairs evaluated by a launch of their own (a merged point, a candidate changed since the speculation) */
  int32_t second_launches;       /* complete: launches of the global-memory list kernel */
  double device_ms;              /* HIP-event time of the speculative launches */
  double replay_ms;              /* host replay, fresh-pair launches included */
  double total_ms;
} pp_tracks_report;

typedef struct pp_tracks_impl* pp_tracks_handle;
/* Validates the descriptor (every index in range, tracks and line_point consistent: PP_ERR_INVALID before any device work), then uploads it.
 * The handle keeps the evolving state (line_point, points, tracks) on the host and re-uploads it at the start of each call. */
int pp_tracks_create(const pp_tracks_desc* desc, int device, pp_tracks_handle* out);
int pp_tracks_destroy(pp_tracks_handle h);
/* CompleteTracks (point_subset: P bytes over the CURRENT points, new ones included) / CompleteAllTracks (NULL).  added_point / added_line: the
 * (point, line) pairs in the order the reference appends them to the tracks. */
int pp_tracks_complete(pp_tracks_handle h, const pp_tracks_options* options, const uint8_t* point_subset, pp_tracks_report* report,
                       int32_t* added_point, int32_t* added_line, int64_t capacity);
/* MergeTracks / MergeAllTracks.  Merge q: points merged_a[q] (the one being visited) and merged_b[q] are deleted, merged_new[q] is created with the
 * next unused index (P, P + 1, ...: ++num_added_points3D_), the length-weighted mean position and track a followed by track b; the merged point is
 * visited at once (the recursion of :684).  A point's merge_trials_ live for one call. */
int pp_tracks_merge(pp_tracks_handle h, const pp_tracks_options* options, const uint8_t* point_subset, pp_tracks_report* report,
                    int32_t* merged_a, int32_t* merged_b, int32_t* merged_new, int64_t capacity);
/* The current state.  *num_points / *num_track_elements are always written; an array that is not NULL is filled: line_point L, points P' x 3,
 * deleted P' (1: merged away or never existed), track_start P' + 1, track_line; PP_ERR_INVALID when a capacity is too small for it. */
/* ERRORS of pp_tracks_complete / pp_tracks_merge: PP_ERR_INVALID (bad argument or options) leaves the handle as it was.  Any other error (PP_ERR_HIP from a
 * launch or a copy, PP_ERR_NOMEM, ...) can arrive in the middle of the host replay, when some pairs or merges have been applied to the handle's state and
 * others have not; `report` and the output arrays are then unspecified.  The handle is no longer the state the caller knows: destroy it and create a new one. */
int pp_tracks_get_state(pp_tracks_handle h, int32_t* num_points, int64_t* num_track_elements, int32_t* line_point, double* points,
                        uint8_t* deleted, int32_t* track_start, int32_t* track_line, int32_t point_capacity, int64_t element_capacity);

/* ---- TriangulateImage / CompleteImage on a pp_tracks_handle (kernels K11a k_image_find, K11b k_image_triangulate) --------------------------------
 * replaces IncrementalTriangulator::TriangulateImage (sfm/incremental_triangulator.cc:63-121: Find :426-466, Continue :563-604, Create :468-561) and
 * CompleteImage (:123-235), the two places where the reference creates 3D points, with FindTransitiveCorrespondences / IsTwoViewObservation
 * (base/correspondence_graph.cc:166-224, 252-263) and CalculateNormalizedLineAngularError (base/projection.cc:241-260).
 * The device speculates over ALL lines of the image on the state at the start of the call (one wavefront per line for the closure, the Continue
 * candidate and the create set; one lane per create set for the LORANSAC of pp_triangulate_tracks with Create's recursion in place); the host
 * visits the lines in ascending line index and applies the answers.  An answer holds only while no line it read (the line itself and its closure)
 * has changed line_point since the snapshot; otherwise the line is evaluated again on the current state by launches of its own.
 * EXACTNESS: the result of a call equals the strictly sequential loop, whatever the schedule of the device work.
 * EVENTS: the (point, line) pairs in the order the reference's Reconstruction receives them - one per AddObservation (a continue, a completion),
 * and for an AddPoint3D the elements of the new track in track order.  New points take the next unused indices P, P + 1, ... as pp_tracks_merge's
 * do; their positions are read with pp_tracks_get_state.  Events beyond `capacity` are not written (num_entries counts them all).
 * An unregistered image, or one whose camera is flagged in camera_skip, returns 0 changes.
 * CompleteImage keeps ONE options object over its loop (:142, :205-209): a set of more than 15 observations runs with the min_num_trials the last
 * shorter set left behind.  That is kept; a line whose speculation assumed another value is evaluated again.
 * ERRORS: as pp_tracks_complete / pp_tracks_merge (PP_ERR_INVALID leaves the handle as it was).                                              */
typedef struct pp_tracks_image_options {   /* IncrementalTriangulator::Options, incremental_triangulator.h:47-87 */
  double create_max_angle_error;     /* 2.0 degrees */
  double continue_max_angle_error;   /* 2.0 degrees */
  double complete_max_reproj_error;  /* 4.0 px */
  double min_angle;                  /* 1.5 degrees */
  int32_t max_transitivity;          /* 1 */
  int32_t complete_max_transitivity; /* 5 */
  int32_t ignore_two_view_tracks;    /* 1 */
  int32_t reserved_;
} pp_tracks_image_options;
void pp_tracks_image_options_default(pp_tracks_image_options* o);

typedef struct pp_tracks_image_report {
  int64_t num_changed;       /* the reference's return value (num_tris) */
  int64_t num_entries;       /* events of this call; those beyond `capacity` are not written */
  int64_t ransac_trials;     /* trials of the RANSACs whose result was applied, summed */
  int32_t points_created;
  int32_t lines_continued;   /* TriangulateImage: lines that joined an existing point (Continue) */
  int32_t lines_redone;      /* lines whose speculation did not hold and which were evaluated again on the current state */
  int32_t fresh_launches;    /* kernel launches spent on them */
  double device_ms;          /* HIP-event time of the speculative launches */
  double replay_ms;          /* host replay, fresh launches included */
  double total_ms;
} pp_tracks_image_report;

/* line_aligned: L bytes, FeatureLine::IsAligned per line (Create makes no point from aligned lines alone, :511-514); NULL = none aligned */
int pp_tracks_triangulate_image(pp_tracks_handle h, const pp_tracks_image_options* options, int32_t image, const uint8_t* line_aligned,
                                pp_tracks_image_report* report, int32_t* event_point, int32_t* event_line, int64_t capacity);
int pp_tracks_complete_image(pp_tracks_handle h, const pp_tracks_image_options* options, int32_t image, pp_tracks_image_report* report,
                             int32_t* event_point, int32_t* event_line, int64_t capacity);

/* ---- FindLocalBundle on a pp_tracks_handle (kernels K12a k_local_bundle_count, K12b k_local_bundle_angles) ---------------------------------------
 * replaces IncrementalMapper::FindLocalBundle (sfm/incremental_mapper.cc:993-1160), the choice of the images that AdjustLocalBundle (:781-891) refines
 * after every registered image, with CalculateTriangulationAngles (base/triangulation.cc:84-118) and Percentile (util/math.h:232-246).
 * The device counts, for every other image, the track elements it shares with the points of the query image (one wavefront per line that has a
 * point) and computes, per image that the sequential loop can ask for, the 75th-percentile triangulation angle over ALL points of the query image
 * (one workgroup per image, a radix select over the bit patterns: exactly the value the nth_element of the reference leaves at the index, whatever the schedule).
 * The host replays the sequential rest: the sort, the eight relaxing (angle, overlap) thresholds, the lazy angle, the fill-up.
 * PINNED where the reference is unspecified: equal counts are ordered by ASCENDING IMAGE INDEX (the reference sorts what an unordered_map hands it);
 * a NaN angle sorts above every number in the percentile, and a NaN percentile fails every comparison, as in the reference.
 * The call does not change the handle's state.  ERRORS: PP_ERR_INVALID for an image index out of range, an UNREGISTERED query image (the reference
 * CHECKs it), local_ba_num_images < 2 or local_ba_min_tri_angle < 0.                                                                            */
typedef struct pp_local_bundle_options {
  int32_t local_ba_num_images;      /* 6   (sfm/incremental_mapper.h:77) */
  int32_t reserved_;
  double  local_ba_min_tri_angle;   /* 6.0 degrees (:80) */
} pp_local_bundle_options;
void pp_local_bundle_options_default(pp_local_bundle_options* o);

typedef struct pp_local_bundle_report {
  int32_t num_points3D;       /* image.NumPoints3D(): lines of the image that have a point */
  int32_t num_overlapping;    /* images sharing at least one track element */
  int32_t num_selected;       /* size of the bundle */
  int32_t angles_computed;    /* percentiles the device computed (speculation included) */
  int32_t angles_used;        /* percentiles the sequential loop would have computed (lazy, :1102-1119) */
  int32_t threshold_level;    /* last of the 8 selection thresholds reached, -1: early return (:1044) */
  int32_t filled;             /* images taken by the fill-up at the end (:1141-1157) */
  int32_t reserved_;
  double device_ms, replay_ms, total_ms;
} pp_local_bundle_report;

/* bundle: the selected image indices IN THE REFERENCE'S ORDER (AdjustLocalBundle fixes the gauge on the last two);
 * entries beyond bundle_capacity are not written (report->num_selected counts all).
 * overlap_image / overlap_count / overlap_tri_angle (C each, any may be NULL): the sorted overlapping list,
 * tri angle in radians, -1 where the sequential loop never asked for it. */
int pp_tracks_find_local_bundle(pp_tracks_handle h, const pp_local_bundle_options* options, int32_t image,
                                pp_local_bundle_report* report, int32_t* bundle, int32_t bundle_capacity,
                                int32_t* overlap_image, int32_t* overlap_count, double* overlap_tri_angle);

/* New poses / point positions / intrinsics on a live handle (after a bundle adjustment).
 * Any of the three groups may be empty / NULL.  intr is K x PP_CAM_STRIDE together with camera_skip (K, NULL = none),
 * re-decided by the caller.  The host state and the device copies change, the projection matrices (and the projection centres) are recomputed:
 * every later pp_tracks_* call on the handle sees the new values, exactly as a handle created from the updated arrays would.
 * ERRORS: PP_ERR_INVALID (an index out of range, a deleted point, a non-finite value, camera_skip without intr) leaves the handle as it was. */
int pp_tracks_update(pp_tracks_handle h, int32_t num_images, const int32_t* image_idx, const double* poses /* x7 */,
                     int32_t num_points, const int32_t* point_idx, const double* xyz /* x3 */,
                     const double* intr, const uint8_t* camera_skip);

/* ---- FindNextImages / RegisterNextImage on a pp_tracks_handle (kernels K13a k_visible_points, K13b k_register_corrs) ------------------------------
 * replaces IncrementalMapper::FindNextImages (sfm/incremental_mapper.cc:139-190) and the parts of RegisterNextImage (:570-760) around the pose
 * refinement: the visibility gate (:585), the 2D-3D correspondence search (:601-647, FindTransitiveCorrespondences(..., 1) =
 * base/correspondence_graph.cc:169-171), EstimateAbsolutePoseFromLines (estimators/pose.cc:52-94, the pp_pose_ransac code path on a pose handle
 * whose correspondences K13b wrote on the device), the gates after it (:725) and the commit (:743-757).  One handle so spans a reconstruction
 * from its first registered images to its last: find_next_images, estimate_image_pose, register_image, triangulate_image, find_local_bundle, update.
 * A line is OBSERVED when its neighbour list is not empty (CorrespondenceGraph::Finalize, correspondence_graph.cc:58-65) and VISIBLE when at
 * least one direct neighbour has a point (what Image::IncrementCorrespondenceHasPoint3D maintains, base/image.cc:91-98); the camera filter
 * applies to the correspondence search only.
 * PINNED where the reference is unspecified: images of equal rank are ordered by ASCENDING IMAGE INDEX (the reference sorts in the
 * order of an unordered_map), as pp_tracks_find_local_bundle pins equal counts.
 * THE CALLER does the pose refinement of :733-737 (RefineAbsolutePoseFromLines: a one-pose bundle adjustment, pp_ba_*) BETWEEN
 * pp_tracks_estimate_image_pose and pp_tracks_register_image: its camera block belongs to the caller, who may share it between images and may
 * refine it; a refined camera goes to the handle with pp_tracks_update.
 * LINES AND POINTS are the handle's line and point indices.                                                                                      */
typedef struct pp_next_image_options {   /* IncrementalMapper::Options, sfm/incremental_mapper.h */
  int32_t abs_pose_min_num_inliers;      /* 30 */
  int32_t max_reg_trials;                /* 3  */
  int32_t image_selection_method;        /* 0 MAX_VISIBLE_POINTS_NUM, 1 MAX_VISIBLE_POINTS_RATIO; default 1 (sfm/incremental_mapper.h:110) */
  int32_t reserved_;
} pp_next_image_options;
void pp_next_image_options_default(pp_next_image_options* o);

typedef struct pp_next_image_report {
  int32_t num_ranked;        /* images returned (both buckets); entries beyond `capacity` are not written */
  int32_t num_first_bucket;  /* of them: never tried and not filtered (:178-179) */
  int32_t num_unregistered;
  int32_t reserved_;
  double device_ms, replay_ms, total_ms;
} pp_next_image_report;

/* FindNextImages.  num_reg_trials (C, NULL = all 0) and filtered (C bytes, NULL = none) are the caller's num_reg_trials_ / filtered_images_.
 * ranked: image indices, first bucket then second bucket; num_visible / num_observations (C each, may be NULL): NumVisiblePoints3D / NumObservations
 * of EVERY image.  The handle does not change.  ERRORS: PP_ERR_INVALID for abs_pose_min_num_inliers <= 0, max_reg_trials < 0, an unknown method,
 * a negative trial count. */
int pp_tracks_find_next_images(pp_tracks_handle h, const pp_next_image_options* o, const int32_t* num_reg_trials, const uint8_t* filtered,
                               pp_next_image_report* report, int32_t* ranked, int32_t capacity, int32_t* num_visible, int32_t* num_observations);

/* pp_image_pose_report.failure: which `return false` of the reference was taken */
enum { PP_REG_OK = 0, PP_REG_FEW_VISIBLE = 1 /* :585 */, PP_REG_FEW_CORRS = 2 /* :653-657 */, PP_REG_NO_INLIERS = 3 /* pose.cc:65 */,
       PP_REG_ALIGNED = 4 /* pose.cc:71-83 */, PP_REG_NAN = 5 /* pose.cc:89 */, PP_REG_FEW_INLIERS = 6 /* :725 */ };

typedef struct pp_image_pose_report {
  int32_t failure;             /* PP_REG_*; 0: pose7 holds a pose */
  int32_t num_visible;         /* image.NumVisiblePoints3D() */
  int64_t num_corrs;           /* tri_corrs.size(); entries beyond `capacity` are not written (0 after PP_REG_FEW_VISIBLE: the search did not run) */
  uint64_t num_trials;         /* RANSAC report */
  int64_t num_inliers;
  int32_t num_aligned_inliers;
  int32_t reserved_;
  double device_ms;            /* HIP-event time of K13b, the scan and the RANSAC's launches */
  double replay_ms;            /* the host side of the RANSAC and the gates */
  double total_ms;
} pp_image_pose_report;

/* RegisterNextImage :584-727: visibility gate, 2D-3D search, P6L RANSAC, the gates after it.  Does NOT change the handle.
 * ransac: as the caller of :668-681 sets it (max_error through pp_camera_image_to_world_threshold).  line_aligned: L bytes, NULL = none.
 * pose7: (qw,qx,qy,qz,tx,ty,tz) as RotationMatrixToQuaternion leaves it (written when the RANSAC had an inlier, also on a later gate's failure).
 * corr_line / corr_point / inlier_mask: `capacity` entries each (corr_start[l + 1] - corr_start[l] summed over the image's lines always suffices);
 * inlier_mask is all 0 unless the RANSAC succeeded.  ERRORS: PP_ERR_INVALID for an image out of range or REGISTERED (the reference CHECKs it),
 * bad options, RANSACOptions::Check. */
int pp_tracks_estimate_image_pose(pp_tracks_handle h, const pp_next_image_options* o, const pp_ransac_options* ransac, int32_t image,
                                  const uint8_t* line_aligned /* L, NULL = none */, pp_image_pose_report* report, double* pose7,
                                  int32_t* corr_line, int32_t* corr_point, uint8_t* inlier_mask, int64_t capacity);

/* :743-757: the image becomes registered with `pose7`; the inlier correspondences (inlier_mask NULL = all) whose line has no point yet get their
 * observation, in list order: the first inlier of a line gives it its point, a later one is skipped; two lines may join one point.
 * event_point / event_line as pp_tracks_triangulate_image's events (one per AddObservation; *num_added counts all, those beyond `capacity` are not
 * written).  Validated BEFORE anything changes (PP_ERR_INVALID leaves the handle as it was): the image exists and is not registered, every line
 * belongs to it, every point exists and is not deleted, the pose is finite.  On success the host state and the device copies change as in
 * pp_tracks_update (pose, projection matrix, projection centre) together with image_registered: every later pp_tracks_* call sees what a handle
 * created from the updated arrays would. */
int pp_tracks_register_image(pp_tracks_handle h, int32_t image, const double* pose7, int64_t n, const int32_t* corr_line, const int32_t* corr_point,
                             const uint8_t* inlier_mask, int64_t* num_added, int32_t* event_point, int32_t* event_line, int64_t capacity);

/* ---- Point filters and image de-registration on a pp_tracks_handle (kernels K14a k_track_filter, K14b k_track_depth) ------------------------------
 * replaces, on the live handle, Reconstruction::FilterPoints3D / FilterPoints3DInImages / FilterAllPoints3D (base/reconstruction.cc:412-439, 594-719),
 * FilterObservationsWithNegativeDepth (:442-460), FilterImages (:462-484) and DeRegisterImage (:285-300), with DeleteObservation's rule that a track of
 * at most three elements takes its point with it (:264-267).  pp_ba_filter_points / pp_ba_filter_negative_depth state the same rules on a pp_ba_handle;
 * these run on the tracks, projection matrices and projection centres the tracks handle already holds, so the mapper neither flattens the model nor
 * builds a second problem to filter it, and the handle stays valid afterwards: one handle serves a reconstruction from its first images to its last.
 * K14a: one wavefront per point - the line error of every track element, the deletion rules of the two point filters, then the triangulation angle over
 * the pairs of surviving elements.  K14b: one lane per line - HasPointPositiveDepth.  The host applies the verdicts (csrc/tracks_filter_replay.hpp).
 * EVENTS, in the order the reference's Reconstruction sees them: (p, l) for a DeleteObservation that removed ONE element, (p, -1) for a DeletePoint3D
 * (a point a filter rule deleted, or the rest of a track that fell to three elements).  Events beyond `capacity` are not written (num_entries counts them all).
 * The point filter visits the points in ascending index and a point's elements in track order; a point the rules delete gives one (p, -1) event.
 * A DELETED point (merged away, filtered earlier) inside a subset is skipped, as the reference skips an id that no longer exists.
 * AFTER any of the three calls every later pp_tracks_* call, pp_tracks_get_state included, behaves as on a handle created from the resulting arrays.
 * ERRORS: PP_ERR_INVALID (a null argument, a negative option, both subsets given, an image_order that is not exactly the registered images, each once) is
 * decided before anything changes and leaves the handle as it was; any other error is as pp_tracks_complete's (destroy the handle).              */
typedef struct pp_tracks_filter_report {
  int64_t num_filtered;                /* the reference's return value */
  int64_t num_points_deleted, num_observations_deleted;   /* the latter: track elements removed, those of deleted points included */
  int64_t num_entries;
  int32_t points_tested, images_filtered;
  double device_ms, replay_ms, total_ms;
} pp_tracks_filter_report;

/* FilterPoints3D over point_subset (P' bytes over the CURRENT points), FilterPoints3DInImages over image_subset (C bytes: the points with a track element
 * in a flagged image), FilterAllPoints3D when both are NULL.  point_error (P', may be NULL): Point3D::Error of the points the filter kept, -1 elsewhere. */
int pp_tracks_filter_points(pp_tracks_handle h, const pp_filter_options* o, const uint8_t* line_aligned /* L, NULL = none */,
                            const uint8_t* point_subset /* P' or NULL */, const uint8_t* image_subset /* C or NULL */,
                            pp_tracks_filter_report* report, int32_t* event_point, int32_t* event_line, int64_t capacity,
                            double* point_error /* P', -1 where not set; may be NULL */);
/* FilterObservationsWithNegativeDepth.  image_order: the registered images in the order of their registration (the order of the reference's loop); the
 * lines of an image are visited in ascending index.  A flagged line whose point an earlier deletion of the call removed is not counted. */
int pp_tracks_filter_negative_depth(pp_tracks_handle h, const int32_t* image_order, int32_t num_registered,
                                    pp_tracks_filter_report* report, int32_t* event_point, int32_t* event_line, int64_t capacity);
/* FilterImages: the registered images, in image_order, that have no line with a point or whose camera is flagged in camera_skip are collected, then
 * de-registered in that order (every observation deleted, image_registered cleared on the host and on the device).  filtered_images (C entries) receives
 * them; report->images_filtered = report->num_filtered counts them.  A host pass over the lines: no kernel.  The kMinNumImages gate of
 * IncrementalMapper::FilterImages is the caller's. */
int pp_tracks_filter_images(pp_tracks_handle h, const int32_t* image_order, int32_t num_registered, int32_t* filtered_images /* C */,
                            pp_tracks_filter_report* report, int32_t* event_point, int32_t* event_line, int64_t capacity);

/* ---- The image sets of RegisterInitialLineImages on a pp_tracks_handle (kernels K15 k_initial_tracks<count / fill>, k_initial_keys) -------------
 * replaces the search for the image quadruples worth a four-view solve in IncrementalMapper::RegisterInitialLineImages (sfm/incremental_mapper.cc:199-435):
 * assemble_tracks (:265-290) over every line of the check images with the alignment filter (:326-332), the de-duplication the reference leaves to a
 * map from image set to a set of feature-index quadruples per class (:243-250, :353-359), the qualifying rule (:393-409), the ranking (:416-423) and the truncation to
 * max_num_init_tries sets (:434-435).  The console histograms (:365-383) are not mirrored.  The four-view solve itself is pp_fourview2d_lomsac /
 * pp_planar_lomsac below; the commit is pp_tracks_register_image with n = 0, then pp_tracks_triangulate_image, pp_tracks_complete, pp_tracks_merge: the
 * handle serves a reconstruction from ZERO registered images (P = 0 points, image_registered all 0) to its last.
 * A line r of a check image keeps the neighbours n with line_aligned[n] == line_aligned[r] whose image is in the subset; every index triple i < j < k of that
 * list for which the four images (r's and the three neighbours') are pairwise different is one TRACK: the four handle line numbers ordered by image index.
 * Identical tracks reached from several lines count once; the graph need not be symmetric.  A SET is the four image indices of a track; it QUALIFIES with
 * at least min_num_aligned_tracks aligned AND at least min_num_random_tracks unaligned unique tracks (and at least one of each).
 * The device counts the triples (one wavefront per line), scans, writes them as 16-byte records, sorts and de-duplicates them, keys them by image set
 * and run-length encodes the keys; the host ranks the runs (csrc/initial_sets_replay.hpp).
 * PINNED where the reference is unspecified (its sort is not a stable one): sets of equal aligned count are ordered by ASCENDING IMAGE SET, lexicographic over
 * the image indices, as pp_tracks_find_next_images and pp_tracks_find_local_bundle pin equal ranks.
 * LIMITS: the set key packs four image indices of 15 bits: at most 32768 images; max_candidates at most 2^31 - 1.
 * The call does not change the handle and reads nothing of its state.
 * ERRORS: PP_ERR_INVALID - decided before any device work, and before the handle is read where only the other arguments are wrong - for a null handle,
 * options, report, line_aligned or check_images, num_check <= 0, a check image that is negative, repeated, out of range or outside the subset, a negative
 * option, capacity > 0 without track_lines, max_num_sets > 0 without the four set arrays, more than 32768 images; and, after the count and BEFORE the
 * records are allocated, for more candidate tracks than max_candidates (pp_last_error names both numbers; the handle stays usable).              */
typedef struct pp_init_sets_options {
  int32_t min_num_aligned_tracks;   /* 20 (sfm/incremental_mapper.cc:396) */
  int32_t min_num_random_tracks;    /* 20 (:397) */
  int32_t max_num_sets;             /* 10 (max_num_init_tries, :434) */
  int32_t reserved_;
  int64_t max_candidates;           /* 1 << 24: tracks before de-duplication, 16 bytes each and as much again for the sort */
} pp_init_sets_options;
void pp_init_sets_options_default(pp_init_sets_options* o);

typedef struct pp_init_sets_report {
  int64_t num_candidates;           /* tracks emitted before de-duplication */
  int64_t num_aligned_tracks;       /* unique tracks of aligned lines, over all sets */
  int64_t num_random_tracks;        /* unique tracks of unaligned lines */
  int64_t num_track_entries;        /* tracks of the returned sets = track_start[2 * num_returned]: the capacity that holds them all */
  int32_t num_aligned_sets;         /* distinct sets with an aligned track */
  int32_t num_random_sets;          /* distinct sets with an unaligned track */
  int32_t num_qualified;
  int32_t num_returned;             /* min(num_qualified, max_num_sets) */
  int32_t num_work_lines;           /* lines of the check images that keep at least three neighbours: the wavefronts of K15 */
  int32_t overflow_lines;           /* of them: the filtered list is longer than the on-chip list (64) and went through global memory */
  double device_ms, replay_ms, total_ms;
} pp_init_sets_report;

/* line_aligned: L bytes, FeatureLine::IsAligned per line.  image_subset: C bytes, NULL = all (the reference's aligned_db_cache: the images that own an
 * aligned line).  check_images: handle image indices, each at most once, inside the subset (the reference draws up to ten).
 * set_images (x4, ascending), set_num_aligned, set_num_random: max_num_sets entries each, best set first.  track_start: 2 * max_num_sets + 1 entries, a CSR
 * over track_lines with two segments per set, the aligned tracks and then the unaligned ones, each in ascending lexicographic order of the four line numbers -
 * the order in which the reference hands the lines to the solver (:459-481).  track_lines: x4 handle line numbers per track, in the order of set_images;
 * tracks beyond `capacity` are not written (report->num_track_entries counts them all). */
int pp_tracks_find_initial_sets(pp_tracks_handle h, const pp_init_sets_options* options, const uint8_t* line_aligned /* L */,
                                const uint8_t* image_subset /* C or NULL */, const int32_t* check_images, int32_t num_check,
                                pp_init_sets_report* report, int32_t* set_images /* x4 */, int32_t* set_num_aligned, int32_t* set_num_random,
                                int64_t* track_start, int32_t* track_lines /* x4 */, int64_t capacity);

/* ---- BundleAdjuster::SetUp on a pp_tracks_handle (kernels K16 k_bundle_lines, k_bundle_tracks<count / fill>, k_bundle_first, k_bundle_gather) ------
 * replaces the flattening of the model in front of every bundle adjustment, BundleAdjuster::SetUp (optim/bundle_adjustment.cc:326-542: AddImageToProblem
 * :348-435, AddPointToProblem :437-488, ParameterizeCameras :490-528, ParameterizePoints :530-542): which observations, poses, points and cameras a
 * BundleAdjustmentConfig puts into the problem, in which order, and which of them are constant.  The arrays are those of pp_ba_problem_desc.
 * THE STREAM of observations: pass A - the lines l in ascending handle line number with image_flags[line_image[l]] & PP_BUNDLE_IMAGE and a point (the
 * images of the config in ascending index, their lines in line order); pass B - the points of variable_points, then those of constant_points, in the
 * order given: a point listed before is skipped, so is one whose observations of pass A already equal its track length; of every other one the track
 * elements, in track order, whose image is NOT in the config.  A pose / point / camera gets the next index when the stream (for cameras: the pose list)
 * first names it; a config image without an observation gets no pose.  The poses of pass A come first: num_config_poses of them.
 * CONSTANT: a pose of pass B, or of an image flagged PP_BUNDLE_CONST_POSE; a point whose track is longer than its observations in the problem, or that
 * constant_points lists (wherever else it is listed); a camera - mask 0xFFFF - when camera_subset_mask is NULL, when camera_const flags it, or when no
 * config image WITH an observation uses it; a variable camera gets its camera_subset_mask entry as given.  pose_tvec_mask is the caller's for a variable
 * pose of the config, else 0.
 * The device flags, counts and scans the lines, walks the listed tracks (one wavefront per point), ranks points and images by first appearance and gathers
 * the line coefficients (from the L x 3 the handle keeps on the device) and the positions; the host validates, de-duplicates the point lists and does
 * what is image- or camera-sized (csrc/bundle_setup_replay.hpp).  Integer atomics whose result is order-free only: the output does not depend on the
 * schedule.
 * bad_line: the reference CHECKs the direction of every line of pass A (CHECK_NEAR(line.head<2>().norm(), 1.0, 1e-6), :373).  pp_tracks_create already
 * REFUSES a line that fails this test (with sqrt(a^2 + b^2) for the norm), so no handle holds one: the device runs the test with hypot(a, b) all the same,
 * and bad_line can differ from -1 only for a norm within one rounding of the bound.  A line it names is reported, not an error of the call: the arrays
 * are filled all the same.
 * The call never changes the handle.  num_obs == 0 is a valid result.
 * CAPACITIES: the current number of track elements always suffices for obs_capacity, the current number of points for point_capacity
 * (pp_tracks_get_state); a smaller one is compared with the exact need, counted on the host.
 * ERRORS: PP_ERR_INVALID before any device work, with the outputs untouched: a null argument (tvec_const_mask, camera_const, camera_subset_mask may be
 * NULL; a point list only with a count of 0), a listed point that is out of range, deleted or has an empty track, an image of the config that is not
 * registered, a capacity that is too small. */
enum { PP_BUNDLE_IMAGE = 1, PP_BUNDLE_CONST_POSE = 2 };
typedef struct pp_bundle_config {
  const uint8_t*  image_flags;        /* C: PP_BUNDLE_IMAGE = in the config; PP_BUNDLE_CONST_POSE = !refine_extrinsics || HasConstantPose */
  const uint8_t*  tvec_const_mask;    /* C, NULL = none: bits as pp_ba_problem_desc (ignored for a constant pose) */
  const uint8_t*  camera_const;       /* K, NULL = none: BundleAdjustmentConfig::SetConstantCamera */
  const uint16_t* camera_subset_mask; /* K: constant-parameter bits a VARIABLE camera gets (from the refine_* flags);
                                         NULL = no refine flag set, every camera constant */
  const int32_t*  variable_points;    /* handle point indices IN THE ORDER VISITED (the mirror passes them sorted by id) */
  const int32_t*  constant_points;
  int32_t num_variable_points, num_constant_points;
} pp_bundle_config;

typedef struct pp_bundle_setup_report {
  int64_t num_obs, num_config_obs;    /* M; those of pass A */
  int32_t num_poses, num_config_poses, num_points, num_cameras;
  int64_t bad_line;                   /* first config line (ascending) with | |(a,b)| - 1 | > 1e-6 (CHECK_NEAR, .cc:373); -1 none */
  double device_ms, replay_ms, total_ms;
} pp_bundle_setup_report;

int pp_tracks_bundle_setup(pp_tracks_handle h, const pp_bundle_config* cfg, pp_bundle_setup_report* report,
    double* lines /* M x 3 */, int32_t* obs_pose, int32_t* obs_point, int32_t* obs_line /* handle line of each observation */, int64_t obs_capacity,
    int32_t* pose_image /* handle image of each pose */, uint8_t* pose_const, uint8_t* pose_tvec_mask, int32_t* pose_camera, /* C entries each */
    int32_t* point_index /* handle point of each problem point */, uint8_t* point_const, double* points /* x 3 */, int32_t point_capacity,
    int32_t* camera_index /* handle camera of each problem camera, K entries */, uint16_t* camera_const_mask /* K */);

/* ======================================================================================== *
 *  Four-view line initialisation (LO-MSAC)                                                   *
 *  replaces, for the out-of-plane-translation stage: ransac_lib::LocallyOptimizedMSAC<        *
 *  PlanarOffsetEstimator::Reconstruction, ..., PlanarOffsetEstimator>::EstimateModel            *
 *  (init/initializer.cc:196-206, lib/RansacLib/RansacLib/ransac.h:127-428) with                 *
 *  PlanarOffsetEstimator::{MinimalSolver, EvaluateModelOnPoint} + four_view_triangulate         *
 *  (init/initializer.cc:219-333); and the triangulate-all + score half of                      *
 *  FourView2dEstimator (init/sfm2d.cc:194-213, 302-319).                                        *
 *  FourView2dEstimator::MinimalSolver (trifocal tensor) and its Ceres LeastSquares: pp_fourview2d_minimal_batch,  *
 *  pp_fourview2d_least_squares, pp_fourview2d_lomsac below.                                      *
 *  Non-finite values keep the reference's meaning: an error is the reference's nested maximum   *
 *  max(e1, max(e2, max(e3, e4))) (sfm2d.cc:316, initializer.cc:332), a score its                *
 *  min(error, threshold) sums (ransac.h:302-305) - a NaN error is never an inlier and makes the *
 *  model's score NaN, which no `score < best` accepts: the model of a degenerate sample is      *
 *  never returned, and data with NaN bearings ends with 0 inliers as in the reference.          *
 * ======================================================================================== */

/* ransac_lib::LORansacOptions (lib/RansacLib/RansacLib/ransac.h:46-92) */
typedef struct pp_lomsac_options {
  uint32_t min_num_iterations;        /* 100   */
  uint32_t max_num_iterations;        /* 10000 */
  double success_probability;         /* 0.9999 */
  double squared_inlier_threshold;    /* 1.0 (the init solvers pass an UNSQUARED threshold: SURVEY.md App. B) */
  uint32_t random_seed;               /* 0 */
  int32_t num_lo_steps;               /* 10 */
  double threshold_multiplier;        /* sqrt(2) */
  int32_t num_lsq_iterations;         /* 4 */
  int32_t min_sample_multiplicator;   /* 7 */
  int32_t non_min_sample_multiplier;  /* 3 */
  uint32_t lo_starting_iterations;    /* 50 */
  int32_t final_least_squares;        /* 0 (initialize_reconstruction sets 1) */
  uint32_t chunk_iterations;          /* speculation width, 0 = auto */
} pp_lomsac_options;
void pp_lomsac_options_default(pp_lomsac_options* o);

/* ransac_lib::RansacStatistics (ransac.h:94-101) */
typedef struct pp_lomsac_report {
  uint32_t num_iterations;
  int32_t best_num_inliers;
  double best_model_score;
  double inlier_ratio;
  int32_t number_lo_iterations;
  int32_t num_inlier_indices;
  uint64_t hypotheses_evaluated;      /* minimal samples solved + scored on the device (>= num_iterations) */
  double device_time_s, total_time_s;
} pp_lomsac_report;

typedef struct pp_planar_impl* pp_planar_handle;
/* PlanarOffsetEstimator(poses, lines_r, Rg, threshold): poses 4 x (3x4 row-major, lifted 2D cameras, t_y = 0),
 * lines 4 x n x 3 (the unaligned line of every track in each view), Rg 4 x (3x3 row-major).          */
int pp_planar_create(int32_t n, const double* poses, const double* lines, const double* Rg, int device, pp_planar_handle* out);
int pp_planar_destroy(pp_planar_handle h);
/* MinimalSolver / NonMinimalSolver for a batch of samples (sample_size 3 = minimal; larger = least squares):
 * offsets num x 3 = t_y of cameras 1..3 (NaN where the 3x3 system is singular).  One lane per sample.   */
int pp_planar_solve_batch(pp_planar_handle h, int64_t num, int32_t sample_size, const int32_t* samples, double* offsets);
/* four_view_triangulate over ALL n tracks + EvaluateModelOnPoint + MSAC score sum_i min(err_i, thr) (summed
 * in index order, one lane per model) and strict-< inlier count, for a batch of models (= offset triples). */
int pp_planar_score(pp_planar_handle h, int32_t num_models, const double* offsets, double threshold, double* msac_score,
                    int32_t* num_inliers);
/* per-track errors (n) and triangulated points (n x 3, may be NULL) of ONE model; cams_out 4 x 12 (may be NULL) */
int pp_planar_evaluate(pp_planar_handle h, const double* offsets, double* errors, double* X, double* cams_out);
/* LocallyOptimizedMSAC<...PlanarOffsetEstimator>::EstimateModel.  cams_out 4 x 12, inlier_indices n ints. */
int pp_planar_lomsac(pp_planar_handle h, const pp_lomsac_options* options, pp_lomsac_report* report, double* offsets_out,
                     double* cams_out, int32_t* inlier_indices);

typedef struct pp_pose2d_impl* pp_pose2d_handle;
/* AbsolutePose2dEstimator(x, X) (src/init/sfm2d.h:99-143, sfm2d.cc:491-530; the estimator of the reference's own
 * RansacLib tests sfm2d_test.cc:164-236): x n x 2 bearings (normalised at create, as the ctor does), X n x 2 points. */
int pp_pose2d_create(int32_t n, const double* x, const double* X, int device, pp_pose2d_handle* out);
int pp_pose2d_destroy(pp_pose2d_handle h);
/* NonMinimalSolver (== MinimalSolver for sample_size 3) per sample, one lane each: poses num x (2x3 row-major) */
int pp_pose2d_solve_batch(pp_pose2d_handle h, int64_t num, int32_t sample_size, const int32_t* samples, double* poses);
/* EvaluateModelOnPoint (1 - cos) over all n points, MSAC sum in index order, strict-< inlier count, per model */
int pp_pose2d_score(pp_pose2d_handle h, int32_t num_models, const double* poses, double threshold, double* msac_score, int32_t* num_inliers);
/* EvaluateModelOnPoint of ONE model on all n points (the vector a RansacLib Solver adaptor answers the driver's per-point
 * calls from, ppsfm/ransaclib_solvers.hpp) */
int pp_pose2d_evaluate(pp_pose2d_handle h, const double* pose, double* errors);
/* LocallyOptimizedMSAC<Pose2d, ..., AbsolutePose2dEstimator>::EstimateModel; LeastSquares == NonMinimalSolver */
int pp_pose2d_lomsac(pp_pose2d_handle h, const pp_lomsac_options* options, pp_lomsac_report* report, double* pose_out, int32_t* inlier_indices);

typedef struct pp_fourview2d_impl* pp_fourview2d_handle;
/* FourView2dEstimator(x1..x4, thr): x = 4 x n x 2 bearings (normalised to unit length at create, as the ctor does) */
int pp_fourview2d_create(int32_t n, const double* x, int device, pp_fourview2d_handle* out);
int pp_fourview2d_destroy(pp_fourview2d_handle h);
/* for each model (4 cameras, 2x3 row-major each): three_view_triangulate2d over ALL n tracks with cameras 0..2,
 * EvaluateModelOnPoint, MSAC score (index order) and strict-< inlier count                                */
int pp_fourview2d_score(pp_fourview2d_handle h, int32_t num_models, const double* cams, double threshold, double* msac_score,
                        int32_t* num_inliers);
int pp_fourview2d_evaluate(pp_fourview2d_handle h, const double* cams, double* errors, double* X);
/* EvaluateModelOnPoint against the model's OWN points X (n x 2): what the reference evaluates (sfm2d.cc:302-319) for a model
 * whose points were refined by LeastSquares instead of triangulated from cameras 0..2 */
int pp_fourview2d_evaluate_points(pp_fourview2d_handle h, const double* cams, const double* X, double* errors);
/* The reference's factorize_trifocal_tensor draws three random 2x2 coordinate changes per call
 * (Matrix2d::setRandom(), sfm2d.cc:231-235).  Here they are an input: frames = A1,A2,A3 row-major (12 doubles);
 * NULL selects the fixed set pp_fourview2d_default_frames() returns.                                       */
int pp_fourview2d_default_frames(double* frames);
/* FourView2dEstimator::MinimalSolver (sfm2d.cc:363-444) for a batch of samples, one lane per sample: trifocal
 * tensor from the sample's bearings in views 1..3, factorisation, metric upgrade, the 8 sign choices, fourth
 * camera by AbsPoseSolver.  cams num x 16 x (4 x 2x3); counts[i] = 0 or 16 (NaN models where 0).           */
int pp_fourview2d_minimal_batch(pp_fourview2d_handle h, int64_t num, int32_t sample_size, const int32_t* samples, const double* frames,
                                double* cams, int32_t* counts);
/* FourView2dEstimator::NonMinimalSolver (sfm2d.cc:446-467): MinimalSolver, MSAC score of every candidate over ALL
 * n tracks, first strictly-smallest score wins.  cams num x (4 x 2x3) (NaN, score DBL_MAX, index -1 where the
 * minimal solver returned nothing); model_index may be NULL.  Everything stays on the device in between.   */
int pp_fourview2d_nonminimal_batch(pp_fourview2d_handle h, int64_t num, int32_t sample_size, const int32_t* samples, const double* frames,
                                   double threshold, double* cams, double* msac_score, int32_t* model_index);

/* FourView2dEstimator::LeastSquares (sfm2d.cc:469-489: bundle_adjust2d on the sample when it has >= 10 tracks, then
 * optimize_points2d on ALL tracks).  cams_inout 4 x (2x3), X_inout n x 2 = the model's points.  The reference calls
 * Ceres (absent, unpinned); the device restates its Levenberg-Marquardt: parity is "same minimiser", unpinned.      */
int pp_fourview2d_least_squares(pp_fourview2d_handle h, int32_t sample_size, const int32_t* sample, double* cams_inout, double* X_inout);
/* LocallyOptimizedMSAC<..., FourView2dEstimator>::EstimateModel, everything on the device (minimal solver + scoring in
 * batches, LeastSquares by the two LM kernels).  frames as for pp_fourview2d_minimal_batch.  cams_out 4 x (2x3),
 * X_out n x 2 (may be NULL), inlier_indices n ints.                                                               */
int pp_fourview2d_lomsac(pp_fourview2d_handle h, const pp_lomsac_options* options, const double* frames, pp_lomsac_report* report,
                         double* cams_out, double* X_out, int32_t* inlier_indices);

/* ======================================================================================== *
 *  SIFT descriptor matching (K17)                                                           *
 *  replaces: MatchSiftFeaturesCPUBruteForce (feature/sift.cc:54-143, 170-203, 957-970), the  *
 *  exact rule behind SiftCPUFeatureMatcher / SiftGPUFeatureMatcher (feature/matching.cc)     *
 * ======================================================================================== */

/* SiftMatchingOptions (feature/sift.h:117-145), the fields the brute-force rule reads.  max_num_matches is not among them: it only truncates the
 * inputs of the reference's SiftGPU path, MatchSiftFeaturesCPUBruteForce never reads it and neither does this library. */
typedef struct pp_sift_match_options {
  double max_ratio;        /* 0.8: a match is rejected when acos(best) >= max_ratio * acos(second), in float as the reference computes it */
  double max_distance;     /* 0.7: a match is rejected when acos(best) > max_distance                                                    */
  int32_t cross_check;     /* 1:   keep (i, j) only when j's best match is i                                                             */
  int32_t min_num_matches; /* 15:  a pair with fewer matches gets an empty list (feature/matching.cc:196-198, 414-416)                   */
  int64_t workspace_bytes; /* cap of the device workspace of one internal batch of pairs; 0 = the default (256 MiB).  A pair that needs
                              more on its own still runs, alone.                                                                         */
} pp_sift_match_options;
void pp_sift_match_options_default(pp_sift_match_options* o);

typedef struct pp_sift_match_report {
  int64_t num_matches;       /* over all pairs                                  */
  int32_t num_pairs_emptied; /* pairs with 1 .. min_num_matches - 1 matches     */
  int32_t num_batches;       /* internal batches the pair list was processed in */
  double device_ms, total_ms;
} pp_sift_match_report;

typedef struct pp_sift_impl* pp_sift_handle;
/* The descriptors of num_images images, uploaded once: descriptors is total x 128 uint8 row-major (FeatureDescriptors), image k owns the rows
 * desc_start[k] .. desc_start[k + 1] (desc_start has num_images + 1 entries, starts at 0 and does not decrease; an image with no descriptor is valid). */
int pp_sift_create(int32_t num_images, const int64_t* desc_start, const uint8_t* descriptors, int device, pp_sift_handle* out);
int pp_sift_destroy(pp_sift_handle h);
/* MatchSiftFeaturesCPUBruteForce for every listed pair (pairs: num_pairs x 2 image indices), the same matches in the same order: the pairs of
 * pair p are matches[2 * match_start[p] .. 2 * match_start[p + 1]) as (feature of the first image, feature of the second), ascending in the first.
 * A pair (i, i) and a pair listed twice are matched like any other: dropping them is the caller's job, as in SiftFeatureMatcher::Match.
 * capacity counts matches (pairs of int32): the sum over the pairs of min(N1, N2) always suffices with cross_check, the sum of N1 without it.  A smaller
 * capacity is compared with the exact need after the device work; too small is PP_ERR_INVALID and match_start, matches and the report are untouched.
 * Pairs are processed in internal batches whose workspace - 12 bytes per feature of both images of a pair for the top-2 results, 8 bytes per possible
 * match for the batch's output - stays below options->workspace_bytes.  One pair occupies only part of the device (a workgroup per 128 features and
 * direction): batches of pairs are the intended use. */
int pp_sift_match_pairs(pp_sift_handle h, const pp_sift_match_options* options, int64_t num_pairs, const int32_t* pairs, pp_sift_match_report* report,
                        int64_t* match_start, int32_t* matches, int64_t capacity);
/* The one-way scan of image1's features against image2's (K17a alone), N1 entries each: best = the largest dist, best_j = the lowest index that attains
 * it (-1: no positive dist), second = the second largest with multiplicity.  For tests and for a caller with another rule on top. */
int pp_sift_top2(pp_sift_handle h, int32_t image1, int32_t image2, int32_t* best_j, int32_t* best, int32_t* second);
/* The uint8 rows of one image of a handle, downloaded: descriptors is capacity x 128.  For a handle from pp_sift_create these are the bytes it was
 * given, for one from pp_sift_extract_to_matcher the bytes pp_sift_extract_batch returns for that image.  *num = the image's rows either way;
 * PP_ERR_INVALID for a null handle or num, an image outside the handle (then *num is untouched) or capacity < *num. */
int pp_sift_get_descriptors(pp_sift_handle h, int32_t image, uint8_t* descriptors, int64_t capacity, int64_t* num);
/* The integers the device compares (host only, needs no device): the distance rule passes iff best >= d_min (and best >= 1), the ratio rule iff
 * min(second, 262144) <= table[min(best, 262144) - d_min] (-1: never).  *count = 262144 - d_min + 1 entries; table may be NULL to ask for the count,
 * else capacity >= *count.  PP_ERR_INTERNAL when this host's acosf is not monotonic (csrc/sift_match_replay.hpp). */
int pp_sift_match_thresholds(const pp_sift_match_options* options, int32_t* d_min, int32_t* table, int64_t capacity, int64_t* count);

/* ======================================================================================== *
 *  Correspondence graph from the match lists (K18)                                          *
 *  replaces: the match loop of DatabaseCache::Load (base/database_cache.cc:82-191) and       *
 *  CorrespondenceGraph::AddCorrespondences / Finalize (base/correspondence_graph.cc:56-163), *
 *  up to the corr_start / corr_line CSR of pp_tracks_desc                                    *
 * ======================================================================================== */

typedef struct pp_corr_graph_report {
  int64_t num_pairs_used;         /* pairs with MORE than min_num_matches matches, self pairs included                                   */
  int64_t num_pairs_ignored;      /* the others                                                                                          */
  int64_t num_matches_in;         /* match_start[num_pairs]                                                                              */
  int64_t num_matches_accepted;   /* matches that entered the graph: the CSR has twice as many entries                                   */
  int64_t num_matches_bad_index;  /* matches of used pairs (self pairs apart) skipped for a line index that does not exist               */
  int64_t num_matches_duplicate;  /* ... skipped because a line already corresponded to the other image                                  */
  int64_t num_pairs_replayed;     /* used pairs whose valid matches repeat indices on BOTH sides: decided by the host's sequential loop  */
  double device_ms, replay_ms, total_ms;
} pp_corr_graph_report;

typedef struct pp_corr_graph_impl* pp_corr_graph_handle;
/* num_images images in ascending image-id order with their line counts (0 is valid).  Line x of image k is global line
 * line_start[k] + x, line_start the exclusive scan of num_lines: the numbering of pp_tracks_desc as IncrementalTriangulator.flatten makes it. */
int pp_corr_graph_create(int32_t num_images, const int32_t* num_lines, int device, pp_corr_graph_handle* out);
int pp_corr_graph_destroy(pp_corr_graph_handle h);
/* Builds the graph of the given match lists; it replaces the handle's previous one.  pairs: num_pairs x 2 image POSITIONS, in any order and either
 * orientation; the matches of pair p are matches[2 * match_start[p] .. 2 * match_start[p + 1]) as (line of the first image, line of the second) - the
 * layout pp_sift_match_pairs writes.  A pair is stored under its smaller image first and the pairs are applied in ascending (image1, image2); a pair is
 * USED iff it has more than min_num_matches matches (counted before any is skipped); a used pair (k, k) marks k connected and adds nothing.  A match
 * with an index out of range (negative included) is skipped, and so is one whose line already corresponds to the other image - the sequential rule of
 * AddCorrespondences, which the device applies as "first occurrence on both sides" and the host replays for the pairs where that differs
 * (csrc/corr_graph_replay.hpp).  The neighbours of a line come in the order of the used pairs that contributed them; the result is the same from run to run.
 * ERRORS: PP_ERR_INVALID before any device work, the previous graph untouched, for: a null argument, a negative min_num_matches, an image position out
 * of range, the same unordered pair listed twice, match_start[0] != 0 or a decreasing match_start, 2^31 matches or more.  PP_ERR_INVALID after the count,
 * the previous graph still untouched, when twice the accepted matches do not fit int32 (the CSR of pp_tracks_desc). */
int pp_corr_graph_build(pp_corr_graph_handle h, int32_t min_num_matches, int64_t num_pairs, const int32_t* pairs, const int64_t* match_start,
                        const int32_t* matches, pp_corr_graph_report* report);
/* The sizes of the last build: the global lines L and the CSR entries.  Either pointer may be NULL.  PP_ERR_INVALID before the first build. */
int pp_corr_graph_num_entries(pp_corr_graph_handle h, int64_t* num_lines, int64_t* num_entries);
/* The last build.  corr_start L + 1, corr_line `capacity` entries of room, image_connected / image_num_observations / image_num_correspondences
 * num_images each: connected = the image belongs to a used pair; observations = its lines with at least one neighbour (0: Finalize drops the image
 * from the graph, it stays connected); correspondences = its accepted matches.  Any pointer may be NULL.  PP_ERR_INVALID, nothing written, when
 * corr_line is given and capacity is too small, and before the first build. */
int pp_corr_graph_get(pp_corr_graph_handle h, int32_t* corr_start, int32_t* corr_line, int64_t capacity, uint8_t* image_connected,
                      int32_t* image_num_observations, int32_t* image_num_correspondences);
/* The accepted matches of every pair of the last build, in its input order (num_pairs entries); 0 for a pair that was not used and for a self pair. */
int pp_corr_graph_pair_counts(pp_corr_graph_handle h, int32_t* pair_num_correspondences);

/* ======================================================================================== *
 *  Line features from keypoints (K19)                                                       *
 *  replaces: the line generation of LineFeatureWriterThread::Run                             *
 *  (feature/extraction.cc:437-505); the detector and the descriptor stay outside            *
 * ======================================================================================== */

typedef struct pp_line_features_desc {
  int32_t num_images, num_cameras;
  const int32_t* image_ids;       /* num_images: the generator is keyed by them, not by the position in the batch                */
  const int64_t* kp_start;        /* num_images + 1: keypoint f of image k is global keypoint (= line) kp_start[k] + f; [0] = 0    */
  const float* keypoints;         /* L x 2 pixel (x, y), L = kp_start[num_images]                                                */
  const int32_t* image_camera;    /* num_images: index into the camera arrays                                                    */
  const int32_t* camera_model;    /* num_cameras model ids                                                                       */
  const double* intr;             /* num_cameras x PP_CAM_STRIDE                                                                 */
  const uint8_t* has_gravity;     /* num_images; NULL = no image has one                                                         */
  const double* gravity;          /* num_images x 3, read where has_gravity is set: Image::GravityDirection(), camera frame        */
} pp_line_features_desc;

typedef struct pp_line_features_options {
  double aligned_line_ratio;      /* 0.5 (feature/extraction.cc:160-162); in [0, 1]                                               */
  uint64_t seed;                  /* of the counter-based generator (csrc/line_features_replay.hpp); 0                            */
} pp_line_features_options;
void pp_line_features_options_default(pp_line_features_options* o);

typedef struct pp_line_features_report {
  int64_t num_lines;                   /* L                                                                                      */
  int64_t num_aligned;                 /* lines through the gravity direction                                                    */
  int64_t num_images_without_gravity;  /* they get random lines only (the reference prints a warning)                            */
  int64_t num_degenerate;              /* lines whose first two components have a zero or non-finite norm: written as computed   */
  int64_t num_newton_exhausted;        /* keypoints whose undistortion ran all 100 Newton iterations                             */
  double device_ms;
} pp_line_features_report;

/* One line per keypoint: the keypoint widened to double and undistorted with its image's camera to (u, v); d = the image's gravity direction for the
 * aligned features, else a random vector in [-1, 1)^3; the line is d x (u, v, 1) divided by the norm of its first two components.  An image with
 * gravity aligns the n features with the smallest generator key, n the smallest count with double(n) / double(N) >= aligned_line_ratio; an image
 * without gravity aligns none.  Every draw is a function of (seed, image id, feature index) alone: the same image gets the same lines in any batch.
 * lines_out L x 3, aligned_out L bytes, dirs_out NULL or L x 3 (the d of every line).
 * ERRORS: PP_ERR_INVALID before any device work for a null argument, a ratio outside [0, 1] (NaN included), kp_start[0] != 0 or a decreasing kp_start,
 * 2^31 keypoints or more, a camera index out of range, an unknown camera model, a non-finite intrinsic parameter or gravity component. */
int pp_line_features_from_keypoints(const pp_line_features_desc* desc, const pp_line_features_options* options, int device, double* lines_out,
                                    uint8_t* aligned_out, double* dirs_out, pp_line_features_report* report);

/* ======================================================================================== *
 *  Image-pair selection (K20)                                                               *
 *  replaces: the neighbour search of SpatialFeatureMatcher::Run (feature/matching.cc:       *
 *  705-768) and the candidate walk of one iteration of TransitiveFeatureMatcher::Run        *
 *  (:818-869); the sequential selection is closed-form host code (feature_matching.py)      *
 * ======================================================================================== */

typedef struct pp_pairs_report {
  int64_t num_pairs;        /* the pairs of the result                                                                                       */
  int64_t num_candidates;   /* spatial: num_locations^2 distances per pass; transitive: the (a, b, c) walks, the sum of degree(b)^2          */
  double device_ms;         /* the kernels, by events                                                                                        */
  double total_ms;          /* the call: checks, uploads, the kernels, the two waits for a count                                             */
} pp_pairs_report;

typedef struct pp_pairs_impl* pp_pairs_handle;
/* A handle keeps the result of its last selection on the device, so that asking for its size and fetching it compute nothing again.  A new handle holds
 * an empty result. */
int pp_pairs_create(int device, pp_pairs_handle* out);
int pp_pairs_destroy(pp_pairs_handle h);
/* The nearest neighbours of every location among all of them: xyz num_locations x 3 floats, knn = min(max_num_neighbors, num_locations).  The squared
 * distance is ((d0*d0) + d1*d1) + d2*d2 in float with every operation rounded on its own (never fused); the candidates of a query are ordered by
 * (squared distance, location index) ascending; of the first knn the query itself is dropped where it is among them, and the list is cut at the first
 * squared distance > (float)(max_distance * max_distance).  The result is the pairs (query, neighbour) as location indices, query by query in that
 * order, with the squared distances beside them: a fixed function of the input, bit for bit.
 * Every 1 <= knn <= num_locations is served.  Up to max_num_neighbors = 256 one selection round per query finds the list (about 6 to 9 passes over the
 * locations); above it the round is repeated for every further 256 ranks, so the cost grows with ceil(knn / 256).
 * ERRORS: PP_ERR_INVALID before any device work, the previous result untouched, for: a null argument, a negative num_locations or 2^31 - 1 or more, a
 * coordinate that is not finite, max_num_neighbors <= 0, max_distance <= 0 (NaN included).  PP_ERR_INVALID after the count and before anything is
 * written, the previous result still untouched, for a result of 2^31 - 1 pairs or more. */
int pp_pairs_spatial(pp_pairs_handle h, int64_t num_locations, const float* xyz, int32_t max_num_neighbors, double max_distance, pp_pairs_report* report);
/* One iteration of the transitive selection over num_images image positions.  matched_pairs (num_matched x 2) are the pairs with a non-empty match
 * list: they make the adjacency, in either orientation, repeats allowed.  tried_pairs (num_tried x 2) are the pairs that have been matched before with
 * whatever outcome.  The matched pairs are UNIONED into the tried ones: a caller may, but need not, list a matched pair among the tried.  The result is
 * every {a, c}, a != c, with a common neighbour that is not tried, as (a, c) with a < c, ascending in (a, c); no distances.  The images are walked in
 * chunks of 32768 positions, any num_images is served.
 * ERRORS: PP_ERR_INVALID before any device work, the previous result untouched, for: a null argument, a negative count, a position outside
 * [0, num_images), 2^30 listed pairs or more.  PP_ERR_INVALID after the count, the previous result still untouched, for 2^31 - 1 pairs or more. */
int pp_pairs_transitive(pp_pairs_handle h, int32_t num_images, int64_t num_matched, const int32_t* matched_pairs, int64_t num_tried,
                        const int32_t* tried_pairs, pp_pairs_report* report);
/* The size of the last result (0 for a new handle). */
int pp_pairs_num(pp_pairs_handle h, int64_t* n);
/* The last result: pairs n x 2 int32 positions, sqdist n floats; `capacity` pairs of room in each.  Either pointer may be NULL; sqdist must be NULL
 * after a transitive selection that found pairs.  PP_ERR_INVALID, nothing written, when capacity is too small. */
int pp_pairs_get(pp_pairs_handle h, int32_t* pairs, float* sqdist, int64_t capacity);

/* ======================================================================================== *
 *  SIFT keypoints and descriptors (K21)                                                     *
 *  replaces: ExtractSiftFeaturesCPU (feature/sift.cc:399-573) over VLFeat's vl_sift_*       *
 *  (lib/VLFeat/sift.c) for one grey image; the covariant extractor, domain-size pooling     *
 *  and SiftGPU's rule are absent                                                            *
 * ======================================================================================== */

typedef struct pp_sift_extract_options {
  int32_t max_num_features;      /* 8192: levels are dropped from the finest one up, whole (sift.cc:534-546)                                   */
  int32_t first_octave;          /* -1: the image is doubled first; -8 .. 8                                                                     */
  int32_t num_octaves;           /* 4; 1 .. 32 (the reference's "as many as fit" for a negative count is absent)                                */
  int32_t octave_resolution;     /* 3 levels per octave; 1 .. 32                                                                                */
  double peak_threshold;         /* 0.02 / 3                                                                                                    */
  double edge_threshold;         /* 10                                                                                                          */
  int32_t max_num_orientations;  /* 2: the FIRST local maxima of the orientation histogram in bin order; 1 .. 4                                 */
  int32_t upright;               /* 0; else one orientation 0 per keypoint                                                                      */
  int32_t normalization;         /* 0 L1_ROOT, 1 L2                                                                                             */
  int32_t phase_timings;         /* 0; else the stream is drained between the phases and phase_ms of the report is filled                       */
} pp_sift_extract_options;
void pp_sift_extract_options_default(pp_sift_extract_options* o);

#define PP_SIFT_MAX_OCTAVES 32
typedef struct pp_sift_extract_report {
  int32_t num_octaves;
  int32_t num_levels;              /* the per-level containers of the reference: one per run of keypoints of one DoG level of one octave        */
  int32_t first_level_to_keep;     /* the first container that max_num_features keeps                                                          */
  int32_t reserved_;
  int64_t num_keypoints;           /* refined keypoints, with or without an orientation                                                         */
  int64_t num_features_found;      /* features (keypoint, orientation) of all containers                                                        */
  int64_t num_features;            /* features kept = *num                                                                                      */
  int64_t num_two_orientations;    /* keypoints that gave more than one feature                                                                 */
  int64_t num_moved;               /* candidates whose refinement moved them                                                                    */
  int64_t num_rejected_peak, num_rejected_edge, num_rejected_offset, num_rejected_bounds;      /* candidates by the first test they failed     */
  int64_t num_windows_cut;         /* descriptors whose window the image border cut                                                             */
  int64_t num_descriptors_skipped; /* descriptors whose keypoint failed vl_sift_calc_keypoint_descriptor's bounds check: 128 zeros here         */
  int32_t octave_width[PP_SIFT_MAX_OCTAVES], octave_height[PP_SIFT_MAX_OCTAVES];
  int32_t octave_candidates[PP_SIFT_MAX_OCTAVES], octave_keypoints[PP_SIFT_MAX_OCTAVES];
  double phase_ms[5];              /* pyramid, detection, gradient, orientation, descriptor: by events, with phase_timings                      */
  double device_ms;                /* all kernels and copies between them, by events                                                            */
  double total_ms;                 /* the call                                                                                                  */
} pp_sift_extract_report;

typedef struct pp_sift_extractor_impl* pp_sift_extractor_handle;
/* A handle owns a stream and a workspace that grows to the largest image it has seen; it keeps the pyramid of its last extraction for the stage
 * readers below. */
int pp_sift_extractor_create(int device, pp_sift_extractor_handle* out);
int pp_sift_extractor_destroy(pp_sift_extractor_handle h);
/* grey: width x height uint8, row-major.  keypoints: capacity x 4 floats (x, y, scale, orientation) as FeatureKeypoint(x + 0.5f, y + 0.5f, sigma,
 * angle) holds them; descriptors: NULL or capacity x 128 bytes in UBC order; both in the reference's order, line index = keypoint index =
 * descriptor row.  The result is a fixed function of the input, bit for bit: keypoints, angles and the float descriptor before the last
 * normalisation equal the reference's CPU path (every sum in its order, nothing contracted; exp, pow, sin and cos are evaluated by the host's libm).
 * ABSENT, UNPINNED: the last normalisation of the reference sums with Eigen's reduction; here the L1 norm (the squared L2 norm) is the float32 sum
 * over the 128 entries from first to last.  A build of the reference can differ from this by one unit in a uint8 entry, and only where 512 v lies
 * within an ulp of a rounding tie.  A descriptor the reference leaves unwritten (its keypoint fails the descriptor's bounds check) is 128 zeros.
 * CAPACITY: the need is known after the device work; with capacity too small PP_ERR_INVALID, keypoints and descriptors untouched; *num is the
 * number of features either way.
 * ERRORS: PP_ERR_INVALID before any device work for: a null argument (descriptors may be NULL), a non-positive size, max_num_features,
 * octave_resolution, peak_threshold, edge_threshold or max_num_orientations not positive (NaN included), max_num_orientations > 4, an unknown
 * normalization, num_octaves or first_octave outside their range, a last octave without a pixel, a first octave of 2^30 pixels or more (int32
 * indexing of its gradient), a negative capacity. */
int pp_sift_extract(pp_sift_extractor_handle h, const pp_sift_extract_options* options, int32_t width, int32_t height, const uint8_t* grey,
                    pp_sift_extract_report* report, int64_t capacity, float* keypoints, uint8_t* descriptors, int64_t* num);
/* Stage readers of the LAST extraction of the handle (tests, and locating a difference).  kind 0 the Gaussian level, 1 the DoG level, 2 the gradient
 * (modulus, angle pairs: 2 floats per pixel); octave first_octave .. ; level s_min = -1 .. (Gaussian up to octave_resolution + 1, DoG one fewer,
 * gradient 0 .. octave_resolution - 1).  out: capacity floats; *width, *height the octave's size.  PP_ERR_INVALID without an extraction, for a
 * level that does not exist (an octave under 2 x 2 has no gradient) or a capacity too small. */
int pp_sift_extract_stage(pp_sift_extractor_handle h, int32_t kind, int32_t octave, int32_t level, float* out, int64_t capacity, int32_t* width,
                          int32_t* height);
/* the unrefined candidates (x, y, level) of one octave in scan order: capacity x 3; *num either way */
int pp_sift_extract_candidates(pp_sift_extractor_handle h, int32_t octave, int32_t* xys, int64_t capacity, int64_t* num);
/* Every feature found, BEFORE the max_num_features cut (the kept ones are the last *num of pp_sift_extract): raw capacity x 128 floats, the descriptor
 * in VLFeat's bin order before the last normalisation (all zero after an extraction without descriptors); octave_level capacity x 2 (octave, DoG
 * level); angles capacity doubles.  Any of the three may be NULL; *num either way. */
int pp_sift_extract_features(pp_sift_extractor_handle h, float* raw, int32_t* octave_level, double* angles, int64_t capacity, int64_t* num);

/* ---- a batch of images in one call (K23) ------------------------------------------------------------------------------------------------------ */
typedef struct pp_sift_batch_image {
  int32_t width, height;
  const uint8_t* grey;             /* width x height uint8, row-major                                                                           */
} pp_sift_batch_image;

typedef struct pp_sift_batch_report {
  int32_t num_images;
  int32_t num_sub_batches;         /* the images ran in this many groups (see MEMORY below)                                                      */
  int64_t num_features;            /* features kept, all images = offsets[num_images]                                                           */
  int64_t workspace_bytes;         /* pyramids, images and row counts of the largest sub-batch                                                  */
  double phase_ms[5];              /* as in pp_sift_extract_report, for the batch as a whole, with phase_timings                                */
  double device_ms;
  double total_ms;
} pp_sift_batch_report;

/* ExtractSiftFeaturesCPU for num_images grey images of possibly different sizes under ONE option set.  Image i's kept features are the rows
 * offsets[i] .. offsets[i + 1] of keypoints (capacity x 4) and descriptors (NULL or capacity x 128): in the order, and with exactly the bytes,
 * pp_sift_extract gives for that image alone; max_num_features cuts per image.  reports: num_images of them, the counts of each image, the timing
 * fields zero.  offsets: num_images + 1.
 * WHAT THE BATCH SHARES: the images go through the octaves in lock-step.  For one octave index the pyramid, the gradient, the candidate counts and
 * their scan of every image are launched (the kernels of pp_sift_extract, per image, on slices of one workspace) and all totals come back in one
 * download and one wait; likewise the refined candidates, the orientations and the descriptors: four waits per octave for the whole batch where a
 * loop over the images pays four per octave per image.  The descriptors of all images of an octave are ONE launch of a kernel that gives a
 * wavefront to every feature.  ITS ORDER RULE: the 64 lanes stage 64 window pixels at a time in scan order; each lane owns two of the 128 bins and
 * adds, pixel by pixel in that order, what the pixels contribute to them - so every bin receives its additions in the reference's order, and the
 * float descriptor, the bytes and the window flags equal the single call's bit for bit.  The norms are summed over the entries 0 .. 127 in order.
 * MEMORY: a group of images keeps the whole pyramid of each of them (a 3200 x 2400 image needs about 3 GB).  workspace_bytes is the target for the
 * sum, 0 means 8 GiB; groups are consecutive images in input order taken greedily under the target, an image that exceeds it on its own runs alone.
 * The result does not depend on the split.
 * AFTER THE CALL the handle holds no single extraction: pp_sift_extract_stage, _candidates and _features are PP_ERR_INVALID until the next
 * pp_sift_extract; pp_sift_extract_batch_features reads the batch.
 * CAPACITY: with capacity < offsets[num_images] PP_ERR_INVALID; batch_report, reports and offsets are filled, keypoints and descriptors untouched.
 * ERRORS: PP_ERR_INVALID before the handle is read, the outputs untouched, for: a null argument (descriptors may be NULL) or a null image,
 * num_images < 1, a negative capacity or workspace_bytes, every option and every size pp_sift_extract refuses - pp_last_error() names the index of
 * the offending image.
 * ABSENT: batch forms of the stage and candidate readers; orientation assignment by wavefront (it is the single call's kernel, per image). */
int pp_sift_extract_batch(pp_sift_extractor_handle h, const pp_sift_extract_options* options, int32_t num_images, const pp_sift_batch_image* images,
                          int64_t workspace_bytes, pp_sift_batch_report* batch_report, pp_sift_extract_report* reports, int64_t capacity, float* keypoints,
                          uint8_t* descriptors, int64_t* offsets);
/* pp_sift_extract_features for image `image` of the LAST batch: every feature of it before the cut.  PP_ERR_INVALID without a batch on the handle
 * (a pp_sift_extract since then discards it) or for an image outside it. */
int pp_sift_extract_batch_features(pp_sift_extractor_handle h, int32_t image, float* raw, int32_t* octave_level, double* angles, int64_t capacity,
                                   int64_t* num);

/* ---- a batch of images straight into a matcher (K24) -------------------------------------------------------------------------------------------- */
/* pp_sift_extract_batch for the case in which the features go to pp_sift_match_pairs: keypoints, offsets, reports, the argument checks, the groups
 * under workspace_bytes and the capacity rule are that call's.  There is no descriptor output on the host: *matcher becomes a NEW pp_sift_handle on
 * the extractor's device whose image i holds exactly the rows offsets[i] .. offsets[i + 1], in the state pp_sift_create would leave it in had it been
 * given the descriptors pp_sift_extract_batch returns - byte for byte (pp_sift_get_descriptors reads them).  Every pp_sift_* call works on it; the
 * caller destroys it with pp_sift_destroy, before or after the extractor.
 * WHAT IS NOT COMPUTED: max_num_features selects levels by their KEYPOINT counts, which are known after refinement.  A group therefore goes through
 * its octaves up to the keypoints first (two waits per octave), the cut is made on the host, and only the kept keypoints get orientations (one wait
 * per group) and descriptors: ONE launch per group over all octaves, a wavefront per feature with the order rule of pp_sift_extract_batch, which
 * writes each row where the matcher reads it.  2 x octaves + 2 waits per group; no float descriptor and no dropped feature leaves the device.
 * REPORTS: as pp_sift_extract_batch fills them, except that num_features_found, num_two_orientations, num_windows_cut and num_descriptors_skipped
 * count the KEPT containers only (num_features_found == num_features): the others were never computed.  The two are equal where nothing is cut.
 * AFTER THE CALL the extractor holds neither a single extraction nor a batch: the stage, candidate and feature readers and
 * pp_sift_extract_batch_features are PP_ERR_INVALID until the next pp_sift_extract or pp_sift_extract_batch.
 * ERRORS: those of pp_sift_extract_batch (descriptors aside), and a null matcher.  On any error *matcher is NULL and nothing stays allocated; with a
 * capacity too small batch_report, reports and offsets are filled as there. */
int pp_sift_extract_to_matcher(pp_sift_extractor_handle h, const pp_sift_extract_options* options, int32_t num_images,
                               const pp_sift_batch_image* images, int64_t workspace_bytes, pp_sift_batch_report* batch_report,
                               pp_sift_extract_report* reports, int64_t capacity, float* keypoints, int64_t* offsets, pp_sift_handle* matcher);

#ifdef __cplusplus
}
#endif
#endif /* PPSFM_HIP_H_ */
