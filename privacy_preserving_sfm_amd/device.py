"""Thin RAII wrappers over the C-ABI handles (pp_ba_handle, pp_pose_handle)."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import (BAOptions, BAProblemDesc, BASummary, RansacOptions, RansacReport, check, dp, f64, ptr)


def ba_options(**kw):
    return _capi.options(_capi.BAOptions, "pp_ba_options_default", **kw)


def ransac_options(**kw):
    return _capi.options(_capi.RansacOptions, "pp_ransac_options_default", **kw)


def _ba_desc(scene, keep, linear_solver=0, ordering=_capi.ORDERING_AUTO):
    """pp_ba_problem_desc of a scene dict (see BAProblem); `keep` receives the arrays the descriptor points to"""
    def k(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a
    d = BAProblemDesc()
    Cn = d.num_poses = int(np.shape(scene["poses"])[0])
    Pn = d.num_points = int(np.shape(scene["points"])[0])
    Kn = d.num_cameras = int(np.shape(scene["intr"])[0])
    d.num_obs = int(len(scene["obs_pose"]))
    d.loss_type = int(scene.get("loss_type", 0))
    d.loss_scale = float(scene.get("loss_scale", 1.0))
    d.lines = dp(k(scene["lines"], np.float64))
    d.obs_pose = ptr(k(scene["obs_pose"], np.int32), _capi.c_ip)
    d.obs_point = ptr(k(scene["obs_point"], np.int32), _capi.c_ip)
    d.pose_camera = ptr(k(scene["pose_camera"], np.int32), _capi.c_ip)
    d.camera_model = ptr(k(scene["camera_model"], np.int32), _capi.c_ip)
    d.pose_const = ptr(k(scene.get("pose_const", np.zeros(Cn)), np.uint8), _capi.c_u8p)
    d.tvec_const_mask = ptr(k(scene.get("tvec_const_mask", np.zeros(Cn)), np.uint8), _capi.c_u8p)
    d.point_const = ptr(k(scene.get("point_const", np.zeros(Pn)), np.uint8), _capi.c_u8p)
    d.camera_const_mask = ptr(k(scene.get("camera_const_mask", np.full(Kn, 0xFFFF)), np.uint16), _capi.c_u16p)
    d.linear_solver = int(scene.get("linear_solver", linear_solver))
    d.ordering = int(scene.get("ordering", ordering))
    cov = scene.get("covisibility")      # C x C bytes: the union co-visibility of a point-sharded group (pp_ba_problem_desc::covisibility)
    if cov is not None:
        cov = k(cov, np.uint8)
        assert cov.shape == (Cn, Cn)
        d.covisibility = ptr(cov, _capi.c_u8p)
    return d


def covisibility(scene):
    """pp_ba_covisibility: C x C bytes, 1 where two variable images of the scene (a shard) share a variable point - host only"""
    keep = []
    d = _ba_desc(scene, keep)
    out = np.zeros((d.num_poses, d.num_poses), dtype=np.uint8)
    check(_capi.lib().pp_ba_covisibility(C.byref(d), ptr(out, _capi.c_u8p)))
    return out


def plan_ordering(scene, linear_solver=0, ordering=_capi.ORDERING_AUTO):
    """pp_ba_plan_ordering: the image order pp_ba_create would choose, on the host alone -> (old_of_new [C], dict(reordered, nnz_natural, nnz_used, chains,
    chain_steps, block_columns, block_sparse, intrinsics_columns))"""
    keep = []
    d = _ba_desc(scene, keep, linear_solver, ordering)
    oon = np.zeros(d.num_poses, dtype=np.int32)
    info = np.zeros(8, dtype=np.int32)
    check(_capi.lib().pp_ba_plan_ordering(C.byref(d), ptr(oon, _capi.c_ip), ptr(info, _capi.c_ip)))
    return oon, dict(reordered=bool(info[0]), nnz_natural=int(info[1]), nnz_used=int(info[2]), chains=int(info[3]), chain_steps=int(info[4]),
                     block_columns=int(info[5]), block_sparse=bool(info[6]), intrinsics_columns=int(info[7]))


_COV_KINDS = {"pose": _capi.COV_POSE, "intrinsics": _capi.COV_INTRINSICS, "point": _capi.COV_POINT}


def _cov_block_request(blocks):
    """((kind, index), (kind, index)) pairs -> (pp_cov_block array, [(w_a, w_b)], offsets [len + 1]: block q at offsets[q] .. offsets[q + 1] of the output)"""
    blocks = list(blocks)
    req = (_capi.CovBlock * max(1, len(blocks)))()
    shapes, offsets = [], [0]
    for q, ((ka, ia), (kb, ib)) in enumerate(blocks):
        for k in (ka, kb):
            if k not in _COV_KINDS:
                raise ValueError("covariance_blocks: block %d has the unknown kind %r (pose, intrinsics, point)" % (q, k))
        req[q] = _capi.CovBlock(_COV_KINDS[ka], int(ia), _COV_KINDS[kb], int(ib))
        shapes.append((_capi.COV_WIDTH[_COV_KINDS[ka]], _capi.COV_WIDTH[_COV_KINDS[kb]]))
        offsets.append(offsets[-1] + shapes[-1][0] * shapes[-1][1])
    return req, shapes, offsets


class _Handle:
    """A C handle and its end: close() gives it to the subclass's pp_*_destroy once, __del__ closes what was left open."""
    _destroy = None

    def __init__(self):
        self._h = C.c_void_p()

    def close(self):
        if self._h:
            getattr(_capi.lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BAProblem(_Handle):
    """Device-resident bundle adjustment problem (one per sub-model / GPU).

    `scene` is a dict of flat arrays (see privacy_preserving_sfm_amd.synthetic.make_ba_scene):
    lines [M,3], obs_pose [M], obs_point [M], pose_camera [C], camera_model [K], poses [C,7],
    points [P,3], intr [K,12], pose_const [C], tvec_const_mask [C], point_const [P],
    camera_const_mask [K], loss_type, loss_scale.
    """
    _destroy = "pp_ba_destroy"

    def __init__(self, scene, device=0, linear_solver=0, ordering=_capi.ORDERING_AUTO):
        L = _capi.lib()
        super().__init__()
        self._keep = []
        # linear_solver: 0 = by image count like BundleAdjuster::Solve (> 1000 images: ITERATIVE_SCHUR + SCHUR_JACOBI), 1 = direct, 2 = iterative
        # ordering: PP_ORDERING_AUTO (2, this mirror's default - Ceres orders without being asked) = the library may renumber the images internally (reverse Cuthill-McKee, nested dissection: when it makes the factor sparser / its
        # factorisation shorter), 1 = the caller's order (the shards of a point-sharded group: every rank must lay out the exchanged system alike)
        d = _ba_desc(scene, self._keep, linear_solver, ordering)
        self.C, self.P, self.K, self.M = int(d.num_poses), int(d.num_points), int(d.num_cameras), int(d.num_obs)
        check(L.pp_ba_create(C.byref(d), int(device), C.byref(self._h)))
        self._keep = []   # the library copied everything it needs
        if "poses" in scene:
            self.set_parameters(scene["poses"], scene["points"], scene["intr"])

    def structure(self):
        """pp_ba_get_structure: dict(tiles, nnz_natural, nnz_used, reordered, block_sparse, iterative, chains, chain_steps) of the reduced camera system, and
        pp_ba_get_intrinsics_layout: intrinsics_columns, private_intrinsics (n_v beside every image's pose columns, 0: behind all pose columns),
        wide_intrinsics (n_v of the wide-row assembly, 0: the general block pairs), jcam_stride"""
        info = np.zeros(8, dtype=np.int32)
        check(_capi.lib().pp_ba_get_structure(self._h, ptr(info, _capi.c_ip)))
        lay = np.zeros(4, dtype=np.int32)
        check(_capi.lib().pp_ba_get_intrinsics_layout(self._h, ptr(lay, _capi.c_ip)))
        return dict(tiles=int(info[0]), nnz_natural=int(info[1]), nnz_used=int(info[2]), reordered=bool(info[3]), block_sparse=bool(info[4]),
                    iterative=bool(info[5]), chains=int(info[6]), chain_steps=int(info[7]), intrinsics_columns=int(lay[0]), private_intrinsics=int(lay[1]),
                    wide_intrinsics=int(lay[2]), jcam_stride=int(lay[3]))

    def create_profile(self):
        """pp_ba_get_create_profile: host ms of the pp_ba_create behind this handle - dict(ordering, pair_lists, structure, upload, task_plan, total)"""
        ms = np.zeros(6)
        check(_capi.lib().pp_ba_get_create_profile(self._h, dp(ms)))
        return dict(ordering=float(ms[0]), pair_lists=float(ms[1]), structure=float(ms[2]), upload=float(ms[3]), task_plan=float(ms[4]), total=float(ms[5]))

    def set_parameters(self, poses=None, points=None, intr=None):
        poses = None if poses is None else f64(poses)
        points = None if points is None else f64(points)
        intr = None if intr is None else f64(intr)
        check(_capi.lib().pp_ba_set_parameters(self._h, dp(poses), dp(points), dp(intr)))

    def get_parameters(self):
        poses = np.zeros((self.C, 7)); points = np.zeros((self.P, 3)); intr = np.zeros((self.K, _capi.CAM_STRIDE))
        check(_capi.lib().pp_ba_get_parameters(self._h, dp(poses), dp(points), dp(intr)))
        return poses, points, intr

    def evaluate(self, ambient=False, want_cam=False):
        """Batched CostFunction::Evaluate (kernel K1): returns (cost, residuals, J_pose, J_point, J_cam|None)."""
        r = np.zeros(2 * self.M)
        jp = np.zeros((self.M, 14 if ambient else 12))
        jx = np.zeros((self.M, 6))
        jc = np.zeros((self.M, 2 * _capi.CAM_STRIDE)) if want_cam else None
        cost = C.c_double(0)
        check(_capi.lib().pp_ba_eval(self._h, 1 if ambient else 0, 1 if want_cam else 0, dp(r), dp(jp), dp(jx), dp(jc),
                                     C.cast(C.byref(cost), _capi.c_dp)))
        return cost.value, r, jp, jx, jc

    def evaluate_device(self, repeat=1, ambient=False, want_cam=False):
        """Runs K1 `repeat` times without host copies; returns HIP-event ms per launch."""
        ms = C.c_float(0)
        check(_capi.lib().pp_ba_eval_device(self._h, 1 if ambient else 0, 1 if want_cam else 0, int(repeat), C.byref(ms)))
        return ms.value

    def solve(self, options=None, iteration_callback=None):
        """pp_ba_solve.  `iteration_callback(it: BAIterationSummary) -> 0 continue / 1 abort / 2 terminate successfully`
        is the ceres::IterationCallback of Solver::Options::callbacks.  A numeric failure raises PPError with the
        filled summary attached as `.summary` (Ceres returns a Summary with termination FAILURE)."""
        o = options or ba_options()
        s = BASummary()
        cb = None
        if iteration_callback is not None:
            def _cb(ctx, it):
                try:
                    return int(iteration_callback(it.contents) or 0)
                except Exception:        # a ctypes callback must not raise: an exception aborts the solve
                    import traceback
                    traceback.print_exc()
                    return _capi.SOLVER_ABORT
            cb = _capi.ITERATION_FN(_cb)
            o.iteration_callback = C.cast(cb, C.c_void_p)
        try:
            rc = _capi.lib().pp_ba_solve(self._h, C.byref(o), C.byref(s))
        finally:
            if cb is not None:
                o.iteration_callback = None
        if rc != 0:
            err = _capi.PPError(rc, _capi.lib().pp_last_error().decode(errors="replace"))
            err.summary = s
            raise err
        return s

    def trace(self, capacity=1024):
        t = np.zeros((capacity, 7))
        n = C.c_int32(0)
        check(_capi.lib().pp_ba_get_trace(self._h, dp(t), capacity, C.byref(n)))
        return t[: n.value].copy()

    def reduced_system(self, radius, options=None):
        o = options or ba_options()
        ncap = 6 * self.C + 12 * self.K      # (every camera block variable at most)
        S = np.zeros(ncap * ncap); rhs = np.zeros(ncap)
        n = C.c_int32(0)
        check(_capi.lib().pp_ba_reduced_system(self._h, C.byref(o), float(radius), C.byref(n), dp(S), dp(rhs), S.size))
        n = n.value
        return S[: n * n].reshape(n, n).copy(), rhs[:n].copy()

    def covariance(self, pose_pairs=None, points=None, options=None, return_info=False):
        """pp_ba_covariance at the current parameters: (pose_cov [pairs, 6, 6], point_cov [points, 3, 3]).
        pose_pairs: sequence of (i, j) in the scene's image order, block = Cov(delta_i, delta_j) in the tangent order of `evaluate` (3 rotation, 3 tvec);
        None = every diagonal block (i, i).  points: point indices; None = no points.  No sigma^2 factor is applied.  return_info: also the
        BACovarianceInfo (n, path, device_ms)."""
        o = options or ba_options()
        if pose_pairs is None:
            pose_pairs = np.stack([np.arange(self.C), np.arange(self.C)], axis=1)
        pp = np.asarray(pose_pairs, dtype=np.int64).reshape(-1, 2)
        pi = np.ascontiguousarray(pp[:, 0], dtype=np.int32); pj = np.ascontiguousarray(pp[:, 1], dtype=np.int32)
        ids = np.ascontiguousarray(np.asarray([] if points is None else points, dtype=np.int64).reshape(-1), dtype=np.int32)
        pc = np.zeros((len(pi), 6, 6)); xc = np.zeros((len(ids), 3, 3))
        info = _capi.BACovarianceInfo()
        check(_capi.lib().pp_ba_covariance(self._h, C.byref(o), len(pi), ptr(pi, _capi.c_ip), ptr(pj, _capi.c_ip), dp(pc), len(ids), ptr(ids, _capi.c_ip), dp(xc),
                                           C.byref(info)))
        return (pc, xc, info) if return_info else (pc, xc)

    def covariance_blocks(self, blocks, options=None, return_info=False):
        """pp_ba_covariance_blocks at the current parameters: the covariance block of every requested pair of parameter blocks.
        blocks: sequence of ((kind, index), (kind, index)), kind "pose" (an image of the scene, 6 rows: 3 rotation, 3 tvec), "intrinsics" (a row of the
        scene's intr, 12 rows: its parameter slots) or "point" (3 rows).  Returns a list of arrays of shape (w_a, w_b), in request order; zero rows and
        columns for what is constant.  No sigma^2 factor is applied.  return_info: also the BACovarianceInfo (n, path, device_ms)."""
        o = options or ba_options()
        req, shapes, offsets = _cov_block_request(blocks)
        out = np.zeros(offsets[-1])
        info = _capi.BACovarianceInfo()
        check(_capi.lib().pp_ba_covariance_blocks(self._h, C.byref(o), len(shapes), req, dp(out), out.size, C.byref(info)))
        res = [out[offsets[q]:offsets[q + 1]].reshape(shapes[q]).copy() for q in range(len(shapes))]
        return (res, info) if return_info else res

    def timings(self):
        ms = np.zeros(len(_capi.BA_T_NAMES)); calls = np.zeros(len(_capi.BA_T_NAMES), dtype=np.int32)
        check(_capi.lib().pp_ba_get_timings(self._h, dp(ms), ptr(calls, _capi.c_ip)))
        return {n: (float(ms[i]), int(calls[i])) for i, n in enumerate(_capi.BA_T_NAMES)}

    def filter_points(self, max_reproj_error, min_tri_angle_deg, cam_size, obs_aligned=None, point_subset=None):
        """Reconstruction::FilterPoints3D on the handle's current parameters -> (report, obs_deleted [M] bool,
        point_deleted [P] bool, point_error [P])."""
        M = self.M
        o = _capi.FilterOptions(float(max_reproj_error), float(min_tri_angle_deg))
        rep = _capi.FilterReport()
        cs = np.ascontiguousarray(cam_size, dtype=np.int32).reshape(self.K, 2)
        al = None if obs_aligned is None else np.ascontiguousarray(obs_aligned, dtype=np.uint8)
        sub = None if point_subset is None else np.ascontiguousarray(point_subset, dtype=np.uint8)
        od = np.zeros(M, dtype=np.uint8); pd = np.zeros(self.P, dtype=np.uint8); pe = np.zeros(self.P)
        check(_capi.lib().pp_ba_filter_points(self._h, C.byref(o), None if al is None else ptr(al, _capi.c_u8p), ptr(cs, _capi.c_ip),
                                              None if sub is None else ptr(sub, _capi.c_u8p), ptr(od, _capi.c_u8p), ptr(pd, _capi.c_u8p), dp(pe), C.byref(rep)))
        return rep, od.astype(bool), pd.astype(bool), pe

    def filter_negative_depth(self):
        """Reconstruction::FilterObservationsWithNegativeDepth -> (count, obs_negative [M] bool)."""
        neg = np.zeros(self.M, dtype=np.uint8); n = C.c_int64(0)
        check(_capi.lib().pp_ba_filter_negative_depth(self._h, ptr(neg, _capi.c_u8p), C.byref(n)))
        return int(n.value), neg.astype(bool)

    def set_communicator(self, comm):
        """The group's reductions as RCCL collectives on the handle's stream (pp_ba_set_communicator); None detaches.
        COLLECTIVE when the communicator has more than one rank: every rank of the group calls it (one all-reduce of three doubles inside the
        call - the common refusal and the hash of the reduced system's layout); all ranks get the same verdict."""
        self._comm = comm
        check(_capi.lib().pp_ba_set_communicator(self._h, comm._h if comm is not None else None))

    def set_allreduce(self, fn, group_rank=0, group_size=1):
        """fn(device_ptr:int, count:int, op:int) reduces `count` doubles in place across the group
        (op 0 = sum, 1 = max).  None => single GPU.
        COLLECTIVE when group_size > 1: the attach itself calls fn once (three doubles, max) - every rank of the group attaches, each from its
        own thread / process, and fn must already be able to rendezvous; all ranks get the same verdict (PPError PP_ERR_INVALID everywhere when
        one rank renumbered its images from its own shard or the ranks' layouts of the reduced system differ)."""
        if fn is None:
            self._ar = None
            check(_capi.lib().pp_ba_set_allreduce(self._h, None, None, 0, 1))
            return
        self._ar = _capi.ALLREDUCE_FN(lambda ctx, p, n, op: int(fn(p, n, op) or 0))
        check(_capi.lib().pp_ba_set_allreduce(self._h, C.cast(self._ar, C.c_void_p), None, int(group_rank), int(group_size)))


class Communicator(_Handle):
    """RCCL communicator of one point-sharded BA group (pp_comm_*): `unique_id()` on the group's rank 0, the 128 bytes sent to
    the other ranks by any means, then `Communicator(id, num_ranks, rank, device)` on every rank of the group."""
    _destroy = "pp_comm_destroy"

    @staticmethod
    def unique_id():
        buf = np.zeros(128, dtype=np.uint8)
        check(_capi.lib().pp_comm_unique_id(ptr(buf, _capi.c_u8p)))
        return buf

    def __init__(self, unique_id, num_ranks, rank, device=0):
        super().__init__()
        uid = np.ascontiguousarray(unique_id, dtype=np.uint8)
        assert uid.size == 128
        self.rank, self.size = int(rank), int(num_ranks)
        check(_capi.lib().pp_comm_create(ptr(uid, _capi.c_u8p), self.size, self.rank, int(device), C.byref(self._h)))

    def allreduce(self, device_ptr, count, op=0):
        check(_capi.lib().pp_comm_allreduce(self._h, C.c_void_p(int(device_ptr)), int(count), int(op)))


class PoseProblem(_Handle):
    """Device-resident 2D-line / 3D-point correspondences of one image (X, Y of the Estimator concept)."""
    _destroy = "pp_pose_destroy"

    def __init__(self, lines2D, points3D, aligned=None, device=0):
        super().__init__()
        lines2D, points3D = f64(lines2D), f64(points3D)
        self.n = int(lines2D.shape[0])
        al = None if aligned is None else np.ascontiguousarray(aligned, dtype=np.uint8)
        check(_capi.lib().pp_pose_create(self.n, dp(lines2D), dp(points3D), ptr(al, _capi.c_u8p), int(device), C.byref(self._h)))

    def residuals(self, models):
        models = f64(models).reshape(-1, 12)
        out = np.zeros((models.shape[0], self.n))
        check(_capi.lib().pp_pose_residuals(self._h, models.shape[0], dp(models), dp(out)))
        return out

    def score(self, models, max_residual, sequential=False):
        models = f64(models).reshape(-1, 12)
        inl = np.zeros(models.shape[0], dtype=np.uint32); sums = np.zeros(models.shape[0])
        fn = _capi.lib().pp_pose_support_sequential if sequential else _capi.lib().pp_pose_score
        check(fn(self._h, models.shape[0], dp(models), float(max_residual), ptr(inl, _capi.c_u32p), dp(sums)))
        return inl, sums

    def p6l_batch(self, samples):
        samples = np.ascontiguousarray(samples, dtype=np.uint32).reshape(-1, 6)
        H = samples.shape[0]
        models = np.zeros((H, 8, 12)); nm = np.zeros(H, dtype=np.int32)
        check(_capi.lib().pp_pose_p6l_batch(self._h, H, ptr(samples, _capi.c_u32p), dp(models), ptr(nm, _capi.c_ip)))
        return models.reshape(H, 8, 3, 4), nm

    def ransac(self, options):
        rep = RansacReport()
        mask = np.zeros(max(self.n, 1), dtype=np.uint8)
        check(_capi.lib().pp_pose_ransac(self._h, C.byref(options), C.byref(rep), ptr(mask, _capi.c_u8p)))
        return rep, mask[: self.n]

    def last_scores(self, num_hyp):
        """(num_models [H], num_inliers [H,8], residual_sum [H,8]) of every model of the last `hypotheses` call."""
        nm = np.zeros(num_hyp, dtype=np.int32); inl = np.zeros((num_hyp, 8), dtype=np.uint32); sm = np.zeros((num_hyp, 8))
        check(_capi.lib().pp_pose_last_scores(self._h, int(num_hyp), ptr(nm, _capi.c_ip), ptr(inl, _capi.c_u32p), dp(sm)))
        return nm, inl, sm

    def hypotheses(self, num_hyp, max_residual, samples=None, seed=0):
        rep = RansacReport()
        s = None if samples is None else np.ascontiguousarray(samples, dtype=np.uint32)
        check(_capi.lib().pp_pose_hypotheses(self._h, int(num_hyp), ptr(s, _capi.c_u32p), int(seed), float(max_residual), C.byref(rep)))
        return rep


def re3q3_batch(coeffs, device=0):
    coeffs = f64(coeffs).reshape(-1, 30)
    n = coeffs.shape[0]
    sols = np.zeros((n, 3, 8)); ns = np.zeros(n, dtype=np.int32)
    check(_capi.lib().pp_re3q3_batch(n, dp(coeffs), dp(sols), ptr(ns, _capi.c_ip), int(device)))
    return sols, ns


def sampler_draw(seed, n, k, count):
    out = np.zeros((count, k), dtype=np.uint32)
    check(_capi.lib().pp_sampler_draw(int(seed), int(n), int(k), int(count), ptr(out, _capi.c_u32p)))
    return out


def device_count():
    c = C.c_int(0)
    check(_capi.lib().pp_device_count(C.byref(c)))
    return c.value


def dense_cholesky_solve(A, b, device=0, repeat=1):
    """Solve the SPD system A x = b with the reduced-camera-system solver (K3b).  Returns (x, ms)."""
    A, b = f64(A), f64(b)
    n = A.shape[0]
    x = np.zeros(n)
    ms = C.c_float(0)
    check(_capi.lib().pp_dense_cholesky_solve(n, dp(A), dp(b), dp(x), int(device), int(repeat), C.byref(ms)))
    return x, ms.value


def lomsac_options(**kw):
    return _capi.options(_capi.LoMsacOptions, "pp_lomsac_options_default", **kw)


class PlanarOffsetProblem(_Handle):
    """Device-resident PlanarOffsetEstimator (init/initializer.h:72-98): poses [4,3,4], lines [4,n,3], Rg [4,3,3]."""
    _destroy = "pp_planar_destroy"

    def __init__(self, poses, lines, Rg, device=0):
        super().__init__()
        poses, lines, Rg = f64(poses).reshape(4, 12), f64(lines), f64(Rg).reshape(4, 9)
        self.n = int(lines.shape[1])
        assert lines.shape == (4, self.n, 3)
        check(_capi.lib().pp_planar_create(self.n, dp(poses), dp(lines), dp(Rg), int(device), C.byref(self._h)))

    def solve_batch(self, samples):
        samples = np.ascontiguousarray(samples, dtype=np.int32)
        num, k = samples.shape
        out = np.zeros((num, 3))
        check(_capi.lib().pp_planar_solve_batch(self._h, num, k, ptr(samples, _capi.c_ip), dp(out)))
        return out

    def score(self, offsets, threshold):
        offsets = f64(offsets).reshape(-1, 3)
        sc = np.zeros(offsets.shape[0]); inl = np.zeros(offsets.shape[0], dtype=np.int32)
        check(_capi.lib().pp_planar_score(self._h, offsets.shape[0], dp(offsets), float(threshold), dp(sc), ptr(inl, _capi.c_ip)))
        return sc, inl

    def evaluate(self, offsets):
        offsets = f64(offsets).reshape(3)
        err = np.zeros(self.n); X = np.zeros((self.n, 3)); cams = np.zeros((4, 12))
        check(_capi.lib().pp_planar_evaluate(self._h, dp(offsets), dp(err), dp(X), dp(cams)))
        return err, X, cams.reshape(4, 3, 4)

    def lomsac(self, options):
        rep = _capi.LoMsacReport()
        off = np.zeros(3); cams = np.zeros((4, 12)); idx = np.zeros(self.n, dtype=np.int32)
        check(_capi.lib().pp_planar_lomsac(self._h, C.byref(options), C.byref(rep), dp(off), dp(cams), ptr(idx, _capi.c_ip)))
        return rep, off, cams.reshape(4, 3, 4), idx[: rep.num_inlier_indices].copy()


class Pose2dProblem(_Handle):
    """Device-resident AbsolutePose2dEstimator (init/sfm2d.h:99-143): bearings x [n,2], points X [n,2]."""
    _destroy = "pp_pose2d_destroy"

    def __init__(self, x, X, device=0):
        super().__init__()
        x, X = f64(x), f64(X)
        self.n = int(x.shape[0])
        assert x.shape == (self.n, 2) and X.shape == (self.n, 2)
        check(_capi.lib().pp_pose2d_create(self.n, dp(x), dp(X), int(device), C.byref(self._h)))

    def solve_batch(self, samples):
        samples = np.ascontiguousarray(samples, dtype=np.int32)
        num, m = samples.shape
        poses = np.zeros((num, 2, 3))
        check(_capi.lib().pp_pose2d_solve_batch(self._h, num, m, ptr(samples, _capi.c_ip), dp(poses)))
        return poses

    def score(self, poses, threshold):
        poses = f64(poses).reshape(-1, 6)
        sc = np.zeros(poses.shape[0]); inl = np.zeros(poses.shape[0], dtype=np.int32)
        check(_capi.lib().pp_pose2d_score(self._h, poses.shape[0], dp(poses), float(threshold), dp(sc), ptr(inl, _capi.c_ip)))
        return sc, inl

    def lomsac(self, options):
        rep = _capi.LoMsacReport()
        pose = np.zeros((2, 3)); idx = np.zeros(self.n, dtype=np.int32)
        check(_capi.lib().pp_pose2d_lomsac(self._h, C.byref(options), C.byref(rep), dp(pose), ptr(idx, _capi.c_ip)))
        return rep, pose, idx[: rep.num_inlier_indices].copy()


class FourView2dProblem(_Handle):
    """Device-resident bearings of FourView2dEstimator (init/sfm2d.h:48-97): x [4,n,2]."""
    _destroy = "pp_fourview2d_destroy"

    def __init__(self, x, device=0):
        super().__init__()
        x = f64(x)
        self.n = int(x.shape[1])
        assert x.shape == (4, self.n, 2)
        check(_capi.lib().pp_fourview2d_create(self.n, dp(x), int(device), C.byref(self._h)))

    def score(self, cams, threshold):
        cams = f64(cams).reshape(-1, 24)
        sc = np.zeros(cams.shape[0]); inl = np.zeros(cams.shape[0], dtype=np.int32)
        check(_capi.lib().pp_fourview2d_score(self._h, cams.shape[0], dp(cams), float(threshold), dp(sc), ptr(inl, _capi.c_ip)))
        return sc, inl

    def evaluate(self, cams):
        cams = f64(cams).reshape(24)
        err = np.zeros(self.n); X = np.zeros((self.n, 2))
        check(_capi.lib().pp_fourview2d_evaluate(self._h, dp(cams), dp(err), dp(X)))
        return err, X

    def evaluate_points(self, cams, X):
        """EvaluateModelOnPoint against the model's own points X [n,2] (a model refined by LeastSquares) -> errors [n]."""
        cams = f64(cams).reshape(24); X = f64(X)
        assert X.shape == (self.n, 2)
        err = np.zeros(self.n)
        check(_capi.lib().pp_fourview2d_evaluate_points(self._h, dp(cams), dp(X), dp(err)))
        return err

    def minimal_batch(self, samples, frames=None):
        """FourView2dEstimator::MinimalSolver per sample -> (cams [num,16,4,2,3], counts [num])."""
        samples = np.ascontiguousarray(samples, dtype=np.int32)
        num, m = samples.shape
        cams = np.zeros((num, 16, 4, 2, 3)); cnt = np.zeros(num, dtype=np.int32)
        fr = None if frames is None else f64(frames).reshape(12)
        check(_capi.lib().pp_fourview2d_minimal_batch(self._h, num, m, ptr(samples, _capi.c_ip), None if fr is None else dp(fr), dp(cams),
                                                       ptr(cnt, _capi.c_ip)))
        return cams, cnt

    def nonminimal_batch(self, samples, threshold, frames=None):
        """FourView2dEstimator::NonMinimalSolver per sample -> (cams [num,4,2,3], msac score [num], chosen candidate [num])."""
        samples = np.ascontiguousarray(samples, dtype=np.int32)
        num, m = samples.shape
        cams = np.zeros((num, 4, 2, 3)); sc = np.zeros(num); idx = np.zeros(num, dtype=np.int32)
        fr = None if frames is None else f64(frames).reshape(12)
        check(_capi.lib().pp_fourview2d_nonminimal_batch(self._h, num, m, ptr(samples, _capi.c_ip), None if fr is None else dp(fr), float(threshold),
                                                          dp(cams), dp(sc), ptr(idx, _capi.c_ip)))
        return cams, sc, idx

    def least_squares(self, sample, cams, X):
        """FourView2dEstimator::LeastSquares on the model (cams [4,2,3], X [n,2]) -> refined (cams, X)."""
        sample = np.ascontiguousarray(sample, dtype=np.int32)
        cams = f64(cams).reshape(24).copy(); X = f64(X).copy()
        assert X.shape == (self.n, 2)
        check(_capi.lib().pp_fourview2d_least_squares(self._h, len(sample), ptr(sample, _capi.c_ip), dp(cams), dp(X)))
        return cams.reshape(4, 2, 3), X

    def lomsac(self, options, frames=None):
        rep = _capi.LoMsacReport()
        cams = np.zeros(24); X = np.zeros((self.n, 2)); idx = np.zeros(self.n, dtype=np.int32)
        fr = None if frames is None else f64(frames).reshape(12)
        check(_capi.lib().pp_fourview2d_lomsac(self._h, C.byref(options), None if fr is None else dp(fr), C.byref(rep), dp(cams), dp(X),
                                               ptr(idx, _capi.c_ip)))
        return rep, cams.reshape(4, 2, 3), X, idx[: rep.num_inlier_indices].copy()


def fourview2d_default_frames():
    fr = np.zeros(12)
    check(_capi.lib().pp_fourview2d_default_frames(dp(fr)))
    return fr


def camera_num_params(model_id):
    """number of intrinsic parameters of a camera model id (reference base/camera_models.h)"""
    return int(_capi.lib().pp_camera_num_params(int(model_id)))


def triangulation_options(min_tri_angle=0.0, residual_type=0, **ransac_kw):
    o = _capi.TriangulationOptions()
    o.min_tri_angle = float(min_tri_angle); o.residual_type = int(residual_type)
    o.ransac = _capi.options(_capi.RansacOptions, "pp_ransac_options_default", **ransac_kw)
    return o


def triangulate_tracks(track_start, lines, obs_view, proj_matrices, proj_centers, view_camera, camera_model, intr, cam_size, options, device=0):
    """One EstimateTriangulation (estimators/triangulation.cc:111-149) per track, all tracks in one launch.
    Returns (success [T] bool, xyz [T,3], inlier_mask [N] bool, num_trials [T], device_ms)."""
    ts = np.ascontiguousarray(track_start, dtype=np.int32); T = len(ts) - 1
    ln = f64(lines).reshape(-1, 3); ov = np.ascontiguousarray(obs_view, dtype=np.int32)
    P = f64(proj_matrices).reshape(-1, 12); ctr = f64(proj_centers).reshape(-1, 3); vc = np.ascontiguousarray(view_camera, dtype=np.int32)
    cm = np.ascontiguousarray(camera_model, dtype=np.int32); it = f64(intr).reshape(len(cm), 12); cs = np.ascontiguousarray(cam_size, dtype=np.int32).reshape(len(cm), 2)
    ok = np.zeros(T, dtype=np.uint8); xyz = np.zeros((T, 3)); mask = np.zeros(max(len(ov), 1), dtype=np.uint8); nt = np.zeros(T, dtype=np.int32)
    ms = C.c_float(0)
    check(_capi.lib().pp_triangulate_tracks(int(device), T, ptr(ts, _capi.c_ip), dp(ln), ptr(ov, _capi.c_ip), P.shape[0], dp(P), dp(ctr), ptr(vc, _capi.c_ip), len(cm),
                                            ptr(cm, _capi.c_ip), dp(it), ptr(cs, _capi.c_ip), C.byref(options), ptr(ok, _capi.c_u8p), dp(xyz), ptr(mask, _capi.c_u8p),
                                            ptr(nt, _capi.c_ip), C.byref(ms)))
    return ok.astype(bool), xyz, mask[: len(ov)].astype(bool), nt, float(ms.value)


def tracks_options(**kw):
    return _capi.options(_capi.TracksOptions, "pp_tracks_options_default", **kw)


def tracks_image_options(**kw):
    return _capi.options(_capi.TracksImageOptions, "pp_tracks_image_options_default", **kw)


def local_bundle_options(**kw):
    return _capi.options(_capi.LocalBundleOptions, "pp_local_bundle_options_default", **kw)


def next_image_options(**kw):
    return _capi.options(_capi.NextImageOptions, "pp_next_image_options_default", **kw)


def init_sets_options(**kw):
    return _capi.options(_capi.InitSetsOptions, "pp_init_sets_options_default", **kw)


_TRACKS_FIELDS = (("poses", np.float64, dp), ("pose_camera", np.int32, None), ("camera_model", np.int32, None), ("intr", np.float64, dp),
                  ("cam_size", np.int32, None), ("camera_skip", np.uint8, None), ("image_registered", np.uint8, None), ("lines", np.float64, dp),
                  ("line_image", np.int32, None), ("line_point", np.int32, None), ("corr_start", np.int32, None), ("corr_line", np.int32, None),
                  ("points", np.float64, dp), ("track_start", np.int32, None), ("track_line", np.int32, None))


def tracks_desc(flat, keep):
    """pp_tracks_desc of a flat dict (IncrementalTriangulator.flatten's first result; camera_skip / image_registered may be missing or None)"""
    d = _capi.TracksDesc()
    d.num_images, d.num_cameras, d.num_points = int(np.shape(flat["poses"])[0]), int(np.shape(flat["intr"])[0]), int(np.shape(flat["points"])[0])
    d.num_lines, d.num_corrs = int(len(flat["line_image"])), int(len(flat["corr_line"]))
    types = {np.int32: _capi.c_ip, np.uint8: _capi.c_u8p}
    for name, dt, _ in _TRACKS_FIELDS:
        a = flat.get(name)
        if a is None:
            continue
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        setattr(d, name, dp(a) if dt is np.float64 else ptr(a, types[dt]))
    return d


class TracksProblem(_Handle):
    """pp_tracks_handle: the flattened state of the triangulator on the device; complete() / merge() advance it, state() reads it."""
    _destroy = "pp_tracks_destroy"

    def __init__(self, flat, device=0):
        self._keep = []
        super().__init__()
        self.num_lines = int(len(flat["line_image"]))
        self.num_images, self.num_cameras = int(np.shape(flat["poses"])[0]), int(np.shape(flat["intr"])[0])
        self._max_image_corrs = 0      # the longest correspondence list an image's lines can give (pp_tracks_estimate_image_pose's capacity)
        if self.num_lines:
            per_line = np.diff(np.asarray(flat["corr_start"], dtype=np.int64))
            self._max_image_corrs = int(np.bincount(np.asarray(flat["line_image"], dtype=np.int64), weights=per_line, minlength=self.num_images).max())
        d = tracks_desc(flat, self._keep)
        check(_capi.lib().pp_tracks_create(C.byref(d), int(device), C.byref(self._h)))

    def num_points(self):
        n, t = C.c_int32(), C.c_int64()
        check(_capi.lib().pp_tracks_get_state(self._h, C.byref(n), C.byref(t), None, None, None, None, None, 0, 0))
        return n.value, t.value

    def _subset(self, point_subset):
        return None if point_subset is None else np.ascontiguousarray(point_subset, dtype=np.uint8)

    def complete(self, options=None, point_subset=None):
        """-> (report, pairs [n, 2] (point, line) in the order the reference appends them)"""
        o = options or tracks_options()
        sub = self._subset(point_subset)
        assert sub is None or len(sub) == self.num_points()[0]
        cap = self.num_lines
        ap, al = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        rep = _capi.TracksReport()
        check(_capi.lib().pp_tracks_complete(self._h, C.byref(o), ptr(sub, _capi.c_u8p), C.byref(rep), ptr(ap, _capi.c_ip), ptr(al, _capi.c_ip), cap))
        n = int(rep.num_entries)
        return rep, np.stack([ap[:n], al[:n]], axis=1)

    def merge(self, options=None, point_subset=None):
        """-> (report, merges [n, 3] (a, b, new index) in order)"""
        o = options or tracks_options()
        sub = self._subset(point_subset)
        cap = self.num_points()[0]
        assert sub is None or len(sub) == cap
        a, b, m = (np.zeros(cap, dtype=np.int32) for _ in range(3))
        rep = _capi.TracksReport()
        check(_capi.lib().pp_tracks_merge(self._h, C.byref(o), ptr(sub, _capi.c_u8p), C.byref(rep), ptr(a, _capi.c_ip), ptr(b, _capi.c_ip), ptr(m, _capi.c_ip), cap))
        n = int(rep.num_entries)
        return rep, np.stack([a[:n], b[:n], m[:n]], axis=1)

    def _image_call(self, fn, options, image, *extra):
        o = options or tracks_image_options()
        cap = 2 * self.num_lines      # every event gives a free line its point, and a line gets one once: L would do
        ep, el = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        rep = _capi.TracksImageReport()
        check(fn(self._h, C.byref(o), int(image), *extra, C.byref(rep), ptr(ep, _capi.c_ip), ptr(el, _capi.c_ip), cap))
        n = int(rep.num_entries)
        return rep, np.stack([ep[:n], el[:n]], axis=1)

    def triangulate_image(self, image, options=None, line_aligned=None):
        """TriangulateImage for image index `image` -> (report, events [n, 2] (point, line) in the order the reference's Reconstruction receives them;
        new points take the next unused indices, their positions are in state()["points"]).  line_aligned: [L] flags or None."""
        al = None if line_aligned is None else np.ascontiguousarray(line_aligned, dtype=np.uint8)
        assert al is None or len(al) == self.num_lines
        return self._image_call(_capi.lib().pp_tracks_triangulate_image, options, image, ptr(al, _capi.c_u8p))

    def complete_image(self, image, options=None):
        """CompleteImage for image index `image` -> (report, events) as triangulate_image"""
        return self._image_call(_capi.lib().pp_tracks_complete_image, options, image)

    def find_local_bundle(self, image, options=None):
        """FindLocalBundle for image index `image` -> (report, bundle [n] image indices in the reference's order,
        overlap dict(image [m], count [m], tri_angle [m] radians, -1 where the sequential loop never asked)).  The state does not change."""
        o = options or local_bundle_options()
        Cn = self.num_images
        bundle, oi, oc, oa = np.zeros(Cn, dtype=np.int32), np.zeros(Cn, dtype=np.int32), np.zeros(Cn, dtype=np.int32), np.zeros(Cn)
        rep = _capi.LocalBundleReport()
        check(_capi.lib().pp_tracks_find_local_bundle(self._h, C.byref(o), int(image), C.byref(rep), ptr(bundle, _capi.c_ip), Cn, ptr(oi, _capi.c_ip),
                                                      ptr(oc, _capi.c_ip), dp(oa)))
        m = int(rep.num_overlapping)
        return rep, bundle[: int(rep.num_selected)].copy(), dict(image=oi[:m].copy(), count=oc[:m].copy(), tri_angle=oa[:m].copy())

    def find_next_images(self, options=None, num_reg_trials=None, filtered=None):
        """FindNextImages -> (report, ranked [n] image indices (first bucket, then second bucket), num_visible [C], num_observations [C]).
        num_reg_trials [C] / filtered [C]: the caller's num_reg_trials_ / filtered_images_ (None: none).  The state does not change."""
        o = options or next_image_options()
        Cn = self.num_images
        nt = None if num_reg_trials is None else np.ascontiguousarray(num_reg_trials, dtype=np.int32).reshape(Cn)
        fi = None if filtered is None else np.ascontiguousarray(filtered, dtype=np.uint8).reshape(Cn)
        ranked, vis, obs = np.zeros(Cn, dtype=np.int32), np.zeros(Cn, dtype=np.int32), np.zeros(Cn, dtype=np.int32)
        rep = _capi.NextImageReport()
        check(_capi.lib().pp_tracks_find_next_images(self._h, C.byref(o), ptr(nt, _capi.c_ip), ptr(fi, _capi.c_u8p), C.byref(rep), ptr(ranked, _capi.c_ip), Cn,
                                                     ptr(vis, _capi.c_ip), ptr(obs, _capi.c_ip)))
        return rep, ranked[: int(rep.num_ranked)].copy(), vis, obs

    def estimate_image_pose(self, image, ransac, options=None, line_aligned=None):
        """RegisterNextImage up to the pose refinement (visibility gate, 2D-3D search, P6L RANSAC, the gates) for the unregistered image index `image`
        -> (report, pose [7] (qvec, tvec), corrs [n, 2] (line, point) in the reference's order, inlier_mask [n]).  report.failure says which
        `return false` was taken (0: a pose was found).  ransac: a pp_ransac_options (device.ransac_options).  The state does not change."""
        o = options or next_image_options()
        al = None if line_aligned is None else np.ascontiguousarray(line_aligned, dtype=np.uint8)
        assert al is None or len(al) == self.num_lines
        cap = self._max_image_corrs
        cl, cp, mask, pose = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.uint8), np.zeros(7)
        rep = _capi.ImagePoseReport()
        check(_capi.lib().pp_tracks_estimate_image_pose(self._h, C.byref(o), C.byref(ransac), int(image), ptr(al, _capi.c_u8p), C.byref(rep), dp(pose),
                                                        ptr(cl, _capi.c_ip), ptr(cp, _capi.c_ip), ptr(mask, _capi.c_u8p), cap))
        n = int(rep.num_corrs)
        return rep, pose, np.stack([cl[:n], cp[:n]], axis=1), mask[:n].copy()

    def register_image(self, image, pose, corrs, inlier_mask=None):
        """The commit of RegisterNextImage: image index `image` becomes registered with pose [7]; the inliers of corrs [n, 2] (line, point) whose line
        has no point yet get their observation -> events [m, 2] (point, line) in list order."""
        pose = f64(pose).reshape(7)
        corrs = np.ascontiguousarray(corrs, dtype=np.int32).reshape(-1, 2)
        n = corrs.shape[0]
        cl, cp = np.ascontiguousarray(corrs[:, 0]), np.ascontiguousarray(corrs[:, 1])
        mask = None if inlier_mask is None else np.ascontiguousarray(inlier_mask, dtype=np.uint8).reshape(n)
        ep, el = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        added = C.c_int64()
        check(_capi.lib().pp_tracks_register_image(self._h, int(image), dp(pose), n, ptr(cl, _capi.c_ip) if n else None, ptr(cp, _capi.c_ip) if n else None,
                                                   ptr(mask, _capi.c_u8p), C.byref(added), ptr(ep, _capi.c_ip), ptr(el, _capi.c_ip), n))
        m = int(added.value)
        return np.stack([ep[:m], el[:m]], axis=1)

    def find_initial_sets(self, line_aligned, check_images, image_subset=None, options=None, capacity=None):
        """The image sets of RegisterInitialLineImages worth a four-view solve, over the lines of the image indices `check_images`
        -> (report, sets: best first, each dict(images [4], num_aligned, num_random, aligned [a, 4], random [r, 4]: handle line numbers per track in the
        order of `images`, each list in ascending lexicographic order)).  line_aligned [L] flags; image_subset [C] flags or None = all.
        capacity: tracks to make room for (None: a first guess, and a second call when the report asks for more; a given capacity is not grown -
        the lists then hold what fitted).  The state does not change; a handle without points or registered images will do."""
        o = options or init_sets_options()
        al = np.ascontiguousarray(line_aligned, dtype=np.uint8).reshape(-1)
        assert len(al) == self.num_lines
        sub = None if image_subset is None else np.ascontiguousarray(image_subset, dtype=np.uint8).reshape(self.num_images)
        chk = np.ascontiguousarray(check_images, dtype=np.int32).reshape(-1)
        ns = int(o.max_num_sets)
        cap = 1 << 14 if capacity is None else int(capacity)
        while True:
            si, sa, sr = np.zeros((max(ns, 1), 4), dtype=np.int32), np.zeros(max(ns, 1), dtype=np.int32), np.zeros(max(ns, 1), dtype=np.int32)
            ts, tl = np.zeros(2 * max(ns, 1) + 1, dtype=np.int64), np.zeros((max(cap, 1), 4), dtype=np.int32)
            rep = _capi.InitSetsReport()
            check(_capi.lib().pp_tracks_find_initial_sets(self._h, C.byref(o), ptr(al, _capi.c_u8p), ptr(sub, _capi.c_u8p), ptr(chk, _capi.c_ip) if len(chk) else None,
                                                          len(chk), C.byref(rep), ptr(si, _capi.c_ip), ptr(sa, _capi.c_ip), ptr(sr, _capi.c_ip),
                                                          ts.ctypes.data_as(C.POINTER(C.c_int64)), ptr(tl, _capi.c_ip), cap))
            if capacity is not None or rep.num_track_entries <= cap:
                break
            cap = int(rep.num_track_entries)
        sets = []
        for k in range(int(rep.num_returned)):
            a0, a1, r1 = (min(int(x), cap) for x in ts[2 * k: 2 * k + 3])
            sets.append(dict(images=si[k].copy(), num_aligned=int(sa[k]), num_random=int(sr[k]), aligned=tl[a0:a1].copy(), random=tl[a1:r1].copy()))
        return rep, sets

    def bundle_setup(self, image_flags, tvec_const_mask=None, camera_const=None, camera_subset_mask=None, variable_points=(), constant_points=(),
                     obs_capacity=None, point_capacity=None):
        """BundleAdjuster::SetUp on the handle (pp_tracks_bundle_setup) -> (report, dict(lines [M, 3], obs_pose [M], obs_point [M], obs_line [M],
        pose_image [C'], pose_const, pose_tvec_mask, pose_camera, point_index [P''], point_const, points [P'', 3], camera_index [K'],
        camera_const_mask)): the arrays of a pp_ba_problem_desc and, per pose / point / camera of the problem, its handle index.
        image_flags [C]: _capi.PP_BUNDLE_IMAGE | PP_BUNDLE_CONST_POSE; tvec_const_mask [C], camera_const [K], camera_subset_mask [K] or None;
        the point lists in the order they are to be visited.  The state does not change."""
        Cn, Kn = self.num_images, self.num_cameras
        fl = np.ascontiguousarray(image_flags, dtype=np.uint8).reshape(Cn)
        tm = None if tvec_const_mask is None else np.ascontiguousarray(tvec_const_mask, dtype=np.uint8).reshape(Cn)
        cc = None if camera_const is None else np.ascontiguousarray(camera_const, dtype=np.uint8).reshape(Kn)
        cs = None if camera_subset_mask is None else np.ascontiguousarray(camera_subset_mask, dtype=np.uint16).reshape(Kn)
        vp = np.ascontiguousarray(variable_points, dtype=np.int32).reshape(-1); cp = np.ascontiguousarray(constant_points, dtype=np.int32).reshape(-1)
        if obs_capacity is None or point_capacity is None:
            P, T = self.num_points()
            obs_capacity = T if obs_capacity is None else obs_capacity
            point_capacity = P if point_capacity is None else point_capacity
        M, Pn = max(int(obs_capacity), 1), max(int(point_capacity), 1)
        cfg = _capi.BundleConfig(ptr(fl, _capi.c_u8p), ptr(tm, _capi.c_u8p), ptr(cc, _capi.c_u8p), ptr(cs, _capi.c_u16p), ptr(vp, _capi.c_ip) if len(vp) else None,
                                 ptr(cp, _capi.c_ip) if len(cp) else None, len(vp), len(cp))
        lines, obs_pose, obs_point, obs_line = np.zeros((M, 3)), np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.int32)
        pose_image, pose_const, pose_tvec = np.zeros(max(Cn, 1), dtype=np.int32), np.zeros(max(Cn, 1), dtype=np.uint8), np.zeros(max(Cn, 1), dtype=np.uint8)
        pose_camera = np.zeros(max(Cn, 1), dtype=np.int32)
        point_index, point_const, points = np.zeros(Pn, dtype=np.int32), np.zeros(Pn, dtype=np.uint8), np.zeros((Pn, 3))
        camera_index, camera_mask = np.zeros(max(Kn, 1), dtype=np.int32), np.zeros(max(Kn, 1), dtype=np.uint16)
        rep = _capi.BundleSetupReport()
        ip = _capi.c_ip
        check(_capi.lib().pp_tracks_bundle_setup(self._h, C.byref(cfg), C.byref(rep), dp(lines), ptr(obs_pose, ip), ptr(obs_point, ip), ptr(obs_line, ip),
                                                 int(obs_capacity), ptr(pose_image, ip), ptr(pose_const, _capi.c_u8p), ptr(pose_tvec, _capi.c_u8p),
                                                 ptr(pose_camera, ip), ptr(point_index, ip), ptr(point_const, _capi.c_u8p), dp(points), int(point_capacity),
                                                 ptr(camera_index, ip), ptr(camera_mask, _capi.c_u16p)))
        m, c, p, k = int(rep.num_obs), int(rep.num_poses), int(rep.num_points), int(rep.num_cameras)
        return rep, dict(lines=lines[:m], obs_pose=obs_pose[:m], obs_point=obs_point[:m], obs_line=obs_line[:m], pose_image=pose_image[:c],
                         pose_const=pose_const[:c], pose_tvec_mask=pose_tvec[:c], pose_camera=pose_camera[:c], point_index=point_index[:p],
                         point_const=point_const[:p], points=points[:p], camera_index=camera_index[:k], camera_const_mask=camera_mask[:k])

    def _filter_call(self, fn, args, trailing=()):
        cap = self.num_lines + self.num_points()[0]      # a line loses its point once, a point is deleted once
        ep, el = np.zeros(max(cap, 1), dtype=np.int32), np.zeros(max(cap, 1), dtype=np.int32)
        rep = _capi.TracksFilterReport()
        check(fn(self._h, *args, C.byref(rep), ptr(ep, _capi.c_ip), ptr(el, _capi.c_ip), cap, *trailing))
        n = int(rep.num_entries)
        return rep, np.stack([ep[:n], el[:n]], axis=1)

    def filter_points(self, max_reproj_error, min_tri_angle_deg, line_aligned=None, point_subset=None, image_subset=None):
        """FilterPoints3D (point_subset [P'] flags) / FilterPoints3DInImages (image_subset [C] flags) / FilterAllPoints3D (neither) on the handle
        -> (report, events [n, 2]: (point, line) for one deleted observation, (point, -1) for a deleted point, in the reference's order,
        point_error [P']: Point3D.error of the points the filter kept, -1 elsewhere)"""
        o = _capi.FilterOptions(float(max_reproj_error), float(min_tri_angle_deg))
        al = None if line_aligned is None else np.ascontiguousarray(line_aligned, dtype=np.uint8)
        assert al is None or len(al) == self.num_lines
        P = self.num_points()[0]
        sub = self._subset(point_subset)
        img = None if image_subset is None else np.ascontiguousarray(image_subset, dtype=np.uint8)
        assert (sub is None or len(sub) == P) and (img is None or len(img) == self.num_images)
        pe = np.full(max(P, 1), -1.0)
        rep, events = self._filter_call(_capi.lib().pp_tracks_filter_points, (C.byref(o), ptr(al, _capi.c_u8p), ptr(sub, _capi.c_u8p), ptr(img, _capi.c_u8p)),
                                        trailing=(dp(pe),))
        return rep, events, pe[:P]

    def filter_negative_depth(self, image_order):
        """FilterObservationsWithNegativeDepth; image_order: the registered image indices in registration order -> (report, events as filter_points)"""
        order = np.ascontiguousarray(image_order, dtype=np.int32).reshape(-1)
        return self._filter_call(_capi.lib().pp_tracks_filter_negative_depth, (ptr(order, _capi.c_ip) if len(order) else None, len(order)))

    def filter_images(self, image_order):
        """FilterImages: the registered images without a point or with a flagged camera are de-registered -> (report, events, filtered image indices)"""
        order = np.ascontiguousarray(image_order, dtype=np.int32).reshape(-1)
        out = np.zeros(max(self.num_images, 1), dtype=np.int32)
        rep, events = self._filter_call(_capi.lib().pp_tracks_filter_images, (ptr(order, _capi.c_ip) if len(order) else None, len(order), ptr(out, _capi.c_ip)))
        return rep, events, out[: int(rep.images_filtered)].copy()

    def update(self, image_idx=(), poses=None, point_idx=(), xyz=None, intr=None, camera_skip=None):
        """New poses [n, 7] of the images image_idx, positions [m, 3] of the points point_idx, intrinsics [K, 12] with camera_skip [K] or None
        (after a bundle adjustment); every later call sees them."""
        ii = np.ascontiguousarray(image_idx, dtype=np.int32).reshape(-1); pi = np.ascontiguousarray(point_idx, dtype=np.int32).reshape(-1)
        ps = None if len(ii) == 0 else f64(poses).reshape(len(ii), 7)
        xs = None if len(pi) == 0 else f64(xyz).reshape(len(pi), 3)
        it = None if intr is None else f64(intr).reshape(self.num_cameras, _capi.CAM_STRIDE)
        sk = None if camera_skip is None else np.ascontiguousarray(camera_skip, dtype=np.uint8).reshape(self.num_cameras)
        check(_capi.lib().pp_tracks_update(self._h, len(ii), ptr(ii, _capi.c_ip) if len(ii) else None, dp(ps), len(pi), ptr(pi, _capi.c_ip) if len(pi) else None,
                                           dp(xs), dp(it), ptr(sk, _capi.c_u8p)))

    def state(self):
        """-> dict(line_point [L], points [P', 3], deleted [P'], track_start [P' + 1], track_line)"""
        P, T = self.num_points()
        lp, pts, dele = np.zeros(self.num_lines, dtype=np.int32), np.zeros((P, 3)), np.zeros(P, dtype=np.uint8)
        ts, tl = np.zeros(P + 1, dtype=np.int32), np.zeros(T, dtype=np.int32)
        n, t = C.c_int32(), C.c_int64()
        check(_capi.lib().pp_tracks_get_state(self._h, C.byref(n), C.byref(t), ptr(lp, _capi.c_ip), dp(pts), ptr(dele, _capi.c_u8p), ptr(ts, _capi.c_ip),
                                              ptr(tl, _capi.c_ip), P, T))
        return dict(line_point=lp, points=pts, deleted=dele, track_start=ts, track_line=tl)


def sift_match_options(**kw):
    return _capi.options(_capi.SiftMatchOptions, "pp_sift_match_options_default", **kw)


def sift_match_thresholds(options=None):
    """-> (d_min, table): the integers the device compares (pp_sift_match_thresholds; host only)"""
    o = options or sift_match_options()
    d_min, count = C.c_int32(), C.c_int64()
    check(_capi.lib().pp_sift_match_thresholds(C.byref(o), C.byref(d_min), None, 0, C.byref(count)))
    table = np.zeros(count.value, dtype=np.int32)
    check(_capi.lib().pp_sift_match_thresholds(C.byref(o), C.byref(d_min), ptr(table, _capi.c_ip), count.value, C.byref(count)))
    return d_min.value, table


class SiftMatcher(_Handle):
    """pp_sift_handle: the descriptors ([N_k, 128] uint8 each) of a list of images on the device; match_pairs() is MatchSiftFeaturesCPUBruteForce for a
    list of pairs of positions in that list, top2() the one-way scan underneath it.  from_handle() wraps a handle that was filled on the device."""
    _destroy = "pp_sift_destroy"

    def __init__(self, descriptors_by_image, device=0):
        super().__init__()
        arrays = []
        for d in descriptors_by_image:
            d = np.asarray(d)
            if d.dtype != np.uint8 or (d.size and (d.ndim != 2 or d.shape[1] != 128)):
                raise ValueError("descriptors are [N, 128] uint8 arrays")
            arrays.append(np.ascontiguousarray(d).reshape(-1, 128))
        self.num_features = [int(a.shape[0]) for a in arrays]
        self.num_images = len(arrays)
        start = np.zeros(self.num_images + 1, dtype=np.int64)
        start[1:] = np.cumsum(self.num_features)
        flat = np.concatenate(arrays) if arrays else np.zeros((0, 128), dtype=np.uint8)
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        check(_capi.lib().pp_sift_create(self.num_images, ptr(start, C.POINTER(C.c_int64)), ptr(flat, _capi.c_u8p) if flat.size else None, int(device),
                                         C.byref(self._h)))

    @classmethod
    def from_handle(cls, handle, offsets):
        """a pp_sift_handle this class did not create (SiftExtractor.extract_to_matcher), owned from here on; offsets [num_images + 1]: image k holds
        the rows offsets[k] .. offsets[k + 1]"""
        self = cls.__new__(cls)
        _Handle.__init__(self)
        self._h = handle
        self.num_features = [int(b - a) for a, b in zip(offsets[:-1], offsets[1:])]
        self.num_images = len(self.num_features)
        return self

    def descriptors(self, image):
        """-> [N, 128] uint8: the descriptor rows of one image as they were given, or as extract_to_matcher made them (pp_sift_get_descriptors)"""
        n = self.num_features[image]
        out, num = np.zeros((max(n, 1), 128), dtype=np.uint8), C.c_int64()
        check(_capi.lib().pp_sift_get_descriptors(self._h, int(image), ptr(out, _capi.c_u8p), n, C.byref(num)))
        return out[:num.value]

    def capacity(self, pairs, cross_check=True):
        """the number of matches that always suffices for these pairs"""
        n = self.num_features
        return int(sum(min(n[a], n[b]) if cross_check else (n[a] if n[b] else 0) for a, b in pairs))

    def match_pairs(self, pairs, options=None, capacity=None):
        """-> (report, list of [n_p, 2] int32 arrays, one per pair, in the reference's order)"""
        o = options or sift_match_options()
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        num = int(pr.shape[0])
        if num and (pr.min() < 0 or pr.max() >= self.num_images):
            raise ValueError("a pair names an image that is not there")
        cap = self.capacity(pr, bool(o.cross_check)) if capacity is None else int(capacity)
        start, out = np.zeros(num + 1, dtype=np.int64), np.zeros((max(cap, 1), 2), dtype=np.int32)
        rep = _capi.SiftMatchReport()
        check(_capi.lib().pp_sift_match_pairs(self._h, C.byref(o), num, ptr(pr, _capi.c_ip) if num else None, C.byref(rep), ptr(start, C.POINTER(C.c_int64)),
                                              ptr(out, _capi.c_ip), cap))
        return rep, [out[start[p]:start[p + 1]].copy() for p in range(num)]

    def top2(self, image1, image2):
        """-> (best_j, best, second), [N1] int32 each: K17a for the direction image1 -> image2"""
        n1 = self.num_features[image1]
        bj, b, s = (np.zeros(max(n1, 1), dtype=np.int32) for _ in range(3))
        check(_capi.lib().pp_sift_top2(self._h, int(image1), int(image2), ptr(bj, _capi.c_ip), ptr(b, _capi.c_ip), ptr(s, _capi.c_ip)))
        return bj[:n1], b[:n1], s[:n1]


class CorrGraphBuilder(_Handle):
    """pp_corr_graph_handle: the images of a problem (their line counts, in ascending image-id order) on the device; build() turns match lists into the
    corr_start / corr_line CSR of pp_tracks_desc by the rules of DatabaseCache::Load and CorrespondenceGraph::AddCorrespondences, get() reads it back."""
    _destroy = "pp_corr_graph_destroy"

    def __init__(self, num_lines_by_image, device=0):
        super().__init__()
        self.num_lines = np.ascontiguousarray(num_lines_by_image, dtype=np.int32).reshape(-1)
        self.num_images = int(self.num_lines.shape[0])
        self.line_start = np.zeros(self.num_images + 1, dtype=np.int64)
        self.line_start[1:] = np.cumsum(self.num_lines, dtype=np.int64)
        self.num_pairs = None
        check(_capi.lib().pp_corr_graph_create(self.num_images, ptr(self.num_lines, _capi.c_ip) if self.num_images else None, int(device), C.byref(self._h)))

    def build(self, pairs, matches, min_num_matches=15):
        """pairs: [num_pairs, 2] image positions; matches: one [n_p, 2] array per pair, or (match_start [num_pairs + 1], flat [n, 2]) as
        pp_sift_match_pairs writes them -> report"""
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        num = int(pr.shape[0])
        if isinstance(matches, tuple):
            start = np.ascontiguousarray(matches[0], dtype=np.int64).reshape(-1)
            flat = np.ascontiguousarray(matches[1], dtype=np.int32).reshape(-1, 2)
        else:
            arrays = [np.asarray(m, dtype=np.int32).reshape(-1, 2) for m in matches]
            start = np.zeros(num + 1, dtype=np.int64)
            start[1:] = np.cumsum([a.shape[0] for a in arrays], dtype=np.int64)
            flat = np.ascontiguousarray(np.concatenate(arrays) if arrays else np.zeros((0, 2), dtype=np.int32))
        if start.shape[0] != num + 1:
            raise ValueError("one match list per pair")
        rep = _capi.CorrGraphReport()
        check(_capi.lib().pp_corr_graph_build(self._h, int(min_num_matches), num, ptr(pr, _capi.c_ip) if num else None, ptr(start, C.POINTER(C.c_int64)),
                                              ptr(flat, _capi.c_ip) if flat.size else None, C.byref(rep)))
        self.num_pairs = num
        return rep

    def get(self):
        """the last build -> dict(corr_start [L + 1], corr_line [E], image_connected, image_num_observations, image_num_correspondences [num_images])"""
        L, E = C.c_int64(), C.c_int64()
        check(_capi.lib().pp_corr_graph_num_entries(self._h, C.byref(L), C.byref(E)))
        n = max(self.num_images, 1)
        corr_start, corr_line = np.zeros(L.value + 1, dtype=np.int32), np.zeros(max(E.value, 1), dtype=np.int32)
        connected, obs, corrs = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        check(_capi.lib().pp_corr_graph_get(self._h, ptr(corr_start, _capi.c_ip), ptr(corr_line, _capi.c_ip), E.value, ptr(connected, _capi.c_u8p),
                                            ptr(obs, _capi.c_ip), ptr(corrs, _capi.c_ip)))
        k = self.num_images
        return dict(corr_start=corr_start, corr_line=corr_line[:E.value], image_connected=connected[:k], image_num_observations=obs[:k],
                    image_num_correspondences=corrs[:k])

    def pair_counts(self):
        """the accepted matches per pair of the last build, in its input order"""
        out = np.zeros(max(self.num_pairs or 0, 1), dtype=np.int32)
        check(_capi.lib().pp_corr_graph_pair_counts(self._h, ptr(out, _capi.c_ip)))
        return out[:self.num_pairs or 0]


class PairSelector(_Handle):
    """pp_pairs_handle (K20): spatial() and transitive() select image pairs on the device and return them; the handle keeps the last result."""
    _destroy = "pp_pairs_destroy"

    def __init__(self, device=0):
        super().__init__()
        check(_capi.lib().pp_pairs_create(int(device), C.byref(self._h)))

    def num(self):
        n = C.c_int64()
        check(_capi.lib().pp_pairs_num(self._h, C.byref(n)))
        return n.value

    def get(self, want_sqdist=True):
        """the last result -> (pairs [n, 2] int32 positions, sqdist [n] float32 or None)"""
        n = self.num()
        pairs = np.zeros((max(n, 1), 2), dtype=np.int32)
        sqdist = np.zeros(max(n, 1), dtype=np.float32) if want_sqdist else None
        check(_capi.lib().pp_pairs_get(self._h, ptr(pairs, _capi.c_ip), ptr(sqdist, C.POINTER(C.c_float)), n))
        return pairs[:n], None if sqdist is None else sqdist[:n]

    def spatial(self, xyz, max_num_neighbors, max_distance):
        """xyz [m, 3] float32 -> (report, pairs [n, 2] of location indices, sqdist [n] float32)"""
        loc = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        rep = _capi.PairsReport()
        check(_capi.lib().pp_pairs_spatial(self._h, int(loc.shape[0]), ptr(loc, C.POINTER(C.c_float)) if loc.size else None, int(max_num_neighbors),
                                           float(max_distance), C.byref(rep)))
        pairs, sqdist = self.get()
        return rep, pairs, sqdist

    def transitive(self, num_images, matched_pairs, tried_pairs=()):
        """matched_pairs / tried_pairs [k, 2] image positions (the matched ones count as tried) -> (report, pairs [n, 2], a < c, ascending)"""
        matched = np.ascontiguousarray(matched_pairs, dtype=np.int32).reshape(-1, 2)
        tried = np.ascontiguousarray(tried_pairs, dtype=np.int32).reshape(-1, 2)
        rep = _capi.PairsReport()
        check(_capi.lib().pp_pairs_transitive(self._h, int(num_images), int(matched.shape[0]), ptr(matched, _capi.c_ip) if matched.size else None,
                                              int(tried.shape[0]), ptr(tried, _capi.c_ip) if tried.size else None, C.byref(rep)))
        return rep, self.get(want_sqdist=False)[0]


def sift_extract_options(**kw):
    return _capi.options(_capi.SiftExtractOptions, "pp_sift_extract_options_default", **kw)


class SiftExtractor(_Handle):
    """pp_sift_extractor_handle (K21): extract() is ExtractSiftFeaturesCPU for one grey image; the handle's workspace grows to the largest image seen
    and keeps the pyramid of the last extraction for stage(), candidates() and features().  extract_batch() is the same for a sequence of images in
    one call (K23); batch_features(i) reads its results.  extract_to_matcher() is extract_batch() with a SiftMatcher as the way out (K24): the
    descriptors of the kept features are written on the device where the matcher reads them."""
    _destroy = "pp_sift_extractor_destroy"

    def __init__(self, device=0):
        super().__init__()
        check(_capi.lib().pp_sift_extractor_create(int(device), C.byref(self._h)))
        self.last_report = None
        self.last_batch_report = None

    def extract(self, image, options=None, want_descriptors=True, capacity=None):
        """image [H, W] uint8 -> (keypoints [N, 4] float32 (x, y, scale, orientation), descriptors [N, 128] uint8 in UBC order or None, report).
        capacity None: the call is repeated with the reported need when the first guess was too small."""
        im = np.asarray(image)
        if im.dtype != np.uint8 or im.ndim != 2:
            raise ValueError("the image is an [H, W] uint8 array")
        im = np.ascontiguousarray(im)
        o = options or sift_extract_options()
        guess = min(2 * int(o.max_num_features), 1 << 16) if capacity is None else int(capacity)
        for cap in (guess, None):
            num, rep = C.c_int64(), _capi.SiftExtractReport()
            if cap is None:
                cap = int(self.last_report.num_features)
            kp = np.zeros((max(cap, 1), 4), dtype=np.float32)
            desc = np.zeros((max(cap, 1), 128), dtype=np.uint8) if want_descriptors else None
            rc = _capi.lib().pp_sift_extract(self._h, C.byref(o), int(im.shape[1]), int(im.shape[0]), ptr(im, _capi.c_u8p), C.byref(rep), cap,
                                             ptr(kp, C.POINTER(C.c_float)), ptr(desc, _capi.c_u8p), C.byref(num))
            self.last_report = rep
            if rc == 0 or capacity is not None or num.value <= cap:
                break
        check(rc)
        n = num.value
        return kp[:n].copy(), None if desc is None else desc[:n].copy(), rep

    def stage(self, kind, octave, level):
        """one level of the last extraction's pyramid: kind _capi.SIFT_STAGE_* -> [h, w] float32 ([h, w, 2] modulus / angle for the gradient)"""
        w, h = C.c_int32(), C.c_int32()
        per = 2 if kind == _capi.SIFT_STAGE_GRADIENT else 1
        out = np.zeros(1, dtype=np.float32)
        rc = _capi.lib().pp_sift_extract_stage(self._h, int(kind), int(octave), int(level), ptr(out, C.POINTER(C.c_float)), 0, C.byref(w), C.byref(h))
        if w.value <= 0 or h.value <= 0:
            check(rc)
        out = np.zeros(per * w.value * h.value, dtype=np.float32)
        check(_capi.lib().pp_sift_extract_stage(self._h, int(kind), int(octave), int(level), ptr(out, C.POINTER(C.c_float)), out.size, C.byref(w), C.byref(h)))
        return out.reshape(h.value, w.value, 2) if per == 2 else out.reshape(h.value, w.value)

    def candidates(self, octave):
        """the unrefined extrema of one octave in scan order -> [M, 3] int32 (x, y, level)"""
        num = C.c_int64()
        _capi.lib().pp_sift_extract_candidates(self._h, int(octave), None, 0, C.byref(num))
        out = np.zeros((max(num.value, 1), 3), dtype=np.int32)
        check(_capi.lib().pp_sift_extract_candidates(self._h, int(octave), ptr(out, _capi.c_ip), num.value, C.byref(num)))
        return out[:num.value]

    def features(self):
        """every feature of the last extraction before the max_num_features cut -> (raw [F, 128] float32 in VLFeat's order before the last
        normalisation, octave_level [F, 2] int32, angles [F] float64); the kept features are the last `report.num_features` rows"""
        num = C.c_int64()
        _capi.lib().pp_sift_extract_features(self._h, None, None, None, 0, C.byref(num))
        n = num.value
        raw, ol, ang = np.zeros((max(n, 1), 128), dtype=np.float32), np.zeros((max(n, 1), 2), dtype=np.int32), np.zeros(max(n, 1))
        check(_capi.lib().pp_sift_extract_features(self._h, ptr(raw, C.POINTER(C.c_float)), ptr(ol, _capi.c_ip), dp(ang), n, C.byref(num)))
        return raw[:n], ol[:n], ang[:n]

    @staticmethod
    def _batch_table(images):
        """the images of a batch call as contiguous arrays (kept alive by the caller) and the pp_sift_batch_image table over them"""
        ims = []
        for image in images:
            im = np.asarray(image)
            if im.dtype != np.uint8 or im.ndim != 2:
                raise ValueError("every image is an [H, W] uint8 array")
            ims.append(np.ascontiguousarray(im))
        table = (_capi.SiftBatchImage * max(len(ims), 1))()
        for i, im in enumerate(ims):
            table[i].width, table[i].height, table[i].grey = int(im.shape[1]), int(im.shape[0]), ptr(im, _capi.c_u8p)
        return ims, table

    @staticmethod
    def _batch_guess(n, o):
        """the first capacity of a batch call that was given none"""
        return min(n * min(2 * int(o.max_num_features), 1 << 16), 1 << 22)

    def extract_batch(self, images, options=None, want_descriptors=True, workspace_bytes=0, capacity=None):
        """pp_sift_extract_batch: images, a sequence of [H, W] uint8 arrays of any sizes -> [(keypoints, descriptors or None, report)] per image, each
        what extract() gives for that image alone; last_batch_report is the batch's.  The images go through the octaves together and their descriptors
        through one launch per octave.  workspace_bytes: the target for the pyramids held at once (0: 8 GiB); more images than fit run in consecutive
        groups, with the same result.  capacity None: the call is repeated with the reported need when the first guess was too small.  Afterwards
        stage(), candidates() and features() raise until the next extract(); batch_features(i) reads the batch."""
        ims, table = self._batch_table(images)
        n = len(ims)
        o = options or sift_extract_options()
        guess = self._batch_guess(n, o) if capacity is None else int(capacity)
        for cap in (guess, None):
            brep, reps, offsets = _capi.SiftBatchReport(), (_capi.SiftExtractReport * max(n, 1))(), np.full(n + 1, -1, dtype=np.int64)
            if cap is None:
                cap = int(self.last_batch_report.num_features)
            kp = np.zeros((max(cap, 1), 4), dtype=np.float32)
            desc = np.zeros((max(cap, 1), 128), dtype=np.uint8) if want_descriptors else None
            rc = _capi.lib().pp_sift_extract_batch(self._h, C.byref(o), n, table, int(workspace_bytes), C.byref(brep), reps, cap,
                                                   ptr(kp, C.POINTER(C.c_float)), ptr(desc, _capi.c_u8p), ptr(offsets, C.POINTER(C.c_int64)))
            if rc == 0 or capacity is not None or offsets[n] <= cap:      # (offsets[n] stays -1 where the arguments were refused)
                break
            self.last_batch_report = brep
        check(rc)
        self.last_batch_report = brep
        out = []
        for i in range(n):
            a, b = int(offsets[i]), int(offsets[i + 1])
            out.append((kp[a:b].copy(), None if desc is None else desc[a:b].copy(), reps[i]))
        return out

    def extract_to_matcher(self, images, options=None, workspace_bytes=0, capacity=None):
        """pp_sift_extract_to_matcher: extract_batch for features that go to the matcher -> (keypoints per image ([N_i, 4] float32 each), reports per
        image, the batch report, a SiftMatcher on this extractor's device whose image i holds the N_i descriptors of images[i]).  Keypoints and
        descriptors (SiftMatcher.descriptors(i)) are extract_batch's; only the kept features get an orientation and a descriptor, and no descriptor
        comes to the host.  The four report counts that follow the features cover the kept ones only.  The caller closes the matcher.  Afterwards
        stage(), candidates(), features() and batch_features() raise until the next extract() or extract_batch()."""
        ims, table = self._batch_table(images)
        n = len(ims)
        o = options or sift_extract_options()
        guess = self._batch_guess(n, o) if capacity is None else int(capacity)
        for cap in (guess, None):
            brep, reps, offsets = _capi.SiftBatchReport(), (_capi.SiftExtractReport * max(n, 1))(), np.full(n + 1, -1, dtype=np.int64)
            if cap is None:
                cap = int(self.last_batch_report.num_features)
            kp, handle = np.zeros((max(cap, 1), 4), dtype=np.float32), C.c_void_p()
            rc = _capi.lib().pp_sift_extract_to_matcher(self._h, C.byref(o), n, table, int(workspace_bytes), C.byref(brep), reps, cap,
                                                        ptr(kp, C.POINTER(C.c_float)), ptr(offsets, C.POINTER(C.c_int64)), C.byref(handle))
            if rc == 0 or capacity is not None or offsets[n] <= cap:      # (offsets[n] stays -1 where the arguments were refused)
                break
            self.last_batch_report = brep
        check(rc)
        self.last_batch_report = brep
        matcher = SiftMatcher.from_handle(handle, offsets)
        return [kp[int(offsets[i]):int(offsets[i + 1])].copy() for i in range(n)], [reps[i] for i in range(n)], brep, matcher

    def batch_features(self, image):
        """features() for image `image` of the last extract_batch"""
        num = C.c_int64()
        _capi.lib().pp_sift_extract_batch_features(self._h, int(image), None, None, None, 0, C.byref(num))
        n = num.value
        raw, ol, ang = np.zeros((max(n, 1), 128), dtype=np.float32), np.zeros((max(n, 1), 2), dtype=np.int32), np.zeros(max(n, 1))
        check(_capi.lib().pp_sift_extract_batch_features(self._h, int(image), ptr(raw, C.POINTER(C.c_float)), ptr(ol, _capi.c_ip), dp(ang), n, C.byref(num)))
        return raw[:n], ol[:n], ang[:n]


def line_features_options(**kw):
    return _capi.options(_capi.LineFeaturesOptions, "pp_line_features_options_default", **kw)


class LineFeatureGenerator:
    """pp_line_features_from_keypoints: keypoints of a batch of images, undistorted with their cameras, to one line each (K19).  Owns nothing between
    calls; generate() is the call."""

    def __init__(self, device=0):
        self.device = int(device)

    def generate(self, image_ids, kp_start, keypoints, image_camera, camera_model, intr, has_gravity=None, gravity=None, aligned_line_ratio=0.5,
                 seed=0, want_dirs=True):
        """-> dict(lines [L, 3], aligned [L] uint8, dirs [L, 3] or None, report)"""
        ids = np.ascontiguousarray(image_ids, dtype=np.int32).reshape(-1)
        num_images = int(ids.shape[0])
        start = np.ascontiguousarray(kp_start, dtype=np.int64).reshape(-1)
        if start.shape[0] != num_images + 1:
            raise ValueError("kp_start has num_images + 1 entries")
        kp = np.ascontiguousarray(keypoints, dtype=np.float32).reshape(-1, 2)
        cam = np.ascontiguousarray(image_camera, dtype=np.int32).reshape(-1)
        model = np.ascontiguousarray(camera_model, dtype=np.int32).reshape(-1)
        num_cameras = int(model.shape[0])
        params = np.ascontiguousarray(intr, dtype=np.float64).reshape(num_cameras, _capi.CAM_STRIDE)
        if cam.shape[0] != num_images:
            raise ValueError("one camera index per image")
        hg = None if has_gravity is None else np.ascontiguousarray(np.asarray(has_gravity, dtype=bool), dtype=np.uint8).reshape(-1)
        gv = None if gravity is None else np.ascontiguousarray(gravity, dtype=np.float64).reshape(num_images, 3)
        if hg is not None and hg.shape[0] != num_images:
            raise ValueError("one has_gravity flag per image")
        L = max(int(start[-1]), 0)
        if kp.shape[0] < L:
            raise ValueError("kp_start names %d keypoints, %d given" % (L, kp.shape[0]))
        desc = _capi.LineFeaturesDesc()
        desc.num_images, desc.num_cameras = num_images, num_cameras
        desc.image_ids = ptr(ids, _capi.c_ip) if num_images else None
        desc.kp_start = ptr(start, C.POINTER(C.c_int64))
        desc.keypoints = ptr(kp, C.POINTER(C.c_float)) if kp.size else None
        desc.image_camera = ptr(cam, _capi.c_ip) if num_images else None
        desc.camera_model = ptr(model, _capi.c_ip) if num_cameras else None
        desc.intr = dp(params) if num_cameras else None
        desc.has_gravity = ptr(hg, _capi.c_u8p) if hg is not None and num_images else None
        desc.gravity = dp(gv) if gv is not None and num_images else None
        opt = line_features_options(aligned_line_ratio=float(aligned_line_ratio), seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
        lines = np.zeros((max(L, 1), 3))
        aligned = np.zeros(max(L, 1), dtype=np.uint8)
        dirs = np.zeros((max(L, 1), 3)) if want_dirs else None
        rep = _capi.LineFeaturesReport()
        check(_capi.lib().pp_line_features_from_keypoints(C.byref(desc), C.byref(opt), self.device, dp(lines), ptr(aligned, _capi.c_u8p), dp(dirs),
                                                          C.byref(rep)))
        return dict(lines=lines[:L], aligned=aligned[:L], dirs=None if dirs is None else dirs[:L], report=rep)
