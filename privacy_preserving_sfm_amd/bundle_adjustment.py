"""Host mirror of the reference's bundle-adjustment interface on top of the C ABI.

Same names, argument meaning and error behaviour as reference src/optim/bundle_adjustment.{h,cc}:
`BundleAdjustmentOptions` (:49-100), `BundleAdjustmentConfig` (:103-167), `BundleAdjuster` (:171-203), and the
minimal data model it reads raw doubles from (`Reconstruction`, `Image`, `Camera`, `Point3D`, `FeatureLine`:
base/image.h, base/camera.h, base/point3d.h, feature/types.h:98-138).  `BundleAdjuster.Solve` performs exactly
the SetUp of bundle_adjustment.cc:326-542 (which observations exist, which blocks are constant), flattens it to
the arrays of `pp_ba_problem_desc`, and hands the solve to the device (`pp_ba_solve`).

Above it, the mapper's global refinement: `Reconstruction.Normalize` (base/reconstruction.cc:302-397), `AdjustGlobalBundle`
(sfm/incremental_mapper.cc:893-939 with the option preset of controllers/incremental_mapper.cc:52-70, 221-243) and
`IterativeGlobalRefinement` (controllers/incremental_mapper.cc:102-124); and the local one after every registered image: `FindLocalBundle`
(sfm/incremental_mapper.cc:993-1160), `AdjustLocalBundle` (:781-891) and `IterativeLocalRefinement` (controllers/incremental_mapper.cc:72-100) on
one `pp_tracks_handle` of an `incremental_triangulator.IncrementalTriangulator`.
"""
import numpy as np

from . import _capi
from .device import BAProblem, ba_options

kInvalidPoint3DId = -1


class FeatureLine:
    """feature/types.h:98-138: a 2D line (a,b,c) in normalised coordinates, gravity-alignment flag, 3D point id."""

    def __init__(self, line, is_aligned=False, point3D_id=kInvalidPoint3DId):
        self._line = np.asarray(line, dtype=np.float64).copy()
        self._aligned = bool(is_aligned)
        self.point3D_id = point3D_id

    def Line(self):
        return self._line

    def IsAligned(self):
        return self._aligned

    def HasPoint3D(self):
        return self.point3D_id != kInvalidPoint3DId

    def Point3DId(self):
        return self.point3D_id


class Camera:
    def __init__(self, camera_id, model_id, params, width=None, height=None):
        self.camera_id, self.model_id = camera_id, int(model_id)
        if width is not None:          # (a camera without a size keeps the filters' "no image bounds" default)
            self.width, self.height = int(width), int(height)
        n = _capi.lib().pp_camera_num_params(self.model_id)
        if n < 0:
            raise ValueError("camera model %d does not exist" % model_id)   # CAMERA_MODEL_DOES_NOT_EXIST_EXCEPTION
        self.params = np.asarray(params, dtype=np.float64).copy()
        assert self.params.shape == (n,)

    def ModelId(self):
        return self.model_id

    def NumParams(self):
        return len(self.params)

    def FocalLengthIdxs(self):
        return [0] if self.model_id in (0, 2, 3, 8, 9) else [0, 1]

    def PrincipalPointIdxs(self):
        return [1, 2] if self.model_id in (0, 2, 3, 8, 9) else [2, 3]

    def ExtraParamsIdxs(self):
        first = 3 if self.model_id in (0, 2, 3, 8, 9) else 4
        return list(range(first, len(self.params)))

    def _map(self, entry, points):
        pts = np.ascontiguousarray(points, dtype=np.float64)
        flat = np.ascontiguousarray(pts.reshape(-1, 2))
        out = np.zeros_like(flat)
        _capi.check(entry(self.model_id, _capi.dp(_capi.f64(self.params)), flat.shape[0], _capi.dp(flat), _capi.dp(out)))
        return out.reshape(pts.shape)

    def ImageToWorld(self, image_points):
        """Camera::ImageToWorld (base/camera.cc): pixel (x, y) or [N, 2] -> normalised (u, v), on the host through pp_camera_image_to_world"""
        return self._map(_capi.lib().pp_camera_image_to_world, image_points)

    def WorldToImage(self, world_points):
        """Camera::WorldToImage: normalised (u, v) or [N, 2] -> pixel (x, y), on the host through pp_camera_world_to_image"""
        return self._map(_capi.lib().pp_camera_world_to_image, world_points)

    def HasBogusParams(self, min_focal_length_ratio, max_focal_length_ratio, max_extra_param):
        """Camera::HasBogusParams (base/camera.cc:186-192, base/camera_models.h:473-531): principal point outside the image, a focal length
        outside [min, max] x max(width, height), or an extra parameter beyond max_extra_param in magnitude"""
        if not hasattr(self, "width"):
            raise ValueError("Camera.HasBogusParams needs the camera's width and height")
        cx, cy = (self.params[i] for i in self.PrincipalPointIdxs())
        if cx < 0 or cx > self.width or cy < 0 or cy > self.height:
            return True
        max_size = max(self.width, self.height)
        for i in self.FocalLengthIdxs():
            ratio = self.params[i] / max_size
            if ratio < min_focal_length_ratio or ratio > max_focal_length_ratio:
                return True
        return any(abs(self.params[i]) > max_extra_param for i in self.ExtraParamsIdxs())


class Image:
    def __init__(self, image_id, camera_id, qvec, tvec, lines=(), gravity=None):
        self.image_id, self.camera_id = image_id, camera_id
        self.qvec = np.asarray(qvec, dtype=np.float64).copy()
        self.tvec = np.asarray(tvec, dtype=np.float64).copy()
        self.lines = list(lines)
        self.gravity = None if gravity is None else np.asarray(gravity, dtype=np.float64).copy()      # base/image.h GravityDirection(), camera frame

    def HasGravity(self):
        return getattr(self, "gravity", None) is not None

    def GravityDirection(self):
        return self.gravity

    def CameraId(self):
        return self.camera_id

    def NormalizeQvec(self):
        n = np.linalg.norm(self.qvec)
        self.qvec = np.array([1.0, 0, 0, 0]) if n == 0 else self.qvec / n      # base/pose.cc NormalizeQuaternion

    def Lines(self):
        return self.lines

    def Line(self, idx):
        return self.lines[idx]


class Point3D:
    def __init__(self, xyz, track=()):
        self.xyz = np.asarray(xyz, dtype=np.float64).copy()
        self.track = list(track)          # [(image_id, line_idx)]
        self.error = -1.0                 # Point3D::Error(), set by FilterPoints3DWithLargeReprojectionError


def _quat_to_rot(q):
    """[..., 4] (w,x,y,z) -> [..., 3, 3], the polynomial Eigen::Quaterniond applies to a vector (no normalisation inside)"""
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return np.moveaxis(R, (0, 1), (-2, -1))


def _normalize_transform(coords, extent, p0, p1):
    """base/reconstruction.cc:324-380: (translation, scale) from N x 3 coordinates - cast to float, sorted per axis, the box between the p0 and p1
    index (all of them up to three coordinates), the mean over that index range."""
    c = np.sort(np.asarray(coords, dtype=np.float64).astype(np.float32), axis=0)
    n = c.shape[0]
    i0 = int(p0 * (n - 1)) if n > 3 else 0
    i1 = int(p1 * (n - 1)) if n > 3 else n - 1
    bbox_min, bbox_max = c[i0].astype(np.float64), c[i1].astype(np.float64)
    mean = np.zeros(3)
    for i in range(i0, i1 + 1):          # summed in double, in sorted order, as the reference does
        mean += c[i]
    mean /= i1 - i0 + 1
    old_extent = float(np.linalg.norm(bbox_max - bbox_min))
    scale = 1.0 if old_extent < np.finfo(np.float64).eps else extent / old_extent
    return mean, scale


class Reconstruction:
    def __init__(self):
        self.cameras, self.images, self.points3D = {}, {}, {}

    def Camera(self, cid):
        return self.cameras[cid]

    def Image(self, iid):
        return self.images[iid]

    def Point3D(self, pid):
        return self.points3D[pid]

    # ---- filters run after every bundle adjustment (base/reconstruction.cc:425-460, 594-719) on the device ------------
    def _filter_scene(self):
        """flat problem over ALL registered images and points (every observation of every point)"""
        image_ids = sorted(self.images)
        point_ids = sorted(self.points3D)
        cam_ids = sorted(self.cameras)
        pose_index = {iid: k for k, iid in enumerate(image_ids)}
        point_index = {pid: k for k, pid in enumerate(point_ids)}
        cam_index = {cid: k for k, cid in enumerate(cam_ids)}
        lines, obs_pose, obs_point, aligned, obs_ref = [], [], [], [], []
        for pid in point_ids:                       # observations in track order: the track IS the per-point list
            for (iid, idx) in self.points3D[pid].track:
                fl = self.images[iid].lines[idx]
                lines.append(fl.Line()); obs_pose.append(pose_index[iid]); obs_point.append(point_index[pid]); aligned.append(bool(fl.IsAligned()))
                obs_ref.append((iid, idx))
        intr = np.zeros((len(cam_ids), 12))
        for cid, k in cam_index.items():
            intr[k, : self.cameras[cid].NumParams()] = self.cameras[cid].params
        scene = dict(lines=np.array(lines, dtype=np.float64).reshape(-1, 3), obs_pose=np.array(obs_pose, dtype=np.int32), obs_point=np.array(obs_point, dtype=np.int32),
                     pose_camera=np.array([cam_index[self.images[i].camera_id] for i in image_ids], dtype=np.int32),
                     camera_model=np.array([self.cameras[c].model_id for c in cam_ids], dtype=np.int32),
                     poses=np.array([np.concatenate([self.images[i].qvec, self.images[i].tvec]) for i in image_ids]),
                     points=np.array([self.points3D[p].xyz for p in point_ids]), intr=intr)
        cam_size = np.array([[getattr(self.cameras[c], "width", 1 << 30), getattr(self.cameras[c], "height", 1 << 30)] for c in cam_ids], dtype=np.int32)
        return scene, np.array(aligned, dtype=bool), cam_size, point_ids, obs_ref

    def DeleteObservation(self, image_id, line_idx):
        fl = self.images[image_id].lines[line_idx]
        pid = fl.point3D_id
        self.points3D[pid].track = [t for t in self.points3D[pid].track if t != (image_id, line_idx)]
        fl.point3D_id = kInvalidPoint3DId

    def DeletePoint3D(self, pid):
        for (iid, idx) in self.points3D[pid].track:
            self.images[iid].lines[idx].point3D_id = kInvalidPoint3DId
        del self.points3D[pid]

    def AddObservation(self, point3D_id, track_el):
        """Reconstruction::AddObservation (base/reconstruction.cc:190-204): the line gets the point, the track its element at the end"""
        image_id, line_idx = track_el
        fl = self.images[image_id].lines[line_idx]
        assert not fl.HasPoint3D()
        fl.point3D_id = point3D_id
        self.points3D[point3D_id].track.append((image_id, line_idx))

    def AddPoint3D(self, xyz, track):
        """Reconstruction::AddPoint3D (base/reconstruction.cc:167-188): a new point under the next unused id (++num_added_points3D_; here one past the
        largest id ever seen), every element of its track gets the point.  -> the id"""
        self._num_added_points3D = max(getattr(self, "_num_added_points3D", 0), max(self.points3D, default=-1) + 1)
        new_id = self._num_added_points3D
        self._num_added_points3D += 1
        self.points3D[new_id] = Point3D(xyz, track)
        for (iid, idx) in self.points3D[new_id].track:
            assert not self.images[iid].lines[idx].HasPoint3D()
            self.images[iid].lines[idx].point3D_id = new_id
        return new_id

    def MergePoints3D(self, point3D_id1, point3D_id2):
        """Reconstruction::MergePoints3D (base/reconstruction.cc:206-232): the length-weighted mean position, track 1 followed by track 2, both points
        deleted, the merged one added under the next unused id (++num_added_points3D_; here one past the largest id ever seen)."""
        p1, p2 = self.points3D[point3D_id1], self.points3D[point3D_id2]
        l1, l2 = float(len(p1.track)), float(len(p2.track))
        merged_xyz = (l1 * p1.xyz + l2 * p2.xyz) / (l1 + l2)
        merged_track = list(p1.track) + list(p2.track)
        self._num_added_points3D = max(getattr(self, "_num_added_points3D", 0), max(self.points3D) + 1)
        self.DeletePoint3D(point3D_id1)
        self.DeletePoint3D(point3D_id2)
        new_id = self._num_added_points3D
        self._num_added_points3D += 1
        self.points3D[new_id] = Point3D(merged_xyz, merged_track)
        for (iid, idx) in merged_track:
            self.images[iid].lines[idx].point3D_id = new_id
        return new_id

    def FilterPoints3D(self, max_reproj_error, min_tri_angle, point3D_ids=None, device=0):
        """Reconstruction::FilterPoints3D / FilterAllPoints3D (point3D_ids = None): returns the number of filtered
        observations as the reference counts them; points and observations are deleted, Point3D.error is set."""
        from .device import BAProblem
        if not self.points3D:
            return 0
        scene, aligned, cam_size, point_ids, obs_ref = self._filter_scene()
        if len(obs_ref) == 0:
            return 0
        subset = None if point3D_ids is None else np.array([p in set(point3D_ids) for p in point_ids], dtype=np.uint8)
        pb = BAProblem(scene, device=device)
        try:
            rep, od, pd, pe = pb.filter_points(max_reproj_error, min_tri_angle, cam_size, obs_aligned=aligned, point_subset=subset)
        finally:
            pb.close()
        self._apply_points_filter(scene, point_ids, obs_ref, od, pd, pe)
        return int(rep.num_filtered)

    def _apply_points_filter(self, scene, point_ids, obs_ref, od, pd, pe):
        """deletes what a FilterPoints3D over `_filter_scene()` reported (masks per observation / per point, error per point)"""
        for k, pid in enumerate(point_ids):
            if pd[k]:
                self.DeletePoint3D(pid)
            elif pe[k] >= 0:
                self.points3D[pid].error = float(pe[k])
        for o, (iid, idx) in enumerate(obs_ref):
            pid = point_ids[scene["obs_point"][o]]
            if od[o] and pid in self.points3D:
                self.DeleteObservation(iid, idx)

    def FilterPoints3DInImages(self, max_reproj_error, min_tri_angle, image_ids, device=0):
        """Reconstruction::FilterPoints3DInImages (base/reconstruction.cc:412-426): FilterPoints3D over the points the lines of these images have"""
        point3D_ids = set(line.Point3DId() for image_id in image_ids for line in self.images[image_id].lines if line.HasPoint3D())
        return self.FilterPoints3D(max_reproj_error, min_tri_angle, point3D_ids, device=device)

    def FilterAllPoints3D(self, max_reproj_error, min_tri_angle, device=0):
        return self.FilterPoints3D(max_reproj_error, min_tri_angle, None, device=device)

    def FilterObservationsWithNegativeDepth(self, device=0):
        from .device import BAProblem
        if not self.points3D:
            return 0
        scene, aligned, cam_size, point_ids, obs_ref = self._filter_scene()
        if len(obs_ref) == 0:
            return 0
        pb = BAProblem(scene, device=device)
        try:
            n, neg = pb.filter_negative_depth()
        finally:
            pb.close()
        for o, (iid, idx) in enumerate(obs_ref):
            if neg[o]:
                self.DeleteObservation(iid, idx)
        return n

    def DeRegisterImage(self, image_id):
        """The bookkeeping half of Reconstruction::DeRegisterImage (base/reconstruction.cc:285-300): the image leaves the registered ones (`registered`
        False, `reg_index` dropped).  Its observations are deleted by the events of pp_tracks_filter_images, which the caller applies
        (incremental_triangulator._TracksSession.filter_images)."""
        image = self.images[image_id]
        image.registered = False
        if hasattr(image, "reg_index"):
            del image.reg_index

    def RegImageIds(self):
        """The registered images in the order of their registration.  An image is registered unless it carries `registered = False`
        (incremental_mapper.IncrementalMapper.RegisterNextImage turns it into True and numbers it with `reg_index`); the images that were registered
        from the start come first, in the order of their ids."""
        reg = [i for i in self.images if getattr(self.images[i], "registered", True)]
        return sorted(reg, key=lambda i: (getattr(self.images[i], "reg_index", -1), i))

    def _observations(self):
        return set((iid, idx) for iid, image in self.images.items() for idx, l in enumerate(image.lines) if l.HasPoint3D())

    def ComputeNumObservations(self):
        """base/reconstruction.cc:486-492"""
        return len(self._observations())

    def Normalize(self, extent=10.0, p0=0.1, p1=0.9, use_images=True):
        """Reconstruction::Normalize (base/reconstruction.cc:302-397): a translation, then a scale, of every image and point, so that the robust
        bounding box of the projection centres (or of the points) has diagonal `extent` around their robust mean.  Host, O(C log C + P)."""
        assert extent > 0 and 0 <= p0 <= p1 <= 1
        image_ids = self.RegImageIds()
        if (use_images and len(image_ids) < 2) or (not use_images and len(self.points3D) < 2):
            return
        qvecs = np.array([self.images[i].qvec for i in image_ids]).reshape(-1, 4)
        tvecs = np.array([self.images[i].tvec for i in image_ids]).reshape(-1, 3)
        unit = qvecs / np.linalg.norm(qvecs, axis=1, keepdims=True)          # ProjectionCenterFromPose normalises (base/pose.cc:94-101)
        centres = -np.einsum("cji,cj->ci", _quat_to_rot(unit), tvecs)
        coords = centres if use_images else np.array([self.points3D[p].xyz for p in sorted(self.points3D)])
        translation, scale = _normalize_transform(coords, extent, p0, p1)
        centres = (centres - translation) * scale
        new_tvecs = np.einsum("cij,cj->ci", _quat_to_rot(qvecs), -centres)    # quat * -centre with Qvec as stored (:386-389)
        for k, iid in enumerate(image_ids):
            self.images[iid].tvec = new_tvecs[k].copy()
        for point in self.points3D.values():
            point.xyz = (point.xyz - translation) * scale

    @staticmethod
    def from_scene(scene):
        """Builds the object model from the flat synthetic scene (images 0..C-1, one line per observation)."""
        rec = Reconstruction()
        for k in range(scene["intr"].shape[0]):
            m = int(scene["camera_model"][k])
            rec.cameras[k] = Camera(k, m, scene["intr"][k, : _capi.lib().pp_camera_num_params(m)])
        for c in range(scene["poses"].shape[0]):
            rec.images[c] = Image(c, int(scene["pose_camera"][c]), scene["poses"][c, :4], scene["poses"][c, 4:])
        for p in range(scene["points"].shape[0]):
            rec.points3D[p] = Point3D(scene["points"][p])
        for o in range(len(scene["obs_pose"])):
            c, p = int(scene["obs_pose"][o]), int(scene["obs_point"][o])
            rec.images[c].lines.append(FeatureLine(scene["lines"][o], False, p))
            rec.points3D[p].track.append((c, len(rec.images[c].lines) - 1))
        return rec


class SolverOptions:
    """The ceres::Solver::Options fields the reference sets (bundle_adjustment.h:80-93)."""

    def __init__(self):
        self.function_tolerance = 0.0
        self.gradient_tolerance = 0.0
        self.parameter_tolerance = 0.0
        self.minimizer_progress_to_stdout = False
        self.max_num_iterations = 100
        self.max_linear_solver_iterations = 200
        self.max_num_consecutive_invalid_steps = 10
        self.max_consecutive_nonmonotonic_steps = 10
        self.num_threads = -1
        # Solver::Options::callbacks: the reference pushes ONE ceres::IterationCallback (controllers/bundle_adjustment.cc:87-88)
        self.iteration_callback = None


class BundleAdjustmentOptions:
    TRIVIAL, SOFT_L1, CAUCHY = 0, 1, 2      # enum class LossFunctionType

    def __init__(self):
        self.loss_function_type = self.TRIVIAL
        self.loss_function_scale = 1.0
        self.refine_focal_length = False
        self.refine_principal_point = False
        self.refine_extra_params = False
        self.refine_extrinsics = True
        self.print_summary = True
        self.min_num_residuals_for_multi_threading = 50000
        self.solver_options = SolverOptions()

    def Check(self):
        if not self.loss_function_scale >= 0:       # CHECK_OPTION_GE(loss_function_scale, 0)
            return False
        return True


class BundleAdjustmentConfig:
    """bundle_adjustment.h:103-167: which images / points take part and what is held constant."""

    def __init__(self):
        self._constant_camera_ids, self._image_ids = set(), set()
        self._variable_point3D_ids, self._constant_point3D_ids = set(), set()
        self._constant_poses, self._constant_tvecs = set(), {}

    def NumImages(self):
        return len(self._image_ids)

    def NumPoints(self):
        return len(self._variable_point3D_ids) + len(self._constant_point3D_ids)

    def NumConstantCameras(self):
        return len(self._constant_camera_ids)

    def NumConstantPoses(self):
        return len(self._constant_poses)

    def NumConstantTvecs(self):
        return len(self._constant_tvecs)

    def NumVariablePoints(self):
        return len(self._variable_point3D_ids)

    def NumConstantPoints(self):
        return len(self._constant_point3D_ids)

    def NumResiduals(self, reconstruction):
        # bundle_adjustment.cc:109-140: two residuals per observation of the images and of the added points
        n = 0
        for iid in self._image_ids:
            n += sum(1 for l in reconstruction.Image(iid).Lines() if l.HasPoint3D())
        for pid in self._variable_point3D_ids | self._constant_point3D_ids:
            n += sum(1 for (iid, _) in reconstruction.Point3D(pid).track if iid not in self._image_ids)
        return 2 * n

    def AddImage(self, image_id):
        self._image_ids.add(image_id)

    def HasImage(self, image_id):
        return image_id in self._image_ids

    def RemoveImage(self, image_id):
        self._image_ids.discard(image_id)

    def SetConstantCamera(self, camera_id):
        self._constant_camera_ids.add(camera_id)

    def SetVariableCamera(self, camera_id):
        self._constant_camera_ids.discard(camera_id)

    def IsConstantCamera(self, camera_id):
        return camera_id in self._constant_camera_ids

    def SetConstantPose(self, image_id):
        assert self.HasImage(image_id) and not self.HasConstantTvec(image_id)
        self._constant_poses.add(image_id)

    def SetVariablePose(self, image_id):
        self._constant_poses.discard(image_id)

    def HasConstantPose(self, image_id):
        return image_id in self._constant_poses

    def SetConstantTvec(self, image_id, idxs):
        idxs = list(idxs)
        assert 0 < len(idxs) <= 3 and self.HasImage(image_id) and not self.HasConstantPose(image_id)
        assert len(set(idxs)) == len(idxs), "Tvec indices must not contain duplicates"
        self._constant_tvecs[image_id] = idxs

    def RemoveConstantTvec(self, image_id):
        self._constant_tvecs.pop(image_id, None)

    def HasConstantTvec(self, image_id):
        return image_id in self._constant_tvecs

    def ConstantTvec(self, image_id):
        return self._constant_tvecs[image_id]

    def AddVariablePoint(self, pid):
        assert not self.HasConstantPoint(pid)
        self._variable_point3D_ids.add(pid)

    def AddConstantPoint(self, pid):
        assert not self.HasVariablePoint(pid)
        self._constant_point3D_ids.add(pid)

    def HasPoint(self, pid):
        return self.HasVariablePoint(pid) or self.HasConstantPoint(pid)

    def HasVariablePoint(self, pid):
        return pid in self._variable_point3D_ids

    def HasConstantPoint(self, pid):
        return pid in self._constant_point3D_ids

    def RemoveVariablePoint(self, pid):
        self._variable_point3D_ids.discard(pid)

    def RemoveConstantPoint(self, pid):
        self._constant_point3D_ids.discard(pid)

    def Images(self):
        return self._image_ids

    def VariablePoints(self):
        return self._variable_point3D_ids

    def ConstantPoints(self):
        return self._constant_point3D_ids


class BundleAdjuster:
    """bundle_adjustment.h:171-203.  `Solve(reconstruction)` -> bool, `Summary()` afterwards."""

    def __init__(self, options, config, device=0):
        assert options.Check()
        self.options_, self.config_, self.device_ = options, config, device
        self.summary_ = None
        self._used = False
        # options.solver_options.callbacks of the reference (controllers/bundle_adjustment.cc:87-88): one
        # ceres::IterationCallback, fn(BAIterationSummary) -> SOLVER_CONTINUE / SOLVER_ABORT / SOLVER_TERMINATE_SUCCESSFULLY
        self.iteration_callback_ = getattr(options.solver_options, "iteration_callback", None)

    def Summary(self):
        return self.summary_

    def flatten(self, reconstruction):
        """SetUp (bundle_adjustment.cc:326-542) -> flat scene dict + id maps.  Host-only; no GPU needed."""
        opt, cfg = self.options_, self.config_
        pose_index, point_index, cam_index = {}, {}, {}
        lines, obs_pose, obs_point = [], [], []
        pose_const, point_num_obs, camera_ids = {}, {}, []

        def pose_of(iid, const):
            if iid not in pose_index:
                pose_index[iid] = len(pose_index)
            pose_const[iid] = const
            return pose_index[iid]

        def point_of(pid):
            if pid not in point_index:
                point_index[pid] = len(point_index)
            return point_index[pid]

        def cam_of(cid):
            if cid not in cam_index:
                cam_index[cid] = len(cam_index)
            return cam_index[cid]

        # AddImageToProblem (:348-435)
        for iid in sorted(cfg.Images()):
            image = reconstruction.Image(iid)
            image.NormalizeQvec()
            constant_pose = (not opt.refine_extrinsics) or cfg.HasConstantPose(iid)
            nobs = 0
            for line in image.Lines():
                if not line.HasPoint3D():
                    continue
                l = line.Line()
                if abs(np.hypot(l[0], l[1]) - 1.0) > 1e-6:
                    raise ValueError("CHECK_NEAR(line.head<2>().norm(), 1.0, 1e-6) failed")   # :373
                nobs += 1
                pid = line.Point3DId()
                point_num_obs[pid] = point_num_obs.get(pid, 0) + 1
                lines.append(l); obs_pose.append(pose_of(iid, constant_pose)); obs_point.append(point_of(pid))
            if nobs > 0 and image.CameraId() not in camera_ids:
                camera_ids.append(image.CameraId())
        # AddPointToProblem (:437-488) for variable then constant points
        constant_cameras = set(c for c in cfg._constant_camera_ids)
        for pid in sorted(cfg.VariablePoints()) + sorted(cfg.ConstantPoints()):
            point = reconstruction.Point3D(pid)
            if point_num_obs.get(pid, 0) == len(point.track):
                continue
            for (iid, line_idx) in point.track:
                if cfg.HasImage(iid):
                    continue
                point_num_obs[pid] = point_num_obs.get(pid, 0) + 1
                image = reconstruction.Image(iid)
                if image.CameraId() not in camera_ids:
                    camera_ids.append(image.CameraId())
                    constant_cameras.add(image.CameraId())
                lines.append(image.Line(line_idx).Line()); obs_pose.append(pose_of(iid, True)); obs_point.append(point_of(pid))
        if not lines:
            return None
        # ParameterizeCameras (:490-528)
        constant_camera = not (opt.refine_focal_length or opt.refine_principal_point or opt.refine_extra_params)
        for iid in pose_index:
            cam_of(reconstruction.Image(iid).CameraId())
        camera_const_mask = np.zeros(len(cam_index), dtype=np.uint16)
        for cid, k in cam_index.items():
            cam = reconstruction.Camera(cid)
            if constant_camera or cid in constant_cameras:
                camera_const_mask[k] = 0xFFFF
                continue
            idxs = []
            if not opt.refine_focal_length:
                idxs += cam.FocalLengthIdxs()
            if not opt.refine_principal_point:
                idxs += cam.PrincipalPointIdxs()
            if not opt.refine_extra_params:
                idxs += cam.ExtraParamsIdxs()
            camera_const_mask[k] = sum(1 << i for i in idxs)
        # ParameterizePoints (:530-542)
        point_const = np.zeros(len(point_index), dtype=np.uint8)
        for pid, k in point_index.items():
            if len(reconstruction.Point3D(pid).track) > point_num_obs.get(pid, 0) or cfg.HasConstantPoint(pid):
                point_const[k] = 1
        C, P, K = len(pose_index), len(point_index), len(cam_index)
        poses = np.zeros((C, 7)); pose_camera = np.zeros(C, dtype=np.int32)
        pconst = np.zeros(C, dtype=np.uint8); tmask = np.zeros(C, dtype=np.uint8)
        for iid, k in pose_index.items():
            image = reconstruction.Image(iid)
            poses[k, :4], poses[k, 4:] = image.qvec, image.tvec
            pose_camera[k] = cam_index[image.CameraId()]
            pconst[k] = 1 if pose_const[iid] else 0
            if not pose_const[iid] and cfg.HasConstantTvec(iid):
                tmask[k] = sum(1 << i for i in cfg.ConstantTvec(iid))
        points = np.zeros((P, 3))
        for pid, k in point_index.items():
            points[k] = reconstruction.Point3D(pid).xyz
        intr = np.zeros((K, _capi.CAM_STRIDE)); camera_model = np.zeros(K, dtype=np.int32)
        for cid, k in cam_index.items():
            cam = reconstruction.Camera(cid)
            intr[k, : cam.NumParams()] = cam.params
            camera_model[k] = cam.ModelId()
        scene = dict(lines=np.array(lines), obs_pose=np.array(obs_pose, dtype=np.int32), obs_point=np.array(obs_point, dtype=np.int32),
                     pose_camera=pose_camera, camera_model=camera_model, poses=poses, points=points, intr=intr,
                     pose_const=pconst, tvec_const_mask=tmask, point_const=point_const, camera_const_mask=camera_const_mask,
                     loss_type=int(opt.loss_function_type), loss_scale=float(opt.loss_function_scale))
        return scene, pose_index, point_index, cam_index

    def flatten_on(self, session):
        """`flatten(session.rec)` from an open tracks session (incremental_triangulator._TracksSession) instead of a loop over the model: SetUp on the
        handle (pp_tracks_bundle_setup) gives the observations, the index arrays, the constant flags and the positions; the poses and the intrinsics
        come from the reconstruction (O(poses + cameras)).  The same (scene, pose_index, point_index, cam_index), array for array and in the same
        order, or None.  The handle must hold the reconstruction's current positions (`session.update()` after whatever changed them)."""
        opt, cfg = self.options_, self.config_
        reconstruction = session.rec
        for iid in sorted(cfg.Images()):
            reconstruction.Image(iid).NormalizeQvec()
        rep, out, pose_ids, point_ids, cam_ids = session.bundle_setup(cfg, opt)
        if rep.bad_line >= 0:
            raise ValueError("CHECK_NEAR(line.head<2>().norm(), 1.0, 1e-6) failed")   # :373
        if rep.num_obs == 0:
            return None
        pose_index = {iid: k for k, iid in enumerate(pose_ids)}
        point_index = {pid: k for k, pid in enumerate(point_ids)}
        cam_index = {cid: k for k, cid in enumerate(cam_ids)}
        C, K = len(pose_ids), len(cam_ids)
        poses = np.zeros((C, 7))
        for k, iid in enumerate(pose_ids):
            image = reconstruction.Image(iid)
            poses[k, :4], poses[k, 4:] = image.qvec, image.tvec
        intr = np.zeros((K, _capi.CAM_STRIDE)); camera_model = np.zeros(K, dtype=np.int32)
        for k, cid in enumerate(cam_ids):
            cam = reconstruction.Camera(cid)
            intr[k, : cam.NumParams()] = cam.params
            camera_model[k] = cam.ModelId()
        scene = dict(lines=out["lines"], obs_pose=out["obs_pose"], obs_point=out["obs_point"], pose_camera=out["pose_camera"], camera_model=camera_model,
                     poses=poses, points=out["points"], intr=intr, pose_const=out["pose_const"], tvec_const_mask=out["pose_tvec_mask"],
                     point_const=out["point_const"], camera_const_mask=out["camera_const_mask"],
                     loss_type=int(opt.loss_function_type), loss_scale=float(opt.loss_function_scale))
        return scene, pose_index, point_index, cam_index

    def Solve(self, reconstruction, session=None):
        """`session`: an open tracks session over this reconstruction whose handle is up to date; without one, the live session of an active
        `with triangulator.Session(...)` is used when there is one.  Either way the problem comes from `flatten_on`; else from `flatten`."""
        assert reconstruction is not None
        assert not self._used, "Cannot use the same BundleAdjuster multiple times"
        self._used = True
        if session is None:
            session = _live_session(reconstruction)
        assert session is None or session.rec is reconstruction
        flat = self.flatten(reconstruction) if session is None else self.flatten_on(session)
        if flat is None:            # problem_->NumResiduals() == 0
            return False
        scene, pose_index, point_index, cam_index = flat
        so = self.options_.solver_options
        opts = ba_options(max_num_iterations=so.max_num_iterations, function_tolerance=so.function_tolerance,
                          gradient_tolerance=so.gradient_tolerance, parameter_tolerance=so.parameter_tolerance,
                          max_num_consecutive_invalid_steps=so.max_num_consecutive_invalid_steps,
                          max_linear_solver_iterations=so.max_linear_solver_iterations)
        # bundle_adjustment.cc:273-286: DENSE_SCHUR up to 50 images, SPARSE_SCHUR up to 1000 (both: the device's direct solve, which
        # finds the block sparsity itself), ITERATIVE_SCHUR + SCHUR_JACOBI above - by the number of images IN THE CONFIG
        kMaxNumImagesDirectSparseSolver = 1000
        linear_solver = _capi.LINEAR_SOLVER_DIRECT if self.config_.NumImages() <= kMaxNumImagesDirectSparseSolver else _capi.LINEAR_SOLVER_ITERATIVE_SCHUR
        pb = BAProblem(scene, device=self.device_, linear_solver=linear_solver)
        try:
            try:
                self.summary_ = pb.solve(opts, iteration_callback=self.iteration_callback_)
            except _capi.PPError as e:
                if e.code != _capi.PP_ERR_NUMERIC:
                    raise
                self.summary_ = e.summary       # termination FAILURE, costs and step counts filled (Ceres returns such a Summary too)
            poses, points, intr = pb.get_parameters()
        finally:
            pb.close()
        if self.options_.print_summary and self.summary_ is not None:
            PrintSolverSummary(self.summary_)
        # Solver::Summary::IsSolutionUsable(): after FAILURE / USER_FAILURE Ceres restores the parameter blocks it was given
        # (recollection of ceres/solver.cc, Ceres absent here: unpinned), so nothing is written back
        if self.summary_.termination in (_capi.TERM_FAILURE, _capi.TERM_USER_FAILURE):
            return True
        self.write_back(reconstruction, flat, poses, points, intr)
        return True

    def Covariance(self, reconstruction, image_ids, point3D_ids=()):
        """Covariance blocks at the reconstruction's current parameters (ceres::Covariance with apply_loss_function = true is the model; the reference has
        no counterpart): ({image_id: 6 x 6}, {point3D_id: 3 x 3}) for the listed ids, and {(image_id_i, image_id_j): 6 x 6} for entries of image_ids that
        are pairs.  Tangent order of a pose: 3 rotation, 3 tvec; no sigma^2 factor; constant blocks are zero.  Does not use up the BundleAdjuster.
        Raises PPError (PP_ERR_NUMERIC) when the problem's gauge is free."""
        flat = self.flatten(reconstruction)
        if flat is None:
            return {}, {}
        scene, pose_index, point_index, _ = flat
        keys = [k if isinstance(k, tuple) else (k, k) for k in image_ids]
        pairs = [(pose_index[i], pose_index[j]) for i, j in keys]
        pids = list(point3D_ids)
        kMaxNumImagesDirectSparseSolver = 1000
        if self.config_.NumImages() > kMaxNumImagesDirectSparseSolver:
            raise ValueError("Covariance needs the direct solver's reduced camera system: at most %d images" % kMaxNumImagesDirectSparseSolver)
        pb = BAProblem(scene, device=self.device_, linear_solver=_capi.LINEAR_SOLVER_DIRECT)
        try:
            pc, xc = pb.covariance(pairs if pairs else np.zeros((0, 2), dtype=np.int32), [point_index[p] for p in pids])
        finally:
            pb.close()
        return ({k: pc[q] for q, k in enumerate(image_ids)}, {p: xc[q] for q, p in enumerate(pids)})

    def CovarianceBlocks(self, reconstruction, blocks):
        """The covariance block of every listed pair of parameter blocks (ceres::Covariance::Compute's list of block pairs): blocks = pairs (key_a, key_b),
        a key ("image", image_id) - 6 rows: 3 rotation, 3 tvec -, ("camera", camera_id) - the camera's NumParams() parameters - or ("point", point3D_id).
        Returns {(key_a, key_b): w_a x w_b array}.  Conventions, refusals and errors as Covariance, which it leaves as it is."""
        flat = self.flatten(reconstruction)
        if flat is None:
            return {}
        scene, pose_index, point_index, cam_index = flat
        index = {"image": ("pose", pose_index), "camera": ("intrinsics", cam_index), "point": ("point", point_index)}
        keys = [(tuple(a), tuple(b)) for a, b in blocks]
        for key in keys:
            for what, _ in key:
                if what not in index:
                    raise ValueError("CovarianceBlocks: unknown key %r (image, camera, point)" % (what,))
        request = [tuple((index[what][0], index[what][1][i]) for what, i in key) for key in keys]
        kMaxNumImagesDirectSparseSolver = 1000
        if self.config_.NumImages() > kMaxNumImagesDirectSparseSolver:
            raise ValueError("CovarianceBlocks needs the direct solver's reduced camera system: at most %d images" % kMaxNumImagesDirectSparseSolver)
        pb = BAProblem(scene, device=self.device_, linear_solver=_capi.LINEAR_SOLVER_DIRECT)
        try:
            out = pb.covariance_blocks(request)
        finally:
            pb.close()

        def rows(side):      # a camera side keeps the parameters its model has
            return reconstruction.Camera(side[1]).NumParams() if side[0] == "camera" else None
        return {key: out[q][:rows(key[0]), :rows(key[1])] for q, key in enumerate(keys)}

    @staticmethod
    def write_back(reconstruction, flat, poses, points, intr):
        """the solved parameters of `flatten()`'s problem into the reconstruction: the variable blocks only"""
        scene, pose_index, point_index, cam_index = flat
        # parameter memory is updated in place, as Ceres does through the raw pointers
        for iid, k in pose_index.items():
            if not scene["pose_const"][k]:
                reconstruction.Image(iid).qvec = poses[k, :4].copy()
                reconstruction.Image(iid).tvec = poses[k, 4:].copy()
        for pid, k in point_index.items():
            if not scene["point_const"][k]:
                reconstruction.Point3D(pid).xyz = points[k].copy()
        for cid, k in cam_index.items():     # variable camera blocks (refine_* flags, bundle_adjustment.cc:490-528)
            cam = reconstruction.Camera(cid)
            n = cam.NumParams()
            if (int(scene["camera_const_mask"][k]) & ((1 << n) - 1)) != (1 << n) - 1:
                cam.params = intr[k, :n].copy()


def PrintSolverSummary(s):
    """bundle_adjustment.cc:544-598."""
    term = {0: "CONVERGENCE", 1: "NO_CONVERGENCE", 2: "FAILURE", 3: "USER_SUCCESS", 4: "USER_FAILURE"}[s.termination]
    rows = (("Residuals", s.num_residuals), ("Parameters", s.num_effective_parameters),
            ("Iterations", s.num_successful_steps + s.num_unsuccessful_steps), ("Time", "%g [s]" % s.total_time_s),
            ("Initial cost", "%g [px]" % np.sqrt(s.initial_cost / max(s.num_residuals, 1))),
            ("Final cost", "%g [px]" % np.sqrt(s.final_cost / max(s.num_residuals, 1))), ("Termination", term))
    for k, v in rows:
        print("%16s%s" % (k + " : ", v))


class IncrementalMapperOptions:
    """The fields of the reference's IncrementalMapperOptions (controllers/incremental_mapper.h:81-108) and IncrementalMapper::Options
    (sfm/incremental_mapper.h:89-98) that the global refinement reads, with their defaults."""

    def __init__(self):
        self.ba_refine_focal_length = False
        self.ba_refine_principal_point = False
        self.ba_refine_extra_params = False
        self.ba_min_num_residuals_for_multi_threading = 50000
        self.ba_global_max_num_iterations = 50
        self.ba_global_max_refinements = 5
        self.ba_global_max_refinement_change = 0.0005
        self.filter_max_reproj_error = 4.0
        self.filter_min_tri_angle = 1.5
        self.print_summary = True
        # the local refinement (controllers/incremental_mapper.h, sfm/incremental_mapper.h:77-80, 98)
        self.local_ba_num_images = 6
        self.local_ba_min_tri_angle = 6.0
        self.fix_existing_images = False
        self.ba_local_max_num_iterations = 25
        self.ba_local_max_refinements = 2
        self.ba_local_max_refinement_change = 0.001
        # choosing and registering the next image (sfm/incremental_mapper.h:62-95, 110)
        self.abs_pose_max_error = 12.0
        self.abs_pose_min_num_inliers = 30
        self.abs_pose_min_inlier_ratio = 0.25
        self.abs_pose_refine_focal_length = False
        self.abs_pose_refine_extra_params = False
        self.min_focal_length_ratio = 0.1
        self.max_focal_length_ratio = 10.0
        self.max_extra_param = 1.0
        self.max_reg_trials = 3
        self.image_selection_method = 1      # 0 MAX_VISIBLE_POINTS_NUM, 1 MAX_VISIBLE_POINTS_RATIO
        # the four initial images (sfm/incremental_mapper.h:52-59; IncrementalMapperOptions::Mapper() passes them on unchanged)
        self.init_min_num_inliers = 20
        self.init_max_error = 5.0            # pixels
        self.init_min_tri_angle = 2.0        # degrees

    def LocalBundleAdjustment(self):
        """controllers/incremental_mapper.cc:196-219"""
        options = BundleAdjustmentOptions()
        options.solver_options.function_tolerance = 0.0
        options.solver_options.gradient_tolerance = 10.0
        options.solver_options.parameter_tolerance = 0.0
        options.solver_options.max_num_iterations = self.ba_local_max_num_iterations
        options.solver_options.max_linear_solver_iterations = 100
        options.solver_options.minimizer_progress_to_stdout = False
        options.print_summary = self.print_summary
        options.refine_focal_length = self.ba_refine_focal_length
        options.refine_principal_point = self.ba_refine_principal_point
        options.refine_extra_params = self.ba_refine_extra_params
        options.min_num_residuals_for_multi_threading = self.ba_min_num_residuals_for_multi_threading
        options.loss_function_scale = 1.0
        options.loss_function_type = BundleAdjustmentOptions.SOFT_L1
        return options

    def GlobalBundleAdjustment(self):
        """controllers/incremental_mapper.cc:221-243"""
        options = BundleAdjustmentOptions()
        options.solver_options.function_tolerance = 0.0
        options.solver_options.gradient_tolerance = 1.0
        options.solver_options.parameter_tolerance = 0.0
        options.solver_options.max_num_iterations = self.ba_global_max_num_iterations
        options.solver_options.max_linear_solver_iterations = 100
        options.solver_options.minimizer_progress_to_stdout = True
        options.print_summary = self.print_summary
        options.refine_focal_length = self.ba_refine_focal_length
        options.refine_principal_point = self.ba_refine_principal_point
        options.refine_extra_params = self.ba_refine_extra_params
        options.min_num_residuals_for_multi_threading = self.ba_min_num_residuals_for_multi_threading
        options.loss_function_type = BundleAdjustmentOptions.TRIVIAL
        return options


def GlobalBundleAdjustmentOptions(num_reg_images, mapper_options=None):
    """The options the controller hands a global bundle adjustment (controllers/incremental_mapper.cc:52-70): the global preset, with
    stricter convergence criteria while fewer than 10 images are registered."""
    options = (mapper_options or IncrementalMapperOptions()).GlobalBundleAdjustment()
    kMinNumRegImagesForFastBA = 10
    if num_reg_images < kMinNumRegImagesForFastBA:
        options.solver_options.function_tolerance /= 10
        options.solver_options.gradient_tolerance /= 10
        options.solver_options.parameter_tolerance /= 10
        options.solver_options.max_num_iterations *= 2
        options.solver_options.max_linear_solver_iterations = 200
    return options


def GlobalBundleAdjustmentConfig(reconstruction):
    """sfm/incremental_mapper.cc:906-926: every registered image, the first one constant, tvec[0] of the second one constant (the 7 gauge DOFs)"""
    reg_image_ids = reconstruction.RegImageIds()
    assert len(reg_image_ids) >= 2, "At least two images must be registered for global bundle-adjustment"
    config = BundleAdjustmentConfig()
    for image_id in reg_image_ids:
        config.AddImage(image_id)
    config.SetConstantPose(reg_image_ids[0])
    config.SetConstantTvec(reg_image_ids[1], [0])
    return config


def _live_session(reconstruction, triangulator=None, options=None):
    """the live session of an active `with triangulator.Session(...)` over this reconstruction (brought up to date with the reconstruction's values), or
    None.  The session registers itself on the reconstruction (`_session_triangulator`), so a call that was not handed the triangulator finds it too and
    cannot delete observations behind the handle's back."""
    triangulator = getattr(reconstruction, "_session_triangulator", None) or triangulator
    if triangulator is None or triangulator._live is None:
        return None
    assert triangulator.reconstruction_ is reconstruction
    return triangulator._open(options or triangulator._live.options)


def AdjustGlobalBundle(reconstruction, ba_options, device=0, summary_out=None, triangulator=None):
    """IncrementalMapper::AdjustGlobalBundle (sfm/incremental_mapper.cc:893-939): negative-depth filter, all images with the gauge fixed, solve,
    Normalize.  Returns the solve's success; `summary_out` (a list) receives the solver summary.  `fix_existing_images` is not mirrored.
    Inside a `with triangulator.Session(...)` the filter runs on the session's handle (pp_tracks_filter_negative_depth, with DeleteObservation's
    "a track of three takes its point" rule, which `Reconstruction.DeleteObservation` and so the path outside a session do not have) and the handle
    receives what the solve and Normalize changed; an active session over this reconstruction is found with or without `triangulator`."""
    live = _live_session(reconstruction, triangulator)
    if live is not None:
        live.filter_negative_depth()
    else:
        reconstruction.FilterObservationsWithNegativeDepth(device=device)
    bundle_adjuster = BundleAdjuster(ba_options, GlobalBundleAdjustmentConfig(reconstruction), device=device)
    ok = bundle_adjuster.Solve(reconstruction, session=live)      # (inside a session: set up on its handle, which the filter above left current)
    if summary_out is not None:
        summary_out.append(bundle_adjuster.Summary())
    if ok:
        reconstruction.Normalize()
    if live is not None:
        live.update()
    return bool(ok)


class GlobalRefinementReport:
    """What IterativeGlobalRefinement did: one entry per round in `summaries` (the solver summary, None where there was nothing to solve),
    `num_filtered` (FilterAllPoints3D's count), `changed` (the changed observations over the observations before the round), and what the round's filter
    deleted: `obs_deleted` (sorted (image_id, line_idx) pairs, those of deleted points included) and `point_deleted` (sorted point ids).
    With a triangulator also, per round, `num_completed` / `num_merged` (CompleteAllTracks' / MergeAllTracks' counts, part of `changed`),
    `completed` [(point id, (image_id, line_idx))] and `merged` [(id a, id b, new id)] in the order they happened, and `initial` = the same four for the
    CompleteAndMergeTracks before the first round."""

    def __init__(self):
        self.num_rounds = 0
        self.summaries, self.num_filtered, self.changed = [], [], []
        self.obs_deleted, self.point_deleted = [], []
        self.num_completed, self.num_merged, self.completed, self.merged = [], [], [], []
        self.initial = None
        self.num_filtered_images = 0      # the closing FilterImages' count (with a mapper)


def IterativeGlobalRefinement(reconstruction, mapper_options=None, device=0, triangulator=None, mapper=None):
    """IterativeGlobalRefinement (controllers/incremental_mapper.cc:102-124): up to `ba_global_max_refinements` rounds of AdjustGlobalBundle,
    CompleteAndMergeTracks and FilterAllPoints3D, until a round changes less than `ba_global_max_refinement_change` of the observations.
    `triangulator` (an incremental_triangulator.IncrementalTriangulator over this reconstruction; its options are `mapper_options.triangulation`
    when that exists, the reference's defaults otherwise) does CompleteAndMergeTracks before the loop and in every round between the bundle adjustment and
    the filter.  Without one that step is left out and `changed` counts filtered observations only, as before.  `mapper` (an
    incremental_mapper.IncrementalMapper over this reconstruction): the closing FilterImages (:122) is its `FilterImages(mapper_options)`; its count goes to
    `report.num_filtered_images`.  Inside a `with triangulator.Session(...)` the negative-depth filter and FilterAllPoints3D run on the session's handle
    (pp_tracks_filter_*) instead of flattening the reconstruction into a throw-away problem each."""
    options = mapper_options or IncrementalMapperOptions()
    report = GlobalRefinementReport()
    tri_options = None
    if triangulator is not None:
        tri_options = getattr(options, "triangulation", None) or triangulator.Options()
        report.initial = triangulator.CompleteAndMergeAllTracks(tri_options)
    for _ in range(options.ba_global_max_refinements):
        num_observations = reconstruction.ComputeNumObservations()
        summaries = []
        AdjustGlobalBundle(reconstruction, GlobalBundleAdjustmentOptions(len(reconstruction.RegImageIds()), options), device=device, summary_out=summaries,
                           triangulator=triangulator)
        num_changed = 0
        if triangulator is not None:
            nc, nm, completed, merged = triangulator.CompleteAndMergeAllTracks(tri_options)
            report.num_completed.append(nc); report.num_merged.append(nm); report.completed.append(completed); report.merged.append(merged)
            num_changed = nc + nm
        obs_before, points_before = reconstruction._observations(), set(reconstruction.points3D)
        live = _live_session(reconstruction, triangulator, tri_options)
        if live is not None:
            num_filtered = live.filter_points(options.filter_max_reproj_error, options.filter_min_tri_angle)
        else:
            num_filtered = reconstruction.FilterAllPoints3D(options.filter_max_reproj_error, options.filter_min_tri_angle, device=device)
        changed = float(num_changed + num_filtered) / num_observations if num_observations else 0.0
        report.num_rounds += 1
        report.summaries.append(summaries[0] if summaries else None)
        report.num_filtered.append(int(num_filtered))
        report.changed.append(changed)
        report.obs_deleted.append(sorted(obs_before - reconstruction._observations()))
        report.point_deleted.append(sorted(points_before - set(reconstruction.points3D)))
        if changed < options.ba_global_max_refinement_change:
            break
    if mapper is not None:
        report.num_filtered_images = mapper.FilterImages(options)
    return report


# ---- the local refinement after every registered image (controllers/incremental_mapper.cc:72-100, sfm/incremental_mapper.cc:781-891, 993-1160) ----

def _local_bundle_options(options):
    from .device import local_bundle_options
    return local_bundle_options(local_ba_num_images=int(options.local_ba_num_images), local_ba_min_tri_angle=float(options.local_ba_min_tri_angle))


def FindLocalBundle(reconstruction, triangulator, options, image_id):
    """IncrementalMapper::FindLocalBundle (sfm/incremental_mapper.cc:993-1160) on the device (pp_tracks_find_local_bundle) -> the image ids in the
    reference's order.  Equal overlap counts are ordered by ascending image id.  `options`: local_ba_num_images, local_ba_min_tri_angle."""
    assert triangulator.reconstruction_ is reconstruction
    ses = triangulator._open(triangulator.Options())
    try:
        return ses.find_local_bundle(image_id, _local_bundle_options(options))[1]
    finally:
        ses.close()


class LocalBundleAdjustmentReport:
    """IncrementalMapper::LocalBundleAdjustmentReport (sfm/incremental_mapper.h:101-106), plus the bundle, the solver summary (None where nothing was
    solved) and what the two filters deleted: `obs_deleted` (sorted (image_id, line_idx), those of deleted points included), `point_deleted`."""

    def __init__(self):
        self.num_merged_observations = self.num_completed_observations = self.num_filtered_observations = self.num_adjusted_observations = 0
        self.local_bundle, self.summary = [], None
        self.variable_point3D_ids = []
        self.obs_deleted, self.point_deleted = [], []


def LocalBundleAdjustmentConfig(reconstruction, options, image_id, local_bundle, point3D_ids, existing_image_ids=(), num_reg_images_per_camera=None):
    """The BundleAdjustmentConfig of AdjustLocalBundle (sfm/incremental_mapper.cc:796-854) -> (config, variable point ids)"""
    existing = set(existing_image_ids)
    config = BundleAdjustmentConfig()
    config.AddImage(image_id)
    for local_image_id in local_bundle:
        config.AddImage(local_image_id)
    if options.fix_existing_images:
        for local_image_id in local_bundle:
            if local_image_id in existing:
                config.SetConstantPose(local_image_id)
    # the cameras stay constant where not all of their registered images are in the bundle
    if num_reg_images_per_camera is None:
        num_reg_images_per_camera = {}
        for iid in reconstruction.RegImageIds():
            if getattr(reconstruction.images[iid], "registered", True):
                cid = reconstruction.images[iid].CameraId()
                num_reg_images_per_camera[cid] = num_reg_images_per_camera.get(cid, 0) + 1
    num_images_per_camera = {}
    for iid in config.Images():
        cid = reconstruction.Image(iid).CameraId()
        num_images_per_camera[cid] = num_images_per_camera.get(cid, 0) + 1
    for cid, n in num_images_per_camera.items():
        if n < num_reg_images_per_camera[cid]:
            config.SetConstantCamera(cid)
    # the 7 gauge degrees of freedom
    if len(local_bundle) == 1:
        config.SetConstantPose(local_bundle[0])
        config.SetConstantTvec(image_id, [0])
    elif len(local_bundle) > 1:
        image_id1, image_id2 = local_bundle[-1], local_bundle[-2]
        config.SetConstantPose(image_id1)
        if not options.fix_existing_images or image_id2 not in existing:
            config.SetConstantTvec(image_id2, [0])
    # new and short-track points are refined, long-track ones that have been through a filter are not
    kMaxTrackLength = 15
    variable = set()
    for pid in point3D_ids:
        point3D = reconstruction.Point3D(pid)
        if not (point3D.error != -1.0) or len(point3D.track) <= kMaxTrackLength:      # !HasError() || Length() <= 15
            config.AddVariablePoint(pid)
            variable.add(pid)
    return config, variable


def AdjustLocalBundle(reconstruction, triangulator, options, ba_options, tri_options, image_id, point3D_ids, existing_image_ids=(),
                      num_reg_images_per_camera=None, device=0):
    """IncrementalMapper::AdjustLocalBundle (sfm/incremental_mapper.cc:781-891) -> LocalBundleAdjustmentReport.  ONE tracks handle serves
    FindLocalBundle, then takes what the bundle adjustment changed (pp_tracks_update), then MergeTracks, CompleteTracks and CompleteImage; the two
    filters run on the reconstruction afterwards - or, inside a `with triangulator.Session(...)`, on that same handle (pp_tracks_filter_points), which
    stays valid for the next step.  `num_reg_images_per_camera` None: counted from the reconstruction's registered images."""
    assert triangulator.reconstruction_ is reconstruction
    report = LocalBundleAdjustmentReport()
    point3D_ids = set(point3D_ids)
    ses = triangulator._open(tri_options)
    try:
        triangulator.last_reports = []
        report.local_bundle = local_bundle = ses.find_local_bundle(image_id, _local_bundle_options(options))[1]
        if len(local_bundle) > 0:
            config, variable = LocalBundleAdjustmentConfig(reconstruction, options, image_id, local_bundle, point3D_ids, existing_image_ids,
                                                           num_reg_images_per_camera)
            report.variable_point3D_ids = sorted(variable)
            bundle_adjuster = BundleAdjuster(ba_options, config, device=device)
            bundle_adjuster.Solve(reconstruction, session=ses)      # (the problem is set up on the handle FindLocalBundle just ran on)
            report.summary = bundle_adjuster.Summary()
            report.num_adjusted_observations = (report.summary.num_residuals if report.summary is not None else 0) // 2
            ses.update()
            report.num_merged_observations = ses.merge(variable)[0]
            report.num_completed_observations = ses.complete(variable)[0]
            report.num_completed_observations += ses.complete_image(image_id)
    finally:
        ses.close()
    obs_before, points_before = reconstruction._observations(), set(reconstruction.points3D)
    filter_image_ids = set([image_id]) | set(local_bundle)
    if ses.live:
        report.num_filtered_observations = ses.filter_points(options.filter_max_reproj_error, options.filter_min_tri_angle, image_ids=filter_image_ids)
        report.num_filtered_observations += ses.filter_points(options.filter_max_reproj_error, options.filter_min_tri_angle, point3D_ids=point3D_ids)
        report.obs_deleted = sorted(obs_before - reconstruction._observations())
        report.point_deleted = sorted(points_before - set(reconstruction.points3D))
        return report
    report.num_filtered_observations = reconstruction.FilterPoints3DInImages(options.filter_max_reproj_error, options.filter_min_tri_angle,
                                                                            filter_image_ids, device=device)
    report.num_filtered_observations += reconstruction.FilterPoints3D(options.filter_max_reproj_error, options.filter_min_tri_angle,
                                                                     point3D_ids, device=device)      # (ids the first filter deleted are skipped)
    report.obs_deleted = sorted(obs_before - reconstruction._observations())
    report.point_deleted = sorted(points_before - set(reconstruction.points3D))
    return report


def IterativeLocalRefinement(reconstruction, triangulator, image_id, mapper_options=None, device=0):
    """IterativeLocalRefinement (controllers/incremental_mapper.cc:72-100): up to `ba_local_max_refinements` rounds of AdjustLocalBundle on the
    triangulator's modified points, the robust loss in the first round only, until a round changes less than `ba_local_max_refinement_change` of the
    adjusted observations; ClearModifiedPoints3D at the end.  -> one LocalBundleAdjustmentReport per round (each with `changed`).  The triangulator's
    options are `mapper_options.triangulation` when that exists, the reference's defaults otherwise."""
    options = mapper_options or IncrementalMapperOptions()
    tri_options = getattr(options, "triangulation", None) or triangulator.Options()
    ba_options = options.LocalBundleAdjustment()
    reports = []
    for _ in range(options.ba_local_max_refinements):
        report = AdjustLocalBundle(reconstruction, triangulator, options, ba_options, tri_options, image_id, triangulator.GetModifiedPoints3D(), device=device)
        n = report.num_merged_observations + report.num_completed_observations + report.num_filtered_observations
        # (the reference divides by zero adjusted observations without a check: inf or NaN, neither is < the bound)
        report.changed = n / float(report.num_adjusted_observations) if report.num_adjusted_observations else (float("inf") if n else float("nan"))
        reports.append(report)
        if report.changed < options.ba_local_max_refinement_change:
            break
        ba_options.loss_function_type = BundleAdjustmentOptions.TRIVIAL
    triangulator.ClearModifiedPoints3D()
    return reports
