"""Host mirror of the steps of the reference's incremental mapper that pick and register images (sfm/incremental_mapper.{h,cc}:
`RegisterInitialLineImages` :192-568, `FindNextImages` :139-190, `RegisterNextImage` :570-760) on top of pp_tracks_find_initial_sets /
pp_tracks_find_next_images / pp_tracks_estimate_image_pose / pp_tracks_register_image (include/ppsfm_hip.h), with the state the reference keeps between
them: `num_reg_trials_`, `filtered_images_`, `num_reg_images_per_camera_`.

`RegisterInitialLineImages` takes a reconstruction from ZERO registered images to four: the image sets worth trying come from the device
(pp_tracks_find_initial_sets), each is handed to `initializer.initialize_reconstruction` (LO-MSAC on the device), the best one is committed on the same
handle and triangulated.  The images that own a gravity-aligned line need `Image.gravity`.  Pinned where the reference is unspecified: sets of equal
aligned count in ascending image set, the four images registered in ascending id, the check images drawn from `random_seed` (the reference seeds from the
wall clock).  Its console histograms (:365-383) are not mirrored.

An unregistered image is an `Image` of `Reconstruction.images` with `registered = False` (an image without the attribute is registered).
With `IncrementalTriangulator.TriangulateImage`, `bundle_adjustment.IterativeLocalRefinement` and `IterativeGlobalRefinement` this is the
reference's per-image sequence (controllers/incremental_mapper.cc:420-520).  Images of equal rank are tried in ascending id (the reference leaves it
to a hash table).  `FilterPoints` (:965-970) and `FilterImages` (:941-963, with `DeRegisterImageEvent` :1177-1192) run on the tracks handle
(pp_tracks_filter_points / pp_tracks_filter_images) and fill `filtered_images_`.  Inside `with triangulator.Session(options):` every step here and in
bundle_adjustment's refinement loops shares ONE handle, from the first image to the last.  The focal-length estimation (never enabled on the reference's
line path) is not mirrored."""
import copy
import ctypes as C

import numpy as np

from . import _capi
from .bundle_adjustment import IncrementalMapperOptions
from .device import init_sets_options, next_image_options, ransac_options
from .estimators import AbsolutePoseRefinementOptions, RefineAbsolutePoseFromLines, RotationMatrixToQuaternion
from .initializer import InitOptions, initialize_reconstruction

kMaxNumCheckImages = 10      # sfm/incremental_mapper.cc:303


def ImageToWorldThreshold(camera, threshold_px):
    """Camera::ImageToWorldThreshold (base/camera_models.h:533-543)"""
    out = C.c_double()
    _capi.check(_capi.lib().pp_camera_image_to_world_threshold(camera.model_id, _capi.dp(_capi.f64(camera.params)), float(threshold_px),
                                                               C.cast(C.byref(out), _capi.c_dp)))
    return out.value


class IncrementalMapper:
    def __init__(self, correspondence_graph, reconstruction, triangulator, database_cameras=None, device=0):
        """database_cameras: {camera id: params} as the database holds them (the camera-reset branch of :686-694 restores them); default: the
        parameters the cameras have now."""
        assert triangulator.reconstruction_ is reconstruction and triangulator.correspondence_graph_ is correspondence_graph
        self.correspondence_graph_, self.reconstruction_, self.triangulator_, self.device_ = correspondence_graph, reconstruction, triangulator, device
        self.database_cameras_ = {cid: np.array(cam.params, dtype=np.float64) for cid, cam in reconstruction.cameras.items()}
        if database_cameras:
            self.database_cameras_.update({cid: np.array(p, dtype=np.float64) for cid, p in database_cameras.items()})
        self.num_reg_trials_ = {}
        self.filtered_images_ = set()
        self.num_reg_images_per_camera_ = {}
        reg = reconstruction.RegImageIds()
        for image_id in reg:
            cid = reconstruction.images[image_id].CameraId()
            self.num_reg_images_per_camera_[cid] = self.num_reg_images_per_camera_.get(cid, 0) + 1
        self._next_reg_index = max([getattr(reconstruction.images[i], "reg_index", -1) for i in reg], default=-1) + 1
        self.ransac_seed = 0              # util/random.h:46 kDefaultPRNGSeed
        self.last_report = None           # the pp_image_pose_report of the last RegisterNextImage
        self.last_refinement = None       # its refinement's solver summary
        self.last_init = None             # what the last RegisterInitialLineImages saw: dict(report, check_image_ids, sets, chosen)

    def _tri_options(self, options):
        o = copy.copy(getattr(options, "triangulation", None) or self.triangulator_.Options())
        o.min_focal_length_ratio, o.max_focal_length_ratio, o.max_extra_param = options.min_focal_length_ratio, options.max_focal_length_ratio, options.max_extra_param
        return o

    @staticmethod
    def _device_options(options):
        assert options.abs_pose_max_error > 0 and options.abs_pose_min_num_inliers > 0 and 0 <= options.abs_pose_min_inlier_ratio <= 1      # Options::Check
        return next_image_options(abs_pose_min_num_inliers=int(options.abs_pose_min_num_inliers), max_reg_trials=int(options.max_reg_trials),
                                  image_selection_method=int(options.image_selection_method))

    def FindNextImages(self, options=None):
        """-> the ids of the unregistered images worth trying, best first; the images that were tried or filtered before come after the others"""
        options = options or IncrementalMapperOptions()
        ses = self.triangulator_._open(self._tri_options(options))
        try:
            return ses.find_next_images(self._device_options(options), self.num_reg_trials_, self.filtered_images_)[1]
        finally:
            ses.close()

    def FilterPoints(self, options=None):
        """IncrementalMapper::FilterPoints (:965-970): FilterAllPoints3D -> num_filtered"""
        options = options or IncrementalMapperOptions()
        ses = self.triangulator_._open(self._tri_options(options))
        try:
            return ses.filter_points(options.filter_max_reproj_error, options.filter_min_tri_angle)
        finally:
            ses.close()

    def FilterImages(self, options=None):
        """IncrementalMapper::FilterImages (:941-963): nothing while fewer than 20 images are registered; then the registered images without a point or with
        bogus camera parameters are de-registered, counted out of `num_reg_images_per_camera_` (DeRegisterImageEvent) and remembered in
        `filtered_images_` -> their number"""
        options = options or IncrementalMapperOptions()
        rec = self.reconstruction_
        kMinNumImages = 20
        if len(rec.RegImageIds()) < kMinNumImages:
            return 0
        ses = self.triangulator_._open(self._tri_options(options))
        try:
            image_ids = ses.filter_images()
        finally:
            ses.close()
        for image_id in image_ids:
            cid = rec.images[image_id].CameraId()
            assert self.num_reg_images_per_camera_.get(cid, 0) > 0
            self.num_reg_images_per_camera_[cid] -= 1
            self.filtered_images_.add(image_id)
        return len(image_ids)

    def AlignedImageIds(self):
        """the images that own at least one gravity-aligned line, ascending: the reference's aligned_db_cache (controllers/incremental_mapper.cc:400-418)"""
        rec = self.reconstruction_
        return [i for i in sorted(rec.images) if any(l.IsAligned() for l in rec.images[i].lines)]

    @staticmethod
    def ChooseCheckImages(image_ids, random_seed=0):
        """:295-309 - up to ten distinct images of the sorted ids.  With at most ten the reference's draw-until-ten-distinct loop yields all of them;
        beyond that it draws from a generator seeded with the wall clock: PINNED here to numpy.random.RandomState(random_seed), returned ascending."""
        image_ids = sorted(image_ids)
        if len(image_ids) <= kMaxNumCheckImages:
            return image_ids
        rng = np.random.RandomState(random_seed)
        return sorted(int(i) for i in rng.choice(np.array(image_ids), kMaxNumCheckImages, replace=False))

    def RegisterInitialLineImages(self, options=None, check_image_ids=None, random_seed=0):
        """IncrementalMapper::RegisterInitialLineImages (:192-568) -> True when four images were registered and triangulated.  False (no qualified image
        set, no set gave poses, or fewer than init_min_num_inliers inliers) leaves the reconstruction as it was.  `self.last_init` keeps the device report,
        the check images, per tried set its images, counts, success and inlier ratio, and the chosen set."""
        options = options or IncrementalMapperOptions()
        rec = self.reconstruction_
        assert len(rec.RegImageIds()) == 0, "CHECK_EQ(reconstruction_->NumRegImages(), 0)"
        assert options.init_min_num_inliers > 0 and options.init_max_error > 0 and options.init_min_tri_angle >= 0      # Options::Check (:78-80)
        subset = self.AlignedImageIds()
        missing = [i for i in subset if not rec.images[i].HasGravity()]
        if missing:
            raise ValueError("RegisterInitialLineImages needs the gravity direction of every image with an aligned line; missing for image ids %s" % missing)
        check_ids = self.ChooseCheckImages(subset, random_seed) if check_image_ids is None else list(check_image_ids)
        self.last_init = dict(report=None, check_image_ids=list(check_ids), sets=[], chosen=None)
        if not check_ids:
            return False
        tri_options = self.triangulator_.Options()      # (:555: DEFAULT triangulator options, whatever the caller's are - the reference's quirk)
        live = self.triangulator_._live      # (the camera thresholds a handle bakes in: the active session's, else the caller's; the defaults are equal)
        baked = live.baked_options if live is not None else options
        tri_options.min_focal_length_ratio, tri_options.max_focal_length_ratio, tri_options.max_extra_param = \
            baked.min_focal_length_ratio, baked.max_focal_length_ratio, baked.max_extra_param
        ses = self.triangulator_._open(tri_options)
        try:
            rep, sets = ses.find_initial_sets(init_sets_options(), check_ids, subset)
            self.last_init["report"] = rep
            best, best_inlier_ratio, best_inliers = None, 0.0, 0
            for s in sets:      # (:436-531)
                ids = s["image_ids"]
                tracks = s["aligned"] + s["random"]      # (:459-481: the aligned tracks first)
                lines = [np.array([rec.images[i].lines[idx].Line() for (i, idx) in (t[v] for t in tracks)]).reshape(-1, 3) for v in range(4)]
                aligned = [np.arange(len(tracks)) < len(s["aligned"])] * 4
                gravity = [rec.images[i].GravityDirection() for i in ids]
                init_options = InitOptions()
                init_options.min_num_inliers, init_options.min_tri_angle = options.init_min_num_inliers, options.init_min_tri_angle
                init_options.max_error = min(ImageToWorldThreshold(rec.Camera(rec.images[i].CameraId()), options.init_max_error) for i in ids)      # (:488-497)
                ok, poses, inlier_ratio = initialize_reconstruction(lines, aligned, gravity, init_options, device=self.device_, random_seed=random_seed)
                ok = bool(ok and poses is not None and len(poses) > 0)
                self.last_init["sets"].append(dict(image_ids=list(ids), num_aligned=s["num_aligned"], num_random=s["num_random"], success=ok,
                                                   inlier_ratio=float(inlier_ratio)))
                if ok and inlier_ratio > best_inlier_ratio:      # (:506, strictly greater)
                    best, best_inlier_ratio = (ids, np.array(poses)), inlier_ratio
                    best_inliers = int(inlier_ratio * len(lines[0]))
            if best is None or best_inliers < options.init_min_num_inliers:      # (:533-541)
                return False
            self.last_init["chosen"] = list(best[0])
            for image_id, pose in sorted(zip(*best), key=lambda x: x[0]):      # (:543-552; PINNED: ascending image id, the reference walks an unordered_map)
                image = rec.images[image_id]
                ses.register_image(image_id, RotationMatrixToQuaternion(pose[:, :3]), pose[:, 3], np.zeros((0, 2), dtype=np.int32), None)
                image.reg_index = self._next_reg_index
                self._next_reg_index += 1
                self.num_reg_images_per_camera_[image.CameraId()] = self.num_reg_images_per_camera_.get(image.CameraId(), 0) + 1      # RegisterImageEvent
            for image_id in rec.RegImageIds():      # (:557-559)
                ses.triangulate_image(image_id)
            if rec.points3D:      # (:562-563; CompleteAllTracks / MergeAllTracks of an empty model do nothing)
                ses.complete(None)
                ses.merge(None)
        finally:
            ses.close()
        return True

    def RegisterNextImage(self, options, image_id):
        """-> True when the image was registered: its pose estimated (P6L RANSAC on the device over the 2D-3D correspondences found on the device),
        refined (RefineAbsolutePoseFromLines) and committed with the observations of its inliers.  False leaves the reconstruction as it was, except
        the trial count, a camera reset by :691 and - as in the reference - the image's pose when the estimate itself succeeded (:721)."""
        options = options or IncrementalMapperOptions()
        rec = self.reconstruction_
        assert len(rec.RegImageIds()) >= 2
        image = rec.Image(image_id)
        camera = rec.Camera(image.CameraId())
        assert not getattr(image, "registered", True), "Image cannot be registered multiple times"
        self.num_reg_trials_[image_id] = self.num_reg_trials_.get(image_id, 0) + 1      # (:582)
        ransac = ransac_options(max_error=ImageToWorldThreshold(camera, options.abs_pose_max_error), min_inlier_ratio=options.abs_pose_min_inlier_ratio,
                                min_num_trials=100, max_num_trials=10000, confidence=0.99999, seed=self.ransac_seed)      # (:673-681)
        ses = self.triangulator_._open(self._tri_options(options))
        try:
            rep, pose, corrs, mask, lines2D, points3D = ses.estimate_image_pose(image_id, self._device_options(options), ransac)
            self.last_report, self.last_refinement = rep, None
            if rep.failure in (_capi.REG_FEW_VISIBLE, _capi.REG_FEW_CORRS):
                return False
            refinement_options = AbsolutePoseRefinementOptions()      # (:683-714: every branch of the line path leaves both refine flags false)
            refinement_options.print_summary = False
            if self.num_reg_images_per_camera_.get(image.CameraId(), 0) > 0 and \
                    camera.HasBogusParams(options.min_focal_length_ratio, options.max_focal_length_ratio, options.max_extra_param):
                camera.params = self.database_cameras_[image.CameraId()].copy()      # previously refined camera has bogus parameters: reset (:691)
                ses.update()
            if rep.failure in (_capi.REG_NO_INLIERS, _capi.REG_ALIGNED):
                return False
            image.qvec, image.tvec = pose[:4].copy(), pose[4:].copy()      # (pose.cc:86-87: written before the NaN test and before :725)
            if rep.failure != _capi.REG_OK:
                return False
            usable, self.last_refinement = RefineAbsolutePoseFromLines(refinement_options, mask, lines2D, points3D, image.qvec, image.tvec, camera,
                                                                       device=self.device_)
            if not usable:
                return False
            ses.update()      # (a refined camera; the pose goes with the commit)
            ses.register_image(image_id, image.qvec, image.tvec, corrs, mask)
        finally:
            ses.close()
        image.reg_index = self._next_reg_index
        self._next_reg_index += 1
        self.num_reg_images_per_camera_[image.CameraId()] = self.num_reg_images_per_camera_.get(image.CameraId(), 0) + 1      # RegisterImageEvent
        return True
