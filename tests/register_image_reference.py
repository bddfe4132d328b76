"""The sequential ORACLE of FindNextImages / RegisterNextImage - TEST INFRASTRUCTURE.

A line-by-line restatement of IncrementalMapper::FindNextImages (reference src/sfm/incremental_mapper.cc:139-190, with SortAndAppendNextImages
:50-64 and the two rank functions :66-73) and RegisterNextImage (:570-760) over the package's host object model (Reconstruction,
CorrespondenceGraph), of what EstimateAbsolutePoseFromLines does with the RANSAC report (src/estimators/pose.cc:52-94), and of the two counters
the ranking reads: Image::NumObservations (CorrespondenceGraph::Finalize, src/base/correspondence_graph.cc:58-65: lines whose correspondence list
is not empty) and Image::NumVisiblePoints3D (src/base/image.cc:91-98 with src/base/reconstruction.cc:1112-1115: lines with at least one direct
correspondence that has a point), both recomputed from scratch here.  The pose estimator, the refinement and ImageToWorldThreshold are passed in as
callables.  The device never runs here.

PINNED where the reference is unspecified: it iterates reconstruction_->Images(), an unordered_map, and std::sort is not stable - equal ranks are
ordered by ASCENDING IMAGE ID (the library's pin).  The rank is a float (numpy float32), as in the reference.

`failure`: which `return false` was taken - 1 :585, 2 :653-657, 3 pose.cc:65, 4 pose.cc:81, 5 pose.cc:89, 6 :725, 7 the refinement (:733-737);
0 = registered."""
import numpy as np

OK, FEW_VISIBLE, FEW_CORRS, NO_INLIERS, ALIGNED, NAN, FEW_INLIERS, REFINEMENT = range(8)
MAX_VISIBLE_POINTS_NUM, MAX_VISIBLE_POINTS_RATIO = 0, 1


class Options:
    """IncrementalMapper::Options (sfm/incremental_mapper.h:40-113), the fields read here, with the reference's defaults"""

    def __init__(self, **kw):
        self.abs_pose_max_error = 12.0
        self.abs_pose_min_num_inliers = 30
        self.abs_pose_min_inlier_ratio = 0.25
        self.abs_pose_refine_focal_length = False
        self.abs_pose_refine_extra_params = False
        self.min_focal_length_ratio = 0.1
        self.max_focal_length_ratio = 10.0
        self.max_extra_param = 1.0
        self.max_reg_trials = 3
        self.image_selection_method = MAX_VISIBLE_POINTS_RATIO
        for k, v in kw.items():
            assert hasattr(self, k)
            setattr(self, k, v)


class RANSACOptions:
    def __init__(self):
        self.max_error, self.min_inlier_ratio, self.confidence, self.dyn_num_trials_multiplier = 0.0, 0.1, 0.99, 3.0
        self.min_num_trials, self.max_num_trials = 0, 2**64 - 1

    def Check(self):
        assert self.max_error > 0 and 0 <= self.min_inlier_ratio <= 1 and 0 <= self.confidence <= 1 and self.min_num_trials <= self.max_num_trials


class RefinementOptions:
    """AbsolutePoseRefinementOptions (src/estimators/pose.h:84-108)"""

    def __init__(self):
        self.gradient_tolerance, self.max_num_iterations, self.loss_function_scale = 1.0, 100, 1.0
        self.refine_focal_length = self.refine_extra_params = False
        self.print_summary = True

    def Check(self):
        assert self.gradient_tolerance >= 0.0 and self.max_num_iterations >= 0 and self.loss_function_scale >= 0.0


def is_registered(image):
    return getattr(image, "registered", True)


def num_observations(graph, image):
    return sum(1 for idx in range(len(image.lines)) if len(graph.FindCorrespondences(image.image_id, idx)) > 0)


def num_visible_points3D(rec, graph, image):
    n = 0
    for idx in range(len(image.lines)):
        if any(rec.images[i2].lines[x2].HasPoint3D() for (i2, x2) in graph.FindCorrespondences(image.image_id, idx)):
            n += 1
    return n


def rank_num(rec, graph, image):
    return np.float32(num_visible_points3D(rec, graph, image))


def rank_ratio(rec, graph, image):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(num_visible_points3D(rec, graph, image)) / np.float32(num_observations(graph, image))


def sort_and_append_next_images(image_ranks, sorted_image_ids):
    for image_id, _ in sorted(image_ranks, key=lambda e: (-float(e[1]), e[0])):      # descending rank; the pin: equal ranks by ascending id
        sorted_image_ids.append(image_id)


def rotation_matrix_to_quaternion(R):
    """base/pose.cc:41-51: Eigen::Quaterniond(rot_mat) as (w, x, y, z)"""
    t = R[0][0] + R[1][1] + R[2][2]
    q = [0.0, 0.0, 0.0, 0.0]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1], q[2], q[3] = (R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t
    else:
        i = 0
        if R[1][1] > R[0][0]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[k][j] - R[j][k]) * t
        q[1 + j] = (R[j][i] + R[i][j]) * t
        q[1 + k] = (R[k][i] + R[i][k]) * t
    return np.array(q, dtype=np.float64)


def estimate_absolute_pose_from_lines(ransac, options, lines2D, points3D):
    """pose.cc:52-94 around `ransac(options, lines2D, points3D) -> (num_inliers, inlier_mask, model 3x4)`
    -> (site, qvec, tvec, num_inliers, inlier_mask): site 0 = true, else the failure code of the `return false` taken"""
    options.Check()
    num_inliers, inlier_mask, model = ransac(options, lines2D, points3D)
    if num_inliers == 0:
        return NO_INLIERS, None, None, num_inliers, inlier_mask
    num_aligned_inliers = 0
    for i in range(len(lines2D)):
        if inlier_mask[i] and lines2D[i].IsAligned():
            num_aligned_inliers += 1
    if num_aligned_inliers > num_inliers * 0.9:
        return ALIGNED, None, None, num_inliers, inlier_mask
    model = np.asarray(model, dtype=np.float64).reshape(3, 4)
    qvec, tvec = rotation_matrix_to_quaternion(model[:, :3]), model[:, 3].copy()
    if np.isnan(qvec).any() or np.isnan(tvec).any():
        return NAN, None, None, num_inliers, inlier_mask
    return OK, qvec, tvec, num_inliers, inlier_mask


class Mapper:
    """the state IncrementalMapper keeps between the two calls: num_reg_trials_, filtered_images_, num_reg_images_per_camera_"""

    def __init__(self, rec, graph, database_cameras=None):
        self.rec, self.graph = rec, graph
        self.database_cameras = database_cameras or {}      # camera id -> params (database_cache_->Camera(id).Params())
        self.num_reg_trials = {}
        self.filtered_images = set()
        self.num_reg_images_per_camera = {}
        for image in rec.images.values():
            if is_registered(image):
                self.num_reg_images_per_camera[image.camera_id] = self.num_reg_images_per_camera.get(image.camera_id, 0) + 1
        self.modified_point3D_ids = []      # triangulator_->AddModifiedPoint3D, in order
        self.last = None                    # what the last register_next_image saw

    def find_next_images(self, options):
        rec, graph = self.rec, self.graph
        rank_image_func = rank_num if options.image_selection_method == MAX_VISIBLE_POINTS_NUM else rank_ratio
        image_ranks, other_image_ranks = [], []
        for image_id in sorted(rec.images):
            image = rec.images[image_id]
            if is_registered(image):
                continue
            if num_visible_points3D(rec, graph, image) < options.abs_pose_min_num_inliers:
                continue
            num_reg_trials = self.num_reg_trials.get(image_id, 0)
            if num_reg_trials >= options.max_reg_trials:
                continue
            rank = rank_image_func(rec, graph, image)
            if image_id not in self.filtered_images and num_reg_trials == 0:
                image_ranks.append((image_id, rank))
            else:
                other_image_ranks.append((image_id, rank))
        ranked_images_ids = []
        sort_and_append_next_images(image_ranks, ranked_images_ids)
        sort_and_append_next_images(other_image_ranks, ranked_images_ids)
        return ranked_images_ids

    def search(self, options, image_id):
        """:601-647 -> (tri_corrs [(line_idx, point3D_id)], tri_lines2D [FeatureLine], tri_points3D [xyz])"""
        rec, graph = self.rec, self.graph
        image = rec.images[image_id]
        tri_corrs, tri_lines2D, tri_points3D = [], [], []
        for line_idx in range(len(image.lines)):
            line = image.lines[line_idx]
            corrs = graph.FindTransitiveCorrespondences(image_id, line_idx, 1)
            point3D_ids = set()
            for (corr_image_id, corr_line_idx) in corrs:
                corr_image = rec.images[corr_image_id]
                if not is_registered(corr_image):
                    continue
                corr_line = corr_image.lines[corr_line_idx]
                if not corr_line.HasPoint3D():
                    continue
                if corr_line.Point3DId() in point3D_ids:
                    continue
                corr_camera = rec.cameras[corr_image.camera_id]
                if corr_camera.HasBogusParams(options.min_focal_length_ratio, options.max_focal_length_ratio, options.max_extra_param):
                    continue
                point3D = rec.points3D[corr_line.Point3DId()]
                tri_corrs.append((line_idx, corr_line.Point3DId()))
                point3D_ids.add(corr_line.Point3DId())
                tri_lines2D.append(line)
                tri_points3D.append(point3D.xyz.copy())
        return tri_corrs, tri_lines2D, tri_points3D

    def commit(self, image_id, tri_corrs, inlier_mask):
        """:743-757 -> the (point3D_id, (image_id, line_idx)) pairs handed to AddObservation, in order"""
        rec = self.rec
        image = rec.images[image_id]
        image.registered = True                                                   # reconstruction_->RegisterImage
        self.num_reg_images_per_camera[image.camera_id] = self.num_reg_images_per_camera.get(image.camera_id, 0) + 1      # RegisterImageEvent
        events = []
        for i in range(len(inlier_mask)):
            if inlier_mask[i]:
                line_idx = tri_corrs[i][0]
                if not image.lines[line_idx].HasPoint3D():
                    point3D_id = tri_corrs[i][1]
                    rec.AddObservation(point3D_id, (image_id, line_idx))
                    self.modified_point3D_ids.append(point3D_id)
                    events.append((point3D_id, (image_id, line_idx)))
        return events

    def register_next_image(self, options, image_id, estimate, refine, image_to_world_threshold):
        """estimate(ransac_options, tri_lines2D, tri_points3D) -> (site, qvec, tvec, num_inliers, inlier_mask) as estimate_absolute_pose_from_lines;
        refine(refinement_options, inlier_mask, tri_lines2D_params, tri_points3D, qvec, tvec, camera) -> bool, qvec / tvec / camera updated in place;
        image_to_world_threshold(camera, pixels) -> Camera::ImageToWorldThreshold.  -> True / False; self.last has the details"""
        rec = self.rec
        assert sum(1 for im in rec.images.values() if is_registered(im)) >= 2
        image = rec.images[image_id]
        camera = rec.cameras[image.camera_id]
        assert not is_registered(image), "Image cannot be registered multiple times"
        self.num_reg_trials[image_id] = self.num_reg_trials.get(image_id, 0) + 1
        last = self.last = dict(failure=OK, tri_corrs=[], num_visible=num_visible_points3D(rec, self.graph, image), events=[])
        if last["num_visible"] < options.abs_pose_min_num_inliers:
            last["failure"] = FEW_VISIBLE
            return False
        tri_corrs, tri_lines2D, tri_points3D = self.search(options, image_id)
        tri_lines2D_params = [l.Line() for l in tri_lines2D]
        last.update(tri_corrs=tri_corrs, tri_lines2D=tri_lines2D, tri_points3D=tri_points3D)
        if len(tri_lines2D) < options.abs_pose_min_num_inliers or len(tri_lines2D) < 6:
            last["failure"] = FEW_CORRS
            return False
        ransac_options = RANSACOptions()
        ransac_options.max_error = image_to_world_threshold(camera, options.abs_pose_max_error)
        ransac_options.min_inlier_ratio = options.abs_pose_min_inlier_ratio
        ransac_options.min_num_trials = 100
        ransac_options.max_num_trials = 10000
        ransac_options.confidence = 0.99999
        last["ransac_options"] = ransac_options
        refinement_options = RefinementOptions()
        if self.num_reg_images_per_camera.get(image.camera_id, 0) > 0:
            if camera.HasBogusParams(options.min_focal_length_ratio, options.max_focal_length_ratio, options.max_extra_param):
                camera.params = np.asarray(self.database_cameras[image.camera_id], dtype=np.float64).copy()
            refinement_options.refine_focal_length = False
            refinement_options.refine_extra_params = False
        else:
            refinement_options.refine_focal_length = False
            refinement_options.refine_extra_params = False
        if not options.abs_pose_refine_focal_length:
            refinement_options.refine_focal_length = False
        if not options.abs_pose_refine_extra_params:
            refinement_options.refine_extra_params = False
        site, qvec, tvec, num_inliers, inlier_mask = estimate(ransac_options, tri_lines2D, tri_points3D)
        last.update(num_inliers=num_inliers, inlier_mask=inlier_mask)
        if site != OK:
            last["failure"] = site
            return False
        image.qvec, image.tvec = np.array(qvec, dtype=np.float64), np.array(tvec, dtype=np.float64)
        last["estimated_pose"] = np.concatenate([image.qvec, image.tvec])
        if num_inliers < options.abs_pose_min_num_inliers:
            last["failure"] = FEW_INLIERS
            return False
        if not refine(refinement_options, inlier_mask, tri_lines2D_params, tri_points3D, image.qvec, image.tvec, camera):
            last["failure"] = REFINEMENT
            return False
        last["events"] = self.commit(image_id, tri_corrs, inlier_mask)
        return True
