"""The sequential ORACLE of track completion and merging - TEST INFRASTRUCTURE.

A literal restatement of IncrementalTriangulator::Complete / Merge and their four drivers (reference src/sfm/incremental_triangulator.cc:237-293,
606-765) over the package's host object model (Reconstruction, CorrespondenceGraph), visiting the points in ASCENDING ID order (the reference's
unordered_set order is unspecified; the device pins the same order).  The pixel line error is CalculateSquaredLineReprojectionError
(src/base/projection.cc:162-203) restated in Python floats around oracle_lib.world_to_image.  The device never runs here.

Every (point id, (image_id, line_idx), squared error, squared threshold) tested is recorded in `tested`; `margin` is the smallest relative
distance of a tested squared error from its squared threshold (gated errors - behind the camera, outside the image - are DBL_MAX and far away)."""
import math
import sys

import oracle_lib

DBL_MAX = sys.float_info.max
DBL_EPS = sys.float_info.epsilon


class Options:
    """incremental_triangulator.h:57-87, the fields read here"""

    def __init__(self, **kw):
        self.merge_max_reproj_error = 4.0
        self.complete_max_reproj_error = 4.0
        self.complete_max_transitivity = 5
        self.min_focal_length_ratio = 0.1
        self.max_focal_length_ratio = 10.0
        self.max_extra_param = 1.0
        for k, v in kw.items():
            assert hasattr(self, k)
            setattr(self, k, v)


def projection_matrix(qvec, tvec):
    """ComposeProjectionMatrix: QuaternionToRotationMatrix(NormalizeQuaternion(q)) | t, as 12 floats row-major"""
    n = math.sqrt(qvec[0] * qvec[0] + qvec[1] * qvec[1] + qvec[2] * qvec[2] + qvec[3] * qvec[3])
    w, x, y, z = qvec[0] / n, qvec[1] / n, qvec[2] / n, qvec[3] / n
    return (1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), float(tvec[0]),
            2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w), float(tvec[1]),
            2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y), float(tvec[2]))


def squared_line_reprojection_error(line, xyz, P, camera):
    a, b, c = float(line[0]), float(line[1]), float(line[2])
    X0, X1, X2 = float(xyz[0]), float(xyz[1]), float(xyz[2])
    pz = P[8] * X0 + P[9] * X1 + P[10] * X2 + P[11]
    if pz < DBL_EPS:
        return DBL_MAX
    px = P[0] * X0 + P[1] * X1 + P[2] * X2 + P[3]
    py = P[4] * X0 + P[5] * X1 + P[6] * X2 + P[7]
    inv = 1.0 / pz
    u, v = inv * px, inv * py
    alpha = a * u + b * v + c
    lu, lv = u - a * alpha, v - b * alpha
    ix, iy = oracle_lib.world_to_image(camera.model_id, camera.params, u, v)
    if not (ix >= 0 and ix < camera.width and iy >= 0 and iy < camera.height):
        return DBL_MAX
    jx, jy = oracle_lib.world_to_image(camera.model_id, camera.params, lu, lv)
    return (ix - jx) * (ix - jx) + (iy - jy) * (iy - jy)


class TracksOracle:
    def __init__(self, correspondence_graph, reconstruction):
        self.graph, self.rec = correspondence_graph, reconstruction
        self.tested = []
        self.margin = math.inf
        self.merge_trials = {}
        self.bogus = {}
        self.proj = {}
        self.completed, self.merged = [], []      # [(point id, (image_id, line_idx))], [(id a, id b, new id)] in order

    def clear_caches(self):
        self.merge_trials, self.bogus, self.proj = {}, {}, {}      # (the poses may have moved since the last driver call)

    def _error(self, point_id, xyz, track_el, max2):
        iid, idx = track_el
        image = self.rec.images[iid]
        if iid not in self.proj:
            self.proj[iid] = projection_matrix(image.qvec, image.tvec)
        e = squared_line_reprojection_error(image.lines[idx].Line(), xyz, self.proj[iid], self.rec.cameras[image.camera_id])
        self.tested.append((point_id, track_el, e, max2))
        if max2 > 0:
            self.margin = min(self.margin, abs(e - max2) / max2)
        return e

    def _bogus(self, options, camera):
        if camera.camera_id not in self.bogus:
            self.bogus[camera.camera_id] = camera.HasBogusParams(options.min_focal_length_ratio, options.max_focal_length_ratio, options.max_extra_param)
        return self.bogus[camera.camera_id]

    def Complete(self, options, point3D_id):
        rec = self.rec
        num_completed = 0
        if point3D_id not in rec.points3D:
            return num_completed
        max2 = options.complete_max_reproj_error * options.complete_max_reproj_error
        point3D = rec.points3D[point3D_id]
        queue = list(point3D.track)
        max_transitivity = options.complete_max_transitivity
        for transitivity in range(max_transitivity):
            if not queue:
                break
            prev_queue, queue = queue, []
            for queue_elem in prev_queue:
                for corr in self.graph.FindCorrespondences(*queue_elem):
                    image = rec.images[corr[0]]
                    if not getattr(image, "registered", True):
                        continue
                    line = image.lines[corr[1]]
                    if line.HasPoint3D():
                        continue
                    if self._bogus(options, rec.cameras[image.camera_id]):
                        continue
                    if self._error(point3D_id, point3D.xyz, corr, max2) > max2:
                        continue
                    rec.AddObservation(point3D_id, corr)
                    self.completed.append((point3D_id, corr))
                    if transitivity < max_transitivity - 1:
                        queue.append(corr)
                    num_completed += 1
        return num_completed

    def Merge(self, options, point3D_id):
        rec = self.rec
        if point3D_id not in rec.points3D:
            return 0
        max2 = options.merge_max_reproj_error * options.merge_max_reproj_error
        point3D = rec.points3D[point3D_id]
        for track_el in list(point3D.track):
            for corr in self.graph.FindCorrespondences(*track_el):
                image = rec.images[corr[0]]
                if not getattr(image, "registered", True):
                    continue
                corr_line = image.lines[corr[1]]
                other = corr_line.Point3DId()
                if not corr_line.HasPoint3D() or other == point3D_id or other in self.merge_trials.setdefault(point3D_id, set()):
                    continue
                corr_point3D = rec.points3D[other]
                self.merge_trials[point3D_id].add(other)
                self.merge_trials.setdefault(other, set()).add(point3D_id)
                l1, l2 = float(len(point3D.track)), float(len(corr_point3D.track))
                merged_xyz = (l1 * point3D.xyz + l2 * corr_point3D.xyz) / (l1 + l2)
                merge_success = True
                for track in (point3D.track, corr_point3D.track):
                    for test_track_el in track:
                        if self._error((point3D_id, other), merged_xyz, test_track_el, max2) > max2:
                            merge_success = False
                            break
                    if not merge_success:
                        break
                if merge_success:
                    num_merged = len(point3D.track) + len(corr_point3D.track)
                    merged_id = rec.MergePoints3D(point3D_id, other)
                    self.merged.append((point3D_id, other, merged_id))
                    num_merged_recursive = self.Merge(options, merged_id)
                    return num_merged_recursive if num_merged_recursive > 0 else num_merged
        return 0

    def _ids(self, point3D_ids):
        return sorted(self.rec.points3D) if point3D_ids is None else sorted(set(point3D_ids))

    def CompleteTracks(self, options, point3D_ids=None):
        self.clear_caches()
        return sum(self.Complete(options, p) for p in self._ids(point3D_ids))

    def CompleteAllTracks(self, options):
        return self.CompleteTracks(options, None)

    def MergeTracks(self, options, point3D_ids=None):
        self.clear_caches()
        return sum(self.Merge(options, p) for p in self._ids(point3D_ids))

    def MergeAllTracks(self, options):
        return self.MergeTracks(options, None)


def state(rec):
    """comparable snapshot: {point id: (xyz tuple, track list)} and {(image_id, line_idx): point id}"""
    return ({p: (tuple(float(v) for v in pt.xyz), list(pt.track)) for p, pt in rec.points3D.items()},
            {(iid, idx): l.Point3DId() for iid, im in rec.images.items() for idx, l in enumerate(im.lines) if l.HasPoint3D()})
