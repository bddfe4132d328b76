"""The sequential ORACLE of TriangulateImage / CompleteImage - TEST INFRASTRUCTURE.

A literal restatement of IncrementalTriangulator::TriangulateImage, CompleteImage, Find, Continue and Create (reference
src/sfm/incremental_triangulator.cc:63-235, 426-604) and of CorrespondenceGraph::FindTransitiveCorrespondences / IsTwoViewObservation
(src/base/correspondence_graph.cc:166-224, 252-263) over the package's host object model, on top of tracks_reference.TracksOracle (Complete).
Each EstimateTriangulation goes through oracle_lib.triangulate_tracks (orc_triangulate_tracks), one track per call.  The angular error is
CalculateNormalizedLineAngularError (src/base/projection.cc:241-260) restated in Python floats around oracle_lib.world_to_image.  The device never
runs here.

`events`: the (point id, (image_id, line_idx)) pairs in the order the Reconstruction receives them (AddObservation; AddPoint3D's track in track order).
`margin`: the smallest relative distance from its threshold of every final inlier / outlier residual (squared against squared), of every Continue
best angle, and of the gap between the best and the second-best Continue angle (relative to the best; gated errors are DBL_MAX and far away), joined
with TracksOracle's margin over Complete.  `arbitrary`: RANSACs whose best support was exactly 3 out of more than 3 observations - such a winner is
rounding noise in any implementation.  `decisions`: per visited line what happened, for the replay test."""
import math

import numpy as np

import oracle_lib
import tracks_reference as tr
from tracks_reference import DBL_MAX

DEG = 0.0174532925199432954743716805978692718781530857086181640625


def DegToRad(deg):
    return deg * DEG


def NChooseK(n, k):
    return 1 if k == 0 else (n * NChooseK(n - 1, k - 1)) // k if n > 0 else 0


class Options:
    """incremental_triangulator.h:47-87, the fields read here and by Complete"""

    def __init__(self, **kw):
        self.max_transitivity = 1
        self.create_max_angle_error = 2.0
        self.continue_max_angle_error = 2.0
        self.merge_max_reproj_error = 4.0
        self.complete_max_reproj_error = 4.0
        self.complete_max_transitivity = 5
        self.min_angle = 1.5
        self.ignore_two_view_tracks = True
        self.min_focal_length_ratio = 0.1
        self.max_focal_length_ratio = 10.0
        self.max_extra_param = 1.0
        for k, v in kw.items():
            assert hasattr(self, k)
            setattr(self, k, v)


def find_transitive_correspondences(graph, image_id, line_idx, transitivity):
    if transitivity == 1:
        return list(graph.FindCorrespondences(image_id, line_idx))
    found = []
    if not graph.FindCorrespondences(image_id, line_idx):
        return found
    found.append((image_id, line_idx))
    seen = {(image_id, line_idx)}
    begin, end = 0, len(found)
    for _ in range(transitivity):
        for i in range(begin, end):
            for corr in graph.FindCorrespondences(*found[i]):
                if corr not in seen:
                    seen.add(corr)
                    found.append(corr)
        begin, end = end, len(found)
        if begin == end:
            break
    if len(found) > 1:
        found[0] = found[-1]
    found.pop()
    return found


def is_two_view_observation(graph, image_id, line_idx):
    corrs = graph.FindCorrespondences(image_id, line_idx)
    if len(corrs) != 1:
        return False
    return len(graph.FindCorrespondences(*corrs[0])) == 1


def normalized_line_angular_error(line, xyz, P, camera):
    a, b, c = float(line[0]), float(line[1]), float(line[2])
    X0, X1, X2 = float(xyz[0]), float(xyz[1]), float(xyz[2])
    r0 = P[0] * X0 + P[1] * X1 + P[2] * X2 + P[3]
    r1 = P[4] * X0 + P[5] * X1 + P[6] * X2 + P[7]
    r2 = P[8] * X0 + P[9] * X1 + P[10] * X2 + P[11]
    if r2 < 0:
        return DBL_MAX
    ix, iy = oracle_lib.world_to_image(camera.model_id, camera.params, r0 / r2, r1 / r2)
    if ix < 0 or ix >= camera.width or iy < 0 or iy >= camera.height:
        return DBL_MAX
    nl, nr = math.sqrt(a * a + b * b + c * c), math.sqrt(r0 * r0 + r1 * r1 + r2 * r2)
    return abs(math.pi / 2 - math.acos(min(1.0, abs((a * r0 + b * r1 + c * r2) / (nl * nr)))))


class CorrData:
    def __init__(self, image_id, line_idx, image, camera):
        self.image_id, self.line_idx, self.image, self.camera = image_id, line_idx, image, camera
        self.line = image.lines[line_idx]      # (the reference holds a pointer: HasPoint3D() is read live)

    def el(self):
        return (self.image_id, self.line_idx)


class ImageOracle(tr.TracksOracle):
    def __init__(self, correspondence_graph, reconstruction):
        super().__init__(correspondence_graph, reconstruction)
        self.events, self.created, self.decisions = [], [], []
        self.arbitrary = 0
        self.num_ransacs = self.num_continued = 0
        self._views = None

    # ---- EstimateTriangulation through the C++ oracle, one track per call -------------------------------------------------------------------
    def _view_arrays(self):
        if self._views is None:
            rec = self.rec
            iids, cids = sorted(rec.images), sorted(rec.cameras)
            P = np.array([tr.projection_matrix(rec.images[i].qvec, rec.images[i].tvec) for i in iids]).reshape(-1, 12)
            R = P.reshape(-1, 3, 4)[:, :, :3]
            centers = -np.einsum("vji,vj->vi", R, P.reshape(-1, 3, 4)[:, :, 3])      # Image::ProjectionCenter: -R^T t
            intr = np.zeros((len(cids), 12))
            for k, c in enumerate(cids):
                intr[k, : rec.cameras[c].NumParams()] = rec.cameras[c].params
            self._views = dict(index={i: k for k, i in enumerate(iids)}, P=P, centers=centers,
                               view_camera=np.array([cids.index(rec.images[i].camera_id) for i in iids], dtype=np.int32),
                               camera_model=np.array([rec.cameras[c].model_id for c in cids], dtype=np.int32), intr=intr,
                               cam_size=np.array([[rec.cameras[c].width, rec.cameras[c].height] for c in cids], dtype=np.int32))
        return self._views

    def _estimate(self, options, corrs, residual_type, max_error, min_num_trials):
        v = self._view_arrays()
        n = len(corrs)
        sc = dict(v, track_start=np.array([0, n], dtype=np.int32), lines=np.array([c.image.lines[c.line_idx].Line() for c in corrs]).reshape(-1, 3),
                  obs_view=np.array([v["index"][c.image_id] for c in corrs], dtype=np.int32))
        ok, xyz, mask, nt = oracle_lib.triangulate_tracks(sc, DegToRad(options.min_angle), residual_type, max_error=max_error, confidence=0.9999,
                                                          min_inlier_ratio=0.02, max_num_trials=10000, min_num_trials=int(min_num_trials))
        self.num_ransacs += 1
        if not ok[0]:
            return False, None, None
        if mask.sum() == 3 and n > 3:
            self.arbitrary += 1
        thr2 = max_error * max_error
        for c in corrs:
            P = v["P"][v["index"][c.image_id]]
            if residual_type == 0:
                r = normalized_line_angular_error(c.line.Line(), xyz[0], P, c.camera)
                r = r if r == DBL_MAX else r * r
            else:
                r = tr.squared_line_reprojection_error(c.line.Line(), xyz[0], tuple(P), c.camera)
            if r != DBL_MAX:
                self.margin = min(self.margin, abs(r - thr2) / thr2)
        return True, xyz[0].copy(), mask

    def _add_point(self, xyz, track):
        rec = self.rec
        pid = rec.AddPoint3D(xyz, track)
        self.created.append(pid)
        self.events.extend((pid, el) for el in track)
        return pid

    # ---- Find / Continue / Create --------------------------------------------------------------------------------------------------------------
    def Find(self, options, image_id, line_idx, transitivity):
        rec = self.rec
        corrs_data, num_triangulated = [], 0
        for corr in find_transitive_correspondences(self.graph, image_id, line_idx, transitivity):
            corr_image = rec.images[corr[0]]
            if not getattr(corr_image, "registered", True):
                continue
            corr_camera = rec.cameras[corr_image.camera_id]
            if self._bogus(options, corr_camera):
                continue
            cd = CorrData(corr[0], corr[1], corr_image, corr_camera)
            corrs_data.append(cd)
            if cd.line.HasPoint3D():
                num_triangulated += 1
        return num_triangulated, corrs_data

    def Create(self, options, corrs_data):
        create = [c for c in corrs_data if not c.line.HasPoint3D()]
        if len(create) < 3:
            return 0
        num_random_lines = sum(1 for c in create if not c.image.lines[c.line_idx].IsAligned())
        if num_random_lines < 1:
            return 0
        min_num_trials = NChooseK(len(create), 3) if len(create) <= 15 else 0      # (the options are built afresh in every call)
        ok, xyz, mask = self._estimate(options, create, 0, DegToRad(options.create_max_angle_error), min_num_trials)
        if not ok:
            return 0
        track = [c.el() for c, m in zip(create, mask) if m]
        self._add_point(xyz, track)
        if len(create) - len(track) >= 3:
            return len(track) + self.Create(options, create)
        return len(track)

    def Continue(self, options, ref, corrs_data):
        if ref.line.HasPoint3D():
            return 0
        best_angle_error, best_idx = DBL_MAX, None
        P = tr.projection_matrix(ref.image.qvec, ref.image.tvec)
        per_point = {}
        for idx, cd in enumerate(corrs_data):
            if not cd.line.HasPoint3D():
                continue
            angle_error = normalized_line_angular_error(ref.line.Line(), self.rec.points3D[cd.line.Point3DId()].xyz, P, ref.camera)
            per_point[cd.line.Point3DId()] = angle_error      # (neighbours on the SAME point give the same angle and the same decision)
            if angle_error < best_angle_error:
                best_angle_error, best_idx = angle_error, idx
        max_angle_error = DegToRad(options.continue_max_angle_error)
        if best_idx is not None:
            self.margin = min(self.margin, abs(best_angle_error - max_angle_error) / max_angle_error)
            others = sorted(a for a in per_point.values() if a != DBL_MAX)[1:]
            if others:
                self.margin = min(self.margin, (others[0] - best_angle_error) / best_angle_error if best_angle_error > 0 else math.inf)
        if best_angle_error <= max_angle_error and best_idx is not None:
            pid = corrs_data[best_idx].line.Point3DId()
            self.rec.AddObservation(pid, ref.el())
            self.events.append((pid, ref.el()))
            self.num_continued += 1
            return 1
        return 0

    # ---- the two drivers -----------------------------------------------------------------------------------------------------------------------
    def _enter(self, options, image_id):
        self.clear_caches()
        self._views = None
        image = self.rec.images[image_id]
        if not getattr(image, "registered", True):
            return None
        camera = self.rec.cameras[image.camera_id]
        if self._bogus(options, camera):
            return None
        return image, camera

    def TriangulateImage(self, options, image_id, line_indices=None):
        """`line_indices`: visit these lines only (the replay test asks for one line on the untouched state: what a speculation answers)"""
        num_tris = 0
        entered = self._enter(options, image_id)
        if entered is None:
            return num_tris
        image, camera = entered
        for line_idx in (range(len(image.lines)) if line_indices is None else line_indices):
            num_triangulated, corrs_data = self.Find(options, image_id, line_idx, options.max_transitivity)
            if not corrs_data:
                continue
            ref = CorrData(image_id, line_idx, image, camera)
            e0, c0 = len(self.events), len(self.created)
            continued = 0
            if num_triangulated == 0:
                corrs_data.append(ref)
                num_tris += self.Create(options, corrs_data)
            else:
                continued = self.Continue(options, ref, corrs_data)
                num_tris += continued
                corrs_data.append(ref)
                num_tris += self.Create(options, corrs_data)
            self.decisions.append(dict(line=(image_id, line_idx), list=[c.el() for c in corrs_data[:-1]], continued=continued, events=self.events[e0:],
                                       created=self.created[c0:]))
        return num_tris

    def CompleteImage(self, options, image_id):
        num_tris = 0
        entered = self._enter(options, image_id)
        if entered is None:
            return num_tris
        image, camera = entered
        min_num_trials = 0      # ONE options object over the loop (:142-149): the value a short set left behind stays for a long one
        max_error = options.complete_max_reproj_error
        for line_idx in range(len(image.lines)):
            line = image.lines[line_idx]
            if line.HasPoint3D():
                c0 = len(self.completed)
                num_tris += self.Complete(options, line.Point3DId())
                self.events.extend(self.completed[c0:])
                continue
            if options.ignore_two_view_tracks and is_two_view_observation(self.graph, image_id, line_idx):
                continue
            num_triangulated, corrs_data = self.Find(options, image_id, line_idx, options.max_transitivity)
            if num_triangulated or not corrs_data:
                continue
            corrs_data.append(CorrData(image_id, line_idx, image, camera))
            if len(corrs_data) <= 15:
                min_num_trials = NChooseK(len(corrs_data), 2)
            ok, xyz, mask = self._estimate(options, corrs_data, 1, max_error, min_num_trials)
            if not ok:
                continue
            track = [c.el() for c, m in zip(corrs_data, mask) if m]
            num_tris += len(track)
            self._add_point(xyz, track)
        return num_tris
