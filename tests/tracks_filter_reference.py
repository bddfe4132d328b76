"""Plain-Python reference of the deletions on a live tracks handle - TEST INFRASTRUCTURE (tests/test_tracks_filter_reference.py, the host replay test and
tests/test_gpu_tracks_filter.py share it).  Everything runs on a `Reconstruction`; the device never runs here.

  filter_points                     Reconstruction::FilterPoints3D / FilterPoints3DInImages / FilterAllPoints3D (base/reconstruction.cc:412-439, 594-719): the
                                    verdicts are oracle_lib.filter_points3d's on rec._filter_scene(), as tests/local_refinement_oracle.filter_points
  delete_observation                Reconstruction::DeleteObservation WITH the "track of at most three elements -> the point goes" rule (:255-275)
  filter_negative_depth             FilterObservationsWithNegativeDepth in the reference's order (:442-460): images in registration order, lines ascending
  deregister_image / filter_images  :285-300, :462-484

EVENTS are what the handle reports, in ids: (point id, (image_id, line_idx)) for one deleted observation, (point id, None) for a deleted point.  The point
filter visits the points in ascending id and a point's elements in track order; a point the rules delete gives one (id, None).
MARGINS: the smallest relative distance of a tested pixel error from max_reproj_error and of a tested angle from min_tri_angle (every pair of surviving
elements, a superset of what an early exit looks at), computed here in numpy with the camera model of oracle_lib.world_to_image."""
import numpy as np

import oracle_lib
from privacy_preserving_sfm_amd.bundle_adjustment import _quat_to_rot

EPS = float(np.finfo(np.float64).eps)


def proj_matrix(image):
    q = np.asarray(image.qvec, dtype=np.float64)
    return _quat_to_rot(q / np.linalg.norm(q)), np.asarray(image.tvec, dtype=np.float64)


def projection_center(image):
    R, t = proj_matrix(image)
    return -R.T @ t


def squared_line_error(rec, image_id, line_idx, X):
    """CalculateSquaredLineReprojectionError (base/projection.cc:162-203) -> squared pixel error, inf behind the camera or outside the image"""
    image = rec.images[image_id]
    cam = rec.cameras[image.camera_id]
    R, t = proj_matrix(image)
    p = R @ X + t
    if p[2] < EPS:
        return np.inf
    u, v = p[0] / p[2], p[1] / p[2]
    a, b, c = image.lines[line_idx].Line()
    alpha = a * u + b * v + c
    ix, iy = oracle_lib.world_to_image(cam.model_id, cam.params, u, v)
    if not (0 <= ix < cam.width and 0 <= iy < cam.height):
        return np.inf
    jx, jy = oracle_lib.world_to_image(cam.model_id, cam.params, u - a * alpha, v - b * alpha)
    return (ix - jx) ** 2 + (iy - jy) ** 2


def triangulation_angle(c1, c2, X):
    """CalculateTriangulationAngle (base/triangulation.cc:59-82)"""
    b2, r1, r2 = np.sum((c1 - c2) ** 2), np.sum((X - c1) ** 2), np.sum((X - c2) ** 2)
    den = 2.0 * np.sqrt(r1 * r2)
    if den == 0.0:
        return 0.0
    ang = abs(np.arccos(np.clip((r1 + r2 - b2) / den, -1.0, 1.0)))
    return min(ang, np.pi - ang)


def delete_observation(rec, image_id, line_idx, events):
    """-> the number of track elements removed"""
    pid = rec.images[image_id].lines[line_idx].Point3DId()
    n = len(rec.points3D[pid].track)
    if n <= 3:
        rec.DeletePoint3D(pid)
        events.append((pid, None))
        return n
    rec.DeleteObservation(image_id, line_idx)      # (the package's: removes that one element)
    events.append((pid, (image_id, line_idx)))
    return 1


def points_in_images(rec, image_ids):
    return set(l.Point3DId() for i in image_ids for l in rec.images[i].lines if l.HasPoint3D())


def filter_points(rec, max_reproj_error, min_tri_angle, point3D_ids=None, image_ids=None):
    """-> dict(num_filtered, events, point_deleted, obs_deleted, errors {id: Point3D.error set}, tested, by_angle (points the angle rule deleted),
    verdicts {id of a tested point: (1 kept | 2 deleted by a track rule | 3 deleted by the angle rule, elements above the threshold, their flags in track order)},
    margin_error, margin_angle)"""
    out = dict(num_filtered=0, events=[], point_deleted=0, obs_deleted=0, errors={}, tested=0, by_angle=0, verdicts={}, margin_error=np.inf, margin_angle=np.inf)
    assert point3D_ids is None or image_ids is None
    if image_ids is not None:
        point3D_ids = points_in_images(rec, image_ids)
    scene, aligned, cam_size, point_ids, obs_ref = rec._filter_scene()
    if len(obs_ref) == 0:
        return out
    wanted = None if point3D_ids is None else set(point3D_ids)
    subset = None if wanted is None else np.array([p in wanted for p in point_ids], dtype=np.uint8)
    nf, od, pd, pe = oracle_lib.filter_points3d(scene, max_reproj_error, min_tri_angle, cam_size, aligned, point_subset=subset)
    out["num_filtered"] = nf
    min_rad = np.deg2rad(min_tri_angle)
    o = 0
    for k, pid in enumerate(point_ids):
        track = list(rec.points3D[pid].track)
        flags = od[o:o + len(track)]
        o += len(track)
        if (wanted is not None and pid not in wanted) or not track:
            continue
        out["tested"] += 1
        X = rec.points3D[pid].xyz
        errs = [squared_line_error(rec, i, x, X) for (i, x) in track]
        for e in errs:
            if np.isfinite(e) and max_reproj_error > 0:
                out["margin_error"] = min(out["margin_error"], abs(np.sqrt(e) - max_reproj_error) / max_reproj_error)
        bad = [e > max_reproj_error ** 2 for e in errs]
        reached = any(not rec.images[i].lines[x].IsAligned() for (i, x) in track) and len(track) >= 3 and sum(bad) < len(track) - 3
        assert reached or pd[k], pid
        if reached:      # the point reached the angle test: the survivors' pairs
            assert pd[k] or [bool(f) for f in flags] == bad, (pid, list(flags), bad)
            centers = [projection_center(rec.images[i]) for (i, _), b in zip(track, bad) if not b]
            for i1 in range(len(centers)):
                for i2 in range(i1):
                    ang = triangulation_angle(centers[i1], centers[i2], X)
                    if min_rad > 0:
                        out["margin_angle"] = min(out["margin_angle"], abs(ang - min_rad) / min_rad)
        out["verdicts"][pid] = ((3 if reached else 2) if pd[k] else 1, sum(bad), [int(b) for b in bad])
        if pd[k]:
            out["by_angle"] += bool(reached)
            out["events"].append((pid, None))
            out["point_deleted"] += 1
            out["obs_deleted"] += len(track)
            rec.DeletePoint3D(pid)
            continue
        for el, f in zip(track, flags):
            if f:
                out["obs_deleted"] += delete_observation(rec, el[0], el[1], out["events"])
        rec.points3D[pid].error = float(pe[k])
        out["errors"][pid] = float(pe[k])
    return out


def has_negative_depth(rec, image_id, X):
    R, t = proj_matrix(rec.images[image_id])
    return not (R[2] @ X + t[2] >= EPS)      # !HasPointPositiveDepth


def filter_negative_depth(rec):
    """-> dict(num_filtered, events, point_deleted, obs_deleted, margin_depth = the smallest |depth| tested)"""
    out = dict(num_filtered=0, events=[], point_deleted=0, obs_deleted=0, margin_depth=np.inf)
    for image_id in rec.RegImageIds():
        image = rec.images[image_id]
        R, t = proj_matrix(image)
        for idx, line in enumerate(image.lines):
            if not line.HasPoint3D():
                continue
            X = rec.points3D[line.Point3DId()].xyz
            out["margin_depth"] = min(out["margin_depth"], abs(R[2] @ X + t[2]))
            if has_negative_depth(rec, image_id, X):
                n = delete_observation(rec, image_id, idx, out["events"])
                out["obs_deleted"] += n
                out["point_deleted"] += out["events"][-1][1] is None
                out["num_filtered"] += 1
    return out


def deregister_image(rec, image_id, out):
    image = rec.images[image_id]
    for idx, line in enumerate(image.lines):
        if line.HasPoint3D():
            out["obs_deleted"] += delete_observation(rec, image_id, idx, out["events"])
            out["point_deleted"] += out["events"][-1][1] is None
    image.registered = False
    if hasattr(image, "reg_index"):
        del image.reg_index


def filter_images(rec, min_focal_length_ratio=0.1, max_focal_length_ratio=10.0, max_extra_param=1.0):
    """-> dict(filtered [image ids in the order they were de-registered], events, point_deleted, obs_deleted, num_filtered)"""
    out = dict(filtered=[], events=[], point_deleted=0, obs_deleted=0)
    for image_id in rec.RegImageIds():
        image = rec.images[image_id]
        if not any(l.HasPoint3D() for l in image.lines) or \
                rec.cameras[image.camera_id].HasBogusParams(min_focal_length_ratio, max_focal_length_ratio, max_extra_param):
            out["filtered"].append(image_id)
    for image_id in out["filtered"]:
        deregister_image(rec, image_id, out)
    out["num_filtered"] = len(out["filtered"])
    return out


def run_op(rec, op):
    """one entry of a scene's `ops`: ("points", dict(point3D_ids= | image_ids=, max_reproj_error=, min_tri_angle=)) | ("depth", {}) | ("images", {})"""
    kind, kw = op
    if kind == "points":
        return filter_points(rec, kw.get("max_reproj_error", 4.0), kw.get("min_tri_angle", 1.5), kw.get("point3D_ids"), kw.get("image_ids"))
    if kind == "depth":
        return filter_negative_depth(rec)
    assert kind == "images"
    return filter_images(rec)


class Indexed:
    """the handle's numbering of a scene (IncrementalTriangulator.flatten at the start: lines image by image, points in id order; the filters create no
    point) - to put the reference's ids beside the handle's indices"""

    def __init__(self, rec, graph):
        from privacy_preserving_sfm_amd.incremental_triangulator import IncrementalTriangulator
        self.rec = rec
        self.flat, self.point_ids, self.line_ref = IncrementalTriangulator(graph, rec).flatten()
        self.image_ids = sorted(rec.images)
        self.point_index = {p: k for k, p in enumerate(self.point_ids)}
        self.line_index = {ref: l for l, ref in enumerate(self.line_ref)}
        self.image_index = {i: c for c, i in enumerate(self.image_ids)}

    def events(self, events):
        return [(self.point_index[p], -1 if el is None else self.line_index[el]) for p, el in events]

    def image_order(self):
        return [self.image_index[i] for i in self.rec.RegImageIds()]

    def point_flags(self, ids):
        return None if ids is None else np.array([p in set(ids) for p in self.point_ids], dtype=np.uint8)

    def image_flags(self, ids):
        return None if ids is None else np.array([i in set(ids) for i in self.image_ids], dtype=np.uint8)

    def state(self):
        """-> (line_point [L], deleted [P], tracks [P lists]) of the reconstruction as it is now"""
        rec = self.rec
        tracks = [[self.line_index[el] for el in rec.points3D[p].track] if p in rec.points3D else [] for p in self.point_ids]
        line_point = np.full(len(self.line_ref), -1, dtype=np.int32)
        for k, t in enumerate(tracks):
            line_point[t] = k
        return line_point, np.array([len(t) == 0 for t in tracks], dtype=np.uint8), tracks

    def depth_flags(self):
        """K14b's output on the current state: a line with a point, in a registered image, whose point has no positive depth there"""
        rec = self.rec
        reg = set(rec.RegImageIds())
        return np.array([int(i in reg and rec.images[i].lines[x].HasPoint3D() and has_negative_depth(rec, i, rec.points3D[rec.images[i].lines[x].Point3DId()].xyz))
                         for (i, x) in self.line_ref], dtype=np.uint8)

    def skip_flags(self, o=None):
        rec = self.rec
        return np.array([int(rec.cameras[rec.images[i].camera_id].HasBogusParams(0.1, 10.0, 1.0)) for i in self.image_ids], dtype=np.uint8)
