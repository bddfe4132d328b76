"""IncrementalMapper::FindLocalBundle in plain Python - TEST INFRASTRUCTURE, written from the reference (src/sfm/incremental_mapper.cc:993-1160,
CalculateTriangulationAngles base/triangulation.cc:84-118, Percentile util/math.h:232-246) on the Reconstruction object model, independent of
csrc/local_bundle_replay.hpp and of the kernels.

Pinned where the reference is unspecified, as include/ppsfm_hip.h states it: equal counts are ordered by ascending image id (the reference sorts the
content of an unordered_map); a NaN angle sorts above every number in the percentile, and a NaN percentile fails every `>=`.

`margin` is the smallest relative distance |angle - threshold| / threshold over every (angle, threshold) comparison the loop makes: a result whose
margin is far above the arithmetic's error (a few 1e-13) cannot depend on who computed the angle."""
import math

import numpy as np

DEG = 0.0174532925199432954743716805978692718781530857086181640625
SELECTION = ((1.0, 0.6), (1.5, 0.6), (2.0, 0.5), (2.5, 0.4), (3.0, 0.3), (4.0, 0.2), (5.0, 0.1), (6.0, 0.1))


class Options:
    def __init__(self, local_ba_num_images=6, local_ba_min_tri_angle=6.0):
        self.local_ba_num_images, self.local_ba_min_tri_angle = local_ba_num_images, local_ba_min_tri_angle


def projection_center(image):
    """Image::ProjectionCenter: -R^T t from the normalised quaternion"""
    q = np.asarray(image.qvec, dtype=np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return -R.T @ np.asarray(image.tvec, dtype=np.float64)


def triangulation_angles(c1, c2, points):
    b2 = float(np.sum((c1 - c2) ** 2))
    out = []
    for X in points:
        r1, r2 = float(np.sum((X - c1) ** 2)), float(np.sum((X - c2) ** 2))
        den = 2.0 * math.sqrt(r1 * r2)
        if den == 0.0:
            out.append(0.0)
            continue
        arg = (r1 + r2 - b2) / den
        ang = abs(math.acos(arg)) if -1.0 <= arg <= 1.0 else float("nan")
        out.append(ang if ang != ang else min(ang, math.pi - ang))
    return out


def percentile_index(n):
    """std::round rounds halves away from zero; Python's round goes to the even neighbour (4 for 4.5, where the reference takes 5: n = 7)"""
    return max(0, min(n - 1, int(math.floor(75.0 / 100 * (n - 1) + 0.5))))


def percentile75(angles):
    ordered = sorted(angles, key=lambda a: (a != a, a))      # NaN above every number
    return ordered[percentile_index(len(ordered))]


def find_local_bundle(rec, options, image_id):
    """-> dict(bundle [image ids in the reference's order], overlap [(image id, count)] sorted, tri_angle [radians, -1 where never asked],
    num_points3D, level (-1: early return), filled, lazy (angles the loop computed), margin)"""
    image = rec.images[image_id]
    assert getattr(image, "registered", True)
    shared, point_ids = {}, []
    for line in image.lines:
        if line.HasPoint3D():
            point_ids.append(line.Point3DId())
            for (iid, _) in rec.points3D[line.Point3DId()].track:
                if iid != image_id:
                    shared[iid] = shared.get(iid, 0) + 1
    n3 = len(point_ids)      # image.NumPoints3D()
    overlap = sorted(shared.items(), key=lambda e: (-e[1], e[0]))
    num_eff = min(options.local_ba_num_images - 1, len(overlap))
    out = dict(overlap=overlap, tri_angle=[-1.0] * len(overlap), num_points3D=n3, level=-1, filled=0, lazy=0, margin=float("inf"))
    if len(overlap) == num_eff:
        out["bundle"] = [e[0] for e in overlap]
        return out
    min_rad = options.local_ba_min_tri_angle * DEG
    thresholds = [(min_rad / d, f * n3) for d, f in SELECTION]
    center = projection_center(image)
    bundle, used, tri = [], [False] * len(overlap), out["tri_angle"]
    for level, (min_angle, min_count) in enumerate(thresholds):
        out["level"] = level
        for i, (iid, count) in enumerate(overlap):
            if float(count) < min_count:
                break
            if used[i]:
                continue
            if tri[i] < 0.0:
                points = [rec.points3D[p].xyz for p in point_ids]      # one entry per line, as :1106-1110
                tri[i] = percentile75(triangulation_angles(center, projection_center(rec.images[iid]), points))
                out["lazy"] += 1
            if min_angle > 0 and tri[i] == tri[i]:
                out["margin"] = min(out["margin"], abs(tri[i] - min_angle) / min_angle)
            if tri[i] >= min_angle:
                bundle.append(iid)
                used[i] = True
                if len(bundle) >= num_eff:
                    break
        if len(bundle) >= num_eff:
            break
    if len(bundle) < num_eff:
        for i, (iid, _) in enumerate(overlap):
            if not used[i]:
                bundle.append(iid)
                used[i] = True
                out["filled"] += 1
                if len(bundle) >= num_eff:
                    break
    out["bundle"] = bundle
    return out
