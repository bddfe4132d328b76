"""Scenes of the FindLocalBundle tests - TEST INFRASTRUCTURE, shared by the CPU test of the reference, the host replay test and the GPU test.

Flat poses: the query camera (image 0) at the origin, identity rotations, the points at depth about 10 in front of it, camera j at
(depth * tan(angle_j), 0, 0) - so its triangulation angle against the query camera is angle_j for a point on the axis and within half a percent
of it for the others - and it sees the first round(share_j * N) points.  Every scene carries its expectation, WORKED OUT BY HAND from
src/sfm/incremental_mapper.cc:993-1160 (the thresholds are (6, 4, 3, 2.4, 2, 1.5, 1.2, 1) degrees at local_ba_min_tri_angle = 6 with
(0.6, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.1) * N shared observations): `bundle` (image ids in order), `level`, `filled`, `lazy` (angles the loop
computes) and `num_points3D`."""
import math

import numpy as np

from privacy_preserving_sfm_amd.bundle_adjustment import Camera, FeatureLine, Image, Point3D, Reconstruction
from privacy_preserving_sfm_amd.incremental_triangulator import CorrespondenceGraph

DEPTH = 10.0


class FlatWorld:
    """image i at centers[i] with the identity rotation; add_point builds exact observations (a random line through the projection)"""

    def __init__(self, centers, seed=0):
        self.rng = np.random.default_rng(seed)
        self.rec, self.graph = Reconstruction(), CorrespondenceGraph()
        self.rec.cameras[0] = Camera(0, 2, np.array([1000.0, 640.0, 480.0, 0.0]), width=1280, height=960)
        self.centers = [np.asarray(c, dtype=np.float64) for c in centers]
        for i, c in enumerate(self.centers):
            self.rec.images[i] = Image(i, 0, np.array([1.0, 0.0, 0.0, 0.0]), -c)

    def add_line(self, image, X, point_id):
        Xc = np.asarray(X, dtype=np.float64) - self.centers[image]
        if abs(Xc[2]) > 1e-9:
            l = np.cross(np.array([Xc[0] / Xc[2], Xc[1] / Xc[2], 1.0]), self.rng.uniform(-1, 1, 3))
            l /= np.linalg.norm(l[:2])
        else:      # a point in the camera's own plane has no projection: any normalised line (FindLocalBundle reads none)
            l = np.array([1.0, 0.0, 0.0])
        self.rec.images[image].lines.append(FeatureLine(l, False, point_id))
        self.rec.points3D[point_id].track.append((image, len(self.rec.images[image].lines) - 1))

    def add_point(self, point_id, X, images):
        self.rec.points3D[point_id] = Point3D(X)
        for i in images:
            self.add_line(i, X, point_id)


def layout(angles_deg, shares, N, depths=None, same_place=0, along_y=(), seed=0):
    """-> FlatWorld with 1 + len(angles_deg) images and points 0..N-1: the first `same_place` of them at exactly one position; the images of
    `along_y` are offset along y instead of x"""
    offsets = [DEPTH * math.tan(math.radians(a)) for a in angles_deg]
    w = FlatWorld([(0.0, 0.0, 0.0)] + [(0.0, d, 0.0) if j + 1 in along_y else (d, 0.0, 0.0) for j, d in enumerate(offsets)], seed=seed)
    rng = np.random.default_rng(seed + 77)
    seen = [int(math.floor(s * N + 0.5)) for s in shares]
    for p in range(N):
        z = DEPTH + rng.uniform(-0.05, 0.05) if depths is None else depths[p]
        X = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), z])
        if p < same_place:
            X = np.array([0.05, -0.1, DEPTH])
        w.add_point(p, X, [0] + [j + 1 for j in range(len(angles_deg)) if p < seen[j]])
    return w


def _want(num_images, bundle, level, filled, lazy, num_points3D, min_tri_angle=6.0, image=0):
    return dict(image=image, options=dict(local_ba_num_images=num_images, local_ba_min_tri_angle=min_tri_angle), bundle=bundle, level=level,
                filled=filled, lazy=lazy, num_points3D=num_points3D)


RELAX = ((0.5, 1.1, 2.2, 5.0, 8.0, 3.2, 0.8), (0.95, 0.9, 0.85, 0.7, 0.65, 0.45, 0.3))
FILL = ((0.3, 0.4, 0.5, 7.0, 0.6, 0.2), (0.95, 0.9, 0.85, 0.8, 0.5, 0.3))
STRICT = ((7.0, 0.5, 9.0, 6.5, 0.4), (0.9, 0.85, 0.8, 0.7, 0.65))


def relax():
    """counts 38 36 34 28 26 18 12 of N = 40, three images wanted.  Level 0 (6 deg, 24): images 1..5 are asked, image 5 (8 deg) passes; level 1 (4 deg):
    image 4 (5 deg); level 2 (3 deg, 20): nobody (2.2 < 3); level 3 (2.4 deg, 16): image 6 (count 18) is asked for the first time and passes with 3.2 deg.
    Image 7 is never asked.  The bundle is NOT the top of the overlap list (1, 2, 3)."""
    return layout(*RELAX, N=40), _want(4, [5, 4, 6], 3, 0, 6, 40)


def fill():
    """counts 38 36 34 32 20 12, four images wanted.  Only image 4 (7 deg) ever passes; by level 5 (0.2 * 40 = 8) all six have been asked, the smallest
    threshold is 1 deg at level 7 and the rest stay below it: the fill-up takes the three most overlapping unused images."""
    return layout(*FILL, N=40), _want(5, [4, 1, 2, 3], 7, 3, 6, 40)


def strict(N=40):
    """two images wanted: level 0 takes image 1 (7 deg), skips image 2 (0.5 deg) and takes image 3 (9 deg); images 4 and 5 are never asked"""
    return layout(*STRICT, N=N), _want(3, [1, 3], 0, 0, 3, N)


def empty_image():
    """N = 0: image 0 has lines but none has a point; the other images share points among themselves"""
    w = layout(*STRICT, N=10)
    for idx in range(len(w.rec.images[0].lines)):
        w.rec.DeleteObservation(0, idx)
    return w, _want(3, [], -1, 0, 0, 0)


def one_point():
    """N = 1 (k = 0): every image shares the one point, the tie rule orders them 1 2 3 4 5, and 0.6 * 1 lets all of them through"""
    return strict(1)


def seven_points():
    """N = 7: counts 6 6 6 5 5 (ties by index), k = round(4.5) = 5"""
    return strict(7)


def rounding():
    """N = 7, five points at depth 10 and two at depth 5: image 1 (all seven points, 4 deg on the axis at depth 10) has the sorted angles
    4 4 4 4 4 7.9 7.9 deg - index std::round(0.75 * 6) = 5 gives 7.9 deg and it passes level 0, index 4 (banker's rounding) would give 4 deg and fail it.
    Image 2 (9 deg, six points) passes next; with the wrong index the bundle would be (2, 3)."""
    return layout((4.0, 9.0, 8.0), (1.0, 0.86, 0.72), N=7, depths=[10.0] * 5 + [5.0] * 2), _want(3, [1, 2], 0, 0, 2, 7)


def wave_64():
    return strict(64)


def wave_65():
    return strict(65)


def three_hundred():
    """more points than a workgroup of K12b has threads"""
    return strict(300)


def long_track():
    """point 0 gets 13 more lines in each of the images 1..5: its track has 1 + 5 + 65 = 71 elements (more than one wavefront of lanes), the counts
    grow by 13 each (49 47 45 41 39), the decisions stay those of `strict`"""
    w, want = strict(40)
    for i in range(1, 6):
        for _ in range(13):
            w.add_line(i, w.rec.points3D[0].xyz, 0)
    assert len(w.rec.points3D[0].track) == 71
    return w, want


def two_lines_one_point():
    """point 0 has a second line in the query image: NumPoints3D is 41, the track is walked twice (images 1..5 count it twice) and the point appears
    twice among the 41 positions of the percentile"""
    w, want = strict(40)
    w.add_line(0, w.rec.points3D[0].xyz, 0)
    return w, dict(want, num_points3D=41)


def equal_counts():
    """three images with 32 shared points each and 7, 9, 8 deg, two wanted: the tie rule orders them 1 2 3, level 0 takes 1 and 2"""
    return layout((7.0, 9.0, 8.0), (0.8, 0.8, 0.8), N=40), _want(3, [1, 2], 0, 0, 2, 40)


def early_return():
    """two overlapping images, two wanted: the list is copied (by count: image 2 first) and no angle is asked for, however small it is"""
    return layout((0.1, 0.2), (0.5, 0.9), N=40), _want(3, [2, 1], -1, 0, 0, 40)


def point_at_a_centre():
    """N = 8 and a ninth point exactly on the projection centre of image 2 (which is offset along y here, so that the point is not in line with the
    other centres): seen by the query image and image 1, its angle against image 2 is 0 by the rule for a vanishing denominator
    (triangulation.cc:103-106).  Decisions as `strict`."""
    w, want = layout(*STRICT, N=8, along_y=(2,)), _want(3, [1, 3], 0, 0, 3, 9)
    w.add_point(8, w.centers[2].copy(), [0, 1])
    return w, want


def equal_angles():
    """30 of the 40 points lie at one place: 30 equal bit patterns in the radix select"""
    return layout(*STRICT, N=40, same_place=30), _want(3, [1, 3], 0, 0, 3, 40)


def count_on_the_threshold():
    """one image wanted; image 2 shares exactly 0.6 * 40 = 24 points: `24 < 24.0` is false, so level 0 asks for it (after image 1, 0.5 deg) and takes it.
    Were it left out, image 2 would be taken at level 2 (0.5 * 40 = 20) only."""
    return layout((0.5, 7.0, 9.0), (0.9, 0.6, 0.5), N=40), _want(2, [2], 0, 0, 2, 40)


SCENES = [relax, fill, strict, empty_image, one_point, seven_points, rounding, wave_64, wave_65, three_hundred, long_track, two_lines_one_point,
          equal_counts, early_return, point_at_a_centre, equal_angles, count_on_the_threshold]
