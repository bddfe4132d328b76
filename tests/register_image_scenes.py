"""Scenes of the FindNextImages / RegisterNextImage tests - TEST INFRASTRUCTURE, shared by the CPU test of the transcription, the host replay test and
the GPU tests.

SEARCH scenes (`World`): image 0 and 1 are registered hosts with a sound camera, image 2 is an UNREGISTERED host, image 3 a registered host whose
camera is flagged (a focal length of 50 px on a 1280 px image: ratio 0.039 < min_focal_length_ratio 0.1).  A query image is unregistered; each of its
lines gets its neighbour list spelled out.  Every scene carries its expectation, WORKED OUT BY HAND from src/sfm/incremental_mapper.cc:601-647:
`tri_corrs` per query image ((line_idx, point id) in order), `visible` and `observed` per query image.  The geometry of a search scene means
nothing: no number is computed from it.

COMMIT scenes: a correspondence list with an inlier mask, and the AddObservation calls of :746-757 by hand.
RANKING scenes: unregistered images with chosen (visible, observed) counts, trial counts and filtered flags, and the list FindNextImages returns.
POSE scenes (`pose_world`): three registered images and a query image at a known pose; every correspondence on an exact line through the projection
of its point, the planted outliers on lines that miss it by at least 0.2 in normalised coordinates (the RANSAC threshold is 0.012)."""
import numpy as np

from privacy_preserving_sfm_amd import synthetic
from privacy_preserving_sfm_amd.bundle_adjustment import Camera, FeatureLine, Image, Point3D, Reconstruction
from privacy_preserving_sfm_amd.incremental_triangulator import CorrespondenceGraph

HOST_A, HOST_B, HOST_UNREG, HOST_FLAGGED = 0, 1, 2, 3
GOOD_CAMERA = np.array([1000.0, 640.0, 480.0, 0.0])
BOGUS_CAMERA = np.array([50.0, 640.0, 480.0, 0.0])
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0])


class World:
    def __init__(self, seed=0):
        self.rng = np.random.default_rng(seed)
        self.rec, self.graph = Reconstruction(), CorrespondenceGraph()
        self.rec.cameras[0] = Camera(0, 2, GOOD_CAMERA, width=1280, height=960)
        self.rec.cameras[1] = Camera(1, 2, BOGUS_CAMERA, width=1280, height=960)
        for iid, cam, reg in ((HOST_A, 0, True), (HOST_B, 0, True), (HOST_UNREG, 0, False), (HOST_FLAGGED, 1, True)):
            self.rec.images[iid] = Image(iid, cam, IDENTITY, np.array([0.1 * iid, 0.0, 0.0]))
            self.rec.images[iid].registered = reg

    def _line(self):
        l = self.rng.normal(size=3)
        return l / np.linalg.norm(l[:2])

    def new_point(self):
        pid = len(self.rec.points3D)
        self.rec.points3D[pid] = Point3D(np.array([self.rng.uniform(-1, 1), self.rng.uniform(-1, 1), self.rng.uniform(4, 8)]))
        return pid

    def host_line(self, image, point="new"):
        """a line of a host image: with a new point, with point id `point`, or (None) without one -> (image, line_idx)"""
        pid = self.new_point() if point == "new" else (-1 if point is None else point)
        self.rec.images[image].lines.append(FeatureLine(self._line(), False, pid))
        el = (image, len(self.rec.images[image].lines) - 1)
        if pid >= 0:
            self.rec.points3D[pid].track.append(el)
        return el

    def point_of(self, el):
        return self.rec.images[el[0]].lines[el[1]].Point3DId()

    def query_image(self, camera=0):
        iid = len(self.rec.images)
        self.rec.images[iid] = Image(iid, camera, IDENTITY, np.array([0.0, 0.1 * iid, 0.0]))
        self.rec.images[iid].registered = False
        return iid

    def query_line(self, q, neighbours, aligned=False):
        """a line of query image q whose correspondence list is `neighbours`, in this order (the graph is symmetric) -> line_idx"""
        self.rec.images[q].lines.append(FeatureLine(self._line(), aligned))
        idx = len(self.rec.images[q].lines) - 1
        for el in neighbours:
            self.graph.AddCorrespondence(q, idx, el[0], el[1])
            self.graph.AddCorrespondence(el[0], el[1], q, idx)
        return idx


def _want(q, tri_corrs, visible, observed):
    return dict(image=q, tri_corrs=tri_corrs, visible=visible, observed=observed)


def dedup():
    """(a) line 0 reaches point A through a line of host A and again through a line of host B, then point B: (0, A), (0, B).  Line 1 reaches B alone:
    the set of seen points is per line, so (1, B) stays"""
    w = World()
    a1 = w.host_line(HOST_A); A = w.point_of(a1)
    a2 = w.host_line(HOST_B, A)
    b1 = w.host_line(HOST_A); B = w.point_of(b1)
    q = w.query_image()
    w.query_line(q, [a1, a2, b1])
    w.query_line(q, [b1])
    return w, [_want(q, [(0, A), (0, B), (1, B)], 2, 2)]


def dedup_across_chunks():
    """(b) 72 neighbours: entry 0 and entry 70 have point A (70 apart: different 64-lane chunks), entry 1 and entry 65 point B, the rest distinct"""
    w = World()
    first = w.host_line(HOST_A); A = w.point_of(first)
    second = w.host_line(HOST_B); B = w.point_of(second)
    n = [first, second] + [w.host_line(HOST_A if i % 2 else HOST_B) for i in range(2, 72)]
    n[70] = w.host_line(HOST_B, A)
    n[65] = w.host_line(HOST_A, B)
    q = w.query_image()
    w.query_line(q, n)
    return w, [_want(q, [(0, w.point_of(el)) for i, el in enumerate(n) if i not in (65, 70)], 1, 1)]


def list_lengths():
    """(c) neighbour lists of 0, 1, 64, 65, 130, 256, 257 and 300 entries, all points distinct (256 / 257: the on-chip list of accepted points is full /
    the list lives in global memory); in the 300 list entry 290 repeats the point of entry 3 and entry 299 that of entry 64"""
    w = World()
    q = w.query_image()
    corrs = []
    for line_idx, length in enumerate((0, 1, 64, 65, 130, 256, 257, 300)):
        n = [w.host_line(HOST_A if i % 3 else HOST_B) for i in range(length)]
        skip = ()
        if length == 300:
            n[290] = w.host_line(HOST_A, w.point_of(n[3]))
            n[299] = w.host_line(HOST_B, w.point_of(n[64]))
            skip = (290, 299)
        w.query_line(q, n)
        corrs += [(line_idx, w.point_of(el)) for i, el in enumerate(n) if i not in skip]
    return w, [_want(q, corrs, 7, 7)]


def filtered_neighbours():
    """(d) line 0: a neighbour in the unregistered host (it HAS a point: the registration test comes first), one behind the flagged camera, one
    without a point, then a good one with point A.  Line 1: the flagged-camera neighbour has point B first, the good host reaches B after it: the
    skipped neighbour does not enter the set of seen points, so (1, B) is kept.  Line 2: only a neighbour without a point: observed, not visible"""
    w = World()
    u = w.host_line(HOST_UNREG); f = w.host_line(HOST_FLAGGED); e = w.host_line(HOST_A, None); a = w.host_line(HOST_A)
    fb = w.host_line(HOST_FLAGGED); B = w.point_of(fb); gb = w.host_line(HOST_B, B)
    q = w.query_image()
    w.query_line(q, [u, f, e, a])
    w.query_line(q, [fb, gb])
    w.query_line(q, [w.host_line(HOST_B, None)])
    return w, [_want(q, [(0, w.point_of(a)), (1, B)], 2, 3)]


def visible_but_unusable():
    """(e) eight lines, each with one neighbour behind the flagged camera: NumVisiblePoints3D is 8, the search returns nothing (-> :653 at
    abs_pose_min_num_inliers <= 8)"""
    w = World()
    q = w.query_image()
    for _ in range(8):
        w.query_line(q, [w.host_line(HOST_FLAGGED)])
    return w, [_want(q, [], 8, 8)]


def image_sizes():
    """(f) query images with 1, 63, 64, 65 and 1100 lines (the scan's workgroup has 1024 threads: two lines per thread), every third line with two
    correspondences, every seventh with none that counts"""
    w = World()
    wants = []
    for num_lines in (1, 63, 64, 65, 1100):
        q = w.query_image()
        corrs, visible = [], 0
        for idx in range(num_lines):
            if idx % 7 == 6:
                w.query_line(q, [w.host_line(HOST_A, None)])
                continue
            n = [w.host_line(HOST_A)] + ([w.host_line(HOST_B)] if idx % 3 == 0 else [])
            w.query_line(q, n)
            corrs += [(idx, w.point_of(el)) for el in n]
            visible += 1
        wants.append(_want(q, corrs, visible, num_lines))
    return w, wants


SEARCH_SCENES = [dedup, dedup_across_chunks, list_lengths, filtered_neighbours, visible_but_unusable, image_sizes]


# ---- the commit rule ------------------------------------------------------------------------------------------------------------------------------

def commit_first_inlier_wins():
    """(g) line 0 has the correspondences (0, A) and (0, B): with A an outlier and B an inlier the line joins B; line 1 has (1, C), (1, D), both
    inliers: it joins C and D is skipped because the line has a point by then"""
    w = World()
    a, b, c, d = (w.host_line(HOST_A) for _ in range(4))
    A, B, Cp, D = (w.point_of(el) for el in (a, b, c, d))
    q = w.query_image()
    w.query_line(q, [a, b])
    w.query_line(q, [c, d])
    return w, dict(image=q, tri_corrs=[(0, A), (0, B), (1, Cp), (1, D)], inlier_mask=[0, 1, 1, 1], events=[(B, (q, 0)), (Cp, (q, 1))])


def commit_two_lines_one_point():
    """(h) lines 0 and 1 of the image both reach point A (through different host lines): both join it, in list order; line 2's only
    correspondence is an outlier and it stays free"""
    w = World()
    a1 = w.host_line(HOST_A); A = w.point_of(a1)
    a2 = w.host_line(HOST_B, A)
    b = w.host_line(HOST_A); B = w.point_of(b)
    q = w.query_image()
    w.query_line(q, [a1])
    w.query_line(q, [a2])
    w.query_line(q, [b])
    return w, dict(image=q, tri_corrs=[(0, A), (1, A), (2, B)], inlier_mask=[1, 1, 0], events=[(A, (q, 0)), (A, (q, 1))])


COMMIT_SCENES = [commit_first_inlier_wins, commit_two_lines_one_point]


# ---- the ranking ----------------------------------------------------------------------------------------------------------------------------------

def ranking():
    """(i) abs_pose_min_num_inliers = 3, max_reg_trials = 3.  Unregistered images (visible / observed):
         4: 6 / 12    5: 6 / 6    6: 8 / 32    7: 6 / 6    8: 5 / 5 with 3 trials (= max_reg_trials: out)    9: 7 / 7 filtered (second bucket)
        10: 2 / 9 (one visible point short of the gate: out)    11: 4 / 4 with 1 trial (second bucket)
    NUM:   first bucket 6 (8), then 4, 5, 7 (6 each: by id); second bucket 9 (7), 11 (4)              -> 6 4 5 7 9 11
    RATIO: first bucket 5, 7 (1.0 each: by id), 4 (0.5), 6 (0.25); second bucket 9, 11 (1.0 each)    -> 5 7 4 6 9 11
    The unregistered host (image 2) has no line here: visible 0, out."""
    w = World()
    spec = [(6, 12), (6, 6), (8, 32), (6, 6), (5, 5), (7, 7), (2, 9), (4, 4)]
    ids = []
    for visible, observed in spec:
        q = w.query_image()
        ids.append(q)
        for idx in range(observed):
            w.query_line(q, [w.host_line(HOST_A if idx % 2 else HOST_B, "new" if idx < visible else None)])
    assert ids == [4, 5, 6, 7, 8, 9, 10, 11]
    return w, dict(options=dict(abs_pose_min_num_inliers=3, max_reg_trials=3), num_reg_trials={8: 3, 11: 1}, filtered=[9],
                   num=[6, 4, 5, 7, 9, 11], ratio=[5, 7, 4, 6, 9, 11],
                   visible={q: s[0] for q, s in zip(ids, spec)}, observed={q: s[1] for q, s in zip(ids, spec)})


# ---- pose scenes ----------------------------------------------------------------------------------------------------------------------------------

QUERY_POSE = np.array([0.9990482215818578, 0.02, -0.03, 0.025, 0.3, -0.2, 0.4])      # (qvec, tvec); the quaternion is normalised in pose_world


def _exact_line(rng, pose, X):
    R = synthetic.quat_to_rot(pose[:4])
    Xc = R @ X + pose[4:]
    assert Xc[2] > 1.0
    l = np.cross(np.array([Xc[0] / Xc[2], Xc[1] / Xc[2], 1.0]), rng.uniform(-1, 1, 3))
    return l / np.linalg.norm(l[:2])


def _missing_line(rng, pose, X):
    """a line at distance >= 0.2 from the projection of X"""
    R = synthetic.quat_to_rot(pose[:4])
    Xc = R @ X + pose[4:]
    x = np.array([Xc[0] / Xc[2], Xc[1] / Xc[2], 1.0])
    while True:
        l = rng.normal(size=3)
        l /= np.linalg.norm(l[:2])
        if abs(l @ x) >= 0.2:
            return l


def pose_world(n=50, outliers=10, aligned=0, extra_unusable=0, seed=0, models=(2, 2, 2)):
    """-> (rec, graph, info).  Images 0, 1, 2 registered (cameras 0, 1, 2 of `models`), image 3 the query (camera 0) whose TRUE pose is info["pose"].
    n points, each with an exact line in two of the registered images; query line i corresponds to the line of point i in image i % 3 (one
    correspondence per line).  The first `outliers` query lines (spread by a fixed permutation) miss their point; the first `aligned` lines in
    index order are flagged aligned (with ALL of them flagged the minimal solver returns no model for any sample - P6LEstimator::Estimate gives up on six
    aligned lines - and the RANSAC ends without an inlier).  extra_unusable: further query lines whose only neighbour is in an unregistered image
    (visible, no correspondence)."""
    rng = np.random.default_rng(seed)
    rec, graph = Reconstruction(), CorrespondenceGraph()
    for k, m in enumerate(models):
        rec.cameras[k] = Camera(k, int(m), synthetic.default_intrinsics(int(m))[: synthetic.NUM_PARAMS[int(m)]], width=1280, height=960)
    host_poses = [np.concatenate([IDENTITY, t]) for t in ([0.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0])]
    for c in range(3):
        rec.images[c] = Image(c, c, host_poses[c][:4], host_poses[c][4:])
    pose = QUERY_POSE.copy()
    pose[:4] /= np.linalg.norm(pose[:4])
    rec.images[3] = Image(3, 0, IDENTITY, np.zeros(3))
    rec.images[3].registered = False
    if extra_unusable:
        rec.images[4] = Image(4, 0, IDENTITY, np.array([0.5, 0.5, 0.0]))
        rec.images[4].registered = False
    is_outlier = np.zeros(n, dtype=bool)
    is_outlier[rng.permutation(n)[:outliers]] = True
    for i in range(n):
        X = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(4.0, 8.0)])
        rec.points3D[i] = Point3D(X)
        els = []
        for c in (i % 3, (i + 1) % 3):
            rec.images[c].lines.append(FeatureLine(_exact_line(rng, host_poses[c], X), False, i))
            els.append((c, len(rec.images[c].lines) - 1))
            rec.points3D[i].track.append(els[-1])
        l = _missing_line(rng, pose, X) if is_outlier[i] else _exact_line(rng, pose, X)
        rec.images[3].lines.append(FeatureLine(l, i < aligned))
        graph.AddCorrespondence(3, i, els[0][0], els[0][1]); graph.AddCorrespondence(els[0][0], els[0][1], 3, i)
    for j in range(extra_unusable):
        X = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(4.0, 8.0)])
        pid = n + j
        rec.points3D[pid] = Point3D(X)
        rec.images[4].lines.append(FeatureLine(_exact_line(rng, np.concatenate([IDENTITY, [0.5, 0.5, 0.0]]), X), False, pid))
        rec.points3D[pid].track.append((4, j))
        rec.images[3].lines.append(FeatureLine(_exact_line(rng, pose, X), False))
        graph.AddCorrespondence(3, n + j, 4, j); graph.AddCorrespondence(4, j, 3, n + j)
    return rec, graph, dict(image=3, pose=pose, inliers=~is_outlier)


# name -> (pose_world arguments, mapper options, the expected failure code (register_image_reference) and what is planted)
POSE_SCENES = {
    "found_50": (dict(n=50, outliers=10, seed=1), dict(abs_pose_min_num_inliers=30), 0),
    "found_40": (dict(n=40, outliers=8, seed=2), dict(abs_pose_min_num_inliers=25), 0),
    "found_60_some_aligned": (dict(n=60, outliers=12, aligned=20, seed=3), dict(abs_pose_min_num_inliers=30), 0),
    "few_visible": (dict(n=20, outliers=0, seed=4), dict(abs_pose_min_num_inliers=21), 1),
    "few_corrs": (dict(n=20, outliers=0, extra_unusable=10, seed=5), dict(abs_pose_min_num_inliers=25), 2),
    "no_inliers": (dict(n=40, outliers=0, aligned=40, seed=6), dict(abs_pose_min_num_inliers=10), 3),
    "mostly_aligned": (dict(n=50, outliers=0, aligned=46, seed=7), dict(abs_pose_min_num_inliers=30), 4),
    "few_inliers": (dict(n=50, outliers=30, seed=8), dict(abs_pose_min_num_inliers=30), 6),
}
