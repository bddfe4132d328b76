"""Scenes of the TriangulateImage / CompleteImage tests - TEST INFRASTRUCTURE, shared by the CPU tests of the oracle, the host replay test and the GPU test.

Synthetic: synthetic.make_completion_scene with exact poses (noise-free inlier lines), its false edges as gross outliers, every line of the chosen
image free, and the POINT of every second such line removed altogether (all its lines free: work for Create; the others keep their point: work for
Continue); every seventh line is flagged aligned.  Hand-built: _World below, the cameras of a make_ba_scene ring at their true poses."""
import numpy as np

from privacy_preserving_sfm_amd import synthetic
from privacy_preserving_sfm_amd.bundle_adjustment import Camera, FeatureLine, Image, Point3D, Reconstruction
from privacy_preserving_sfm_amd.incremental_triangulator import CorrespondenceGraph, reconstruction_from_completion_scene

# seeds and images picked on the CPU with the oracle alone: margin > 1e-6, no RANSAC with an arbitrary winner, creates and continues at both transitivities with a
# pp_tracks_complete and a pp_tracks_merge (which merges) in between
SYNTHETIC = [dict(cfg=(8, 60, 6), seed=6, image=3), dict(cfg=(12, 120, 8), seed=1, image=5)]
# the hand-built scenes are exact, so their angular thresholds can be tight: at the default 2 degrees a random line through one place passes another
# place's ray often enough to blur the groups
TIGHT = dict(create_max_angle_error=0.05, continue_max_angle_error=0.05)


def synthetic_world(cfg, seed, image, false_edges=0.02, **scene_kw):
    sc = synthetic.make_completion_scene(*cfg, seed=seed, noise_point=1e-4, noise_t=0.0, noise_q=0.0, split=0.0, false_edges=false_edges, **scene_kw)
    lp = sc["line_point"].copy()
    own = np.flatnonzero(sc["line_image"] == image)
    removed = set(int(sc["line_true_point"][l]) for l in own[::2])
    for l in range(len(lp)):
        if lp[l] in removed or sc["line_image"][l] == image:
            lp[l] = -1
    # the removed points leave no hole in the ids: the kept ones are renumbered in order
    keep = [p for p in range(sc["points"].shape[0]) if p not in removed and (lp == p).any()]
    renum = {p: k for k, p in enumerate(keep)}
    sc["points"] = sc["points"][keep]
    sc["line_point"] = np.array([renum.get(int(p), -1) for p in lp], dtype=np.int32)
    rec, graph = reconstruction_from_completion_scene(sc)
    k = 0
    for iid in sorted(rec.images):
        for fl in rec.images[iid].lines:
            fl._aligned = (k % 7 == 3)
            k += 1
    return rec, graph


class World:
    """cameras of a make_ba_scene ring at their true poses; add_point / add_line build exact observations (a random line through the projection)"""

    def __init__(self, num_cams=12, seed=0):
        base = synthetic.make_ba_scene(num_cams, 10, 4, seed=seed)
        self.rng = np.random.default_rng(seed + 1000)
        self.rec, self.graph = Reconstruction(), CorrespondenceGraph()
        self.rec.cameras[0] = Camera(0, 2, base["intr"][0, :4], width=1280, height=960)
        self.poses = base["gt_poses"]
        for c in range(num_cams):
            self.rec.images[c] = Image(c, 0, self.poses[c, :4], self.poses[c, 4:])

    def add_line(self, c, X, point_id=-1, aligned=False):
        R = synthetic.quat_to_rot(self.poses[c, :4])
        Xc = R @ np.asarray(X) + self.poses[c, 4:]
        l = np.cross(np.array([Xc[0] / Xc[2], Xc[1] / Xc[2], 1.0]), self.rng.uniform(-1, 1, 3))
        l /= np.linalg.norm(l[:2])
        self.rec.images[c].lines.append(FeatureLine(l, aligned, point_id))
        el = (c, len(self.rec.images[c].lines) - 1)
        if point_id >= 0:
            self.rec.points3D[point_id].track.append(el)
        return el

    def add_point(self, pid, X, cams, at=None):
        self.rec.points3D[pid] = Point3D(X if at is None else at)
        return [self.add_line(c, X, pid) for c in cams]

    def link(self, a, b):
        self.graph.AddCorrespondence(a[0], a[1], b[0], b[1]); self.graph.AddCorrespondence(b[0], b[1], a[0], a[1])

    def arc(self, a, b):
        self.graph.AddCorrespondence(a[0], a[1], b[0], b[1])


X, Y, Z = np.array([0.1, -0.2, 0.3]), np.array([-0.4, 0.3, 0.1]), np.array([0.3, 0.25, -0.2])


def shared_neighbour():
    """lines r0 and r1 of image 0 see X; both reach the free lines of X in images 1..3: r0 creates the point from all of them and r1, r1's speculation
    (the same point again) is stale and must be redone - it then finds its neighbours triangulated, is itself taken, and does nothing"""
    w = World()
    r0, r1 = w.add_line(0, X), w.add_line(0, X)
    n = [w.add_line(c, X) for c in (1, 2, 3)]
    for f in n:
        w.link(r0, f); w.link(r1, f)
    w.link(r0, r1)
    return w, dict(image=0, ops="t", events=[(0, n[0]), (0, n[1]), (0, n[2]), (0, r1), (0, r0)], num_changed=5, redone=1)


def continue_then_create():
    """r sees X; its neighbours: a line of point 0 (at X: the continue), then four free lines of Y: the create set is those four and NOT r"""
    w = World()
    a = w.add_point(0, X, [1, 2, 3, 4])
    r = w.add_line(0, X)
    f = [w.add_line(c, Y) for c in (5, 6, 7, 8)]
    w.link(r, a[0])
    for g in f:
        w.link(r, g)
    return w, dict(image=0, ops="t", events=[(0, r)] + [(1, g) for g in f], num_changed=5, redone=0)


def line_with_point_still_creates():
    w = World()
    a = w.add_point(0, X, [0, 1, 2, 3])      # a[0] is line 0 of image 0 and has its point
    f = [w.add_line(c, Y) for c in (5, 6, 7, 8)]
    for g in f:
        w.link(a[0], g)
    return w, dict(image=0, ops="t", events=[(1, g) for g in f], num_changed=4, redone=0)


def only_aligned_lines():
    w = World()
    r = w.add_line(0, X, aligned=True)
    for c in (1, 2, 3, 4):
        w.link(r, w.add_line(c, X, aligned=True))
    return w, dict(image=0, ops="t", events=[], num_changed=0, redone=0)


def create_recursion():
    """one closure holds four lines of X and four of Y (and r, a line of X): two points from one Create"""
    w = World()
    r = w.add_line(0, X)
    fx = [w.add_line(c, X) for c in (1, 2, 3, 4)]
    fy = [w.add_line(c, Y) for c in (5, 6, 7, 8)]
    for g, k in zip(fx, fy):
        w.link(r, g); w.link(r, k)
    order = [v for pair in zip(fx, fy) for v in pair]
    return w, dict(image=0, ops="t", events=[(0, g) for g in order if g in fx] + [(0, r)] + [(1, g) for g in fy], num_changed=9, redone=0)


def long_closure():
    """r has 70 free neighbours on X (more than one wavefront of lanes) and, in their middle, a line of point 0 which lies elsewhere: no continue, and one
    point from the 70 and r"""
    w = World()
    a = w.add_point(0, Z, [1, 2, 3, 4])
    r = w.add_line(0, X)
    f = [w.add_line(1 + (i % 11), X) for i in range(70)]
    for g in f[:35]:
        w.link(r, g)
    w.link(r, a[0])
    for g in f[35:]:
        w.link(r, g)
    return w, dict(image=0, ops="t", events=[(1, g) for g in f] + [(1, r)], num_changed=71, redone=0)


def swap_order():
    """transitivity 2: r -> (n1, n2), n1 -> m1, n2 -> m2: collected [r, n1, n2, m1, m2], returned [m2, n1, n2, m1] - the track of the new point shows it"""
    w = World()
    r = w.add_line(0, X)
    n1, n2, m1, m2 = (w.add_line(c, X) for c in (1, 2, 3, 4))
    w.arc(r, n1); w.arc(r, n2); w.arc(n1, m1); w.arc(n2, m2)
    return w, dict(image=0, ops="t", transitivity=2, events=[(0, m2), (0, n1), (0, n2), (0, m1), (0, r)], num_changed=5, redone=0)


def two_view_rule():
    """CompleteImage: r0 and its only neighbour see each other alone (a two-view observation: skipped); r1 has three neighbours and gets a point; r2 has
    point 0, whose completion takes the free line behind it"""
    w = World()
    a = w.add_point(0, Z, [1, 2, 3, 4])
    r0 = w.add_line(0, X); p0 = w.add_line(1, X); w.link(r0, p0)
    r1 = w.add_line(0, Y)
    f = [w.add_line(c, Y) for c in (5, 6, 7)]
    for g in f:
        w.link(r1, g)
    r2 = w.add_line(0, Z, 0)
    b = w.add_line(6, Z); w.link(r2, b)
    return w, dict(image=0, ops="c", events=[(1, g) for g in f] + [(1, r1), (0, b)], num_changed=5, redone=0)


def unregistered_image():
    w, want = shared_neighbour()
    w.rec.images[0].registered = False
    return w, dict(image=0, ops="tc", events=[], num_changed=0, redone=0)


def skipped_camera():
    w, want = shared_neighbour()
    w.rec.cameras[1] = Camera(1, 2, np.array([1e6, 640.0, 480.0, 0.0]), width=1280, height=960)      # a bogus focal length
    w.rec.images[0].camera_id = 1
    return w, dict(image=0, ops="tc", events=[], num_changed=0, redone=0)


HAND_BUILT = [shared_neighbour, continue_then_create, line_with_point_still_creates, only_aligned_lines, create_recursion, long_closure, swap_order,
              two_view_rule, unregistered_image, skipped_camera]
