"""The scene of the incremental-registration tests - TEST INFRASTRUCTURE, shared by the CPU check with the oracles and the GPU test.

8 images on a line of camera centres, 150 points in front of them, each seen by a window of 4-6 consecutive images on EXACT lines (a random
line through the projection of the point).  The correspondence graph joins every two lines of one point, the neighbours of a line in ascending
image order.  Images 0-2 start registered at their true poses with the points that at least two of them see (their tracks hold the lines of images
0-2 only); images 3-7 start with `registered = False`, an identity pose and free lines, and the other points do not exist yet.

`spoil_image`: every line of that image whose point's window starts at image 0 or 1 misses the projection by at least 0.2 (normalised
coordinates).  Those are all the correspondences the image can have before an image after it is registered (a point needs three registered
images to be created), so its first registration finds correspondences and no pose; once a later image has been registered and triangulated, the
points of the windows that start at image 2 exist, and the retry succeeds."""
import numpy as np

from privacy_preserving_sfm_amd import synthetic
from privacy_preserving_sfm_amd.bundle_adjustment import Camera, FeatureLine, Image, Point3D, Reconstruction
from privacy_preserving_sfm_amd.incremental_triangulator import CorrespondenceGraph

NUM_IMAGES, NUM_POINTS, NUM_START = 8, 150, 3
MIN_NUM_INLIERS = 15


def make_world(seed=0, spoil_image=None):
    """-> (rec, graph, info): info["poses"] [8, 7] the true poses, info["windows"] [(first image, length)] per point"""
    rng = np.random.default_rng(seed)
    rec, graph = Reconstruction(), CorrespondenceGraph()
    rec.cameras[0] = Camera(0, 2, np.array([1000.0, 640.0, 480.0, 0.0]), width=1280, height=960)
    poses = np.zeros((NUM_IMAGES, 7))
    for c in range(NUM_IMAGES):
        centre = np.array([-2.1 + 0.6 * c, 0.15 * (-1) ** c, 0.05 * c])
        q = np.concatenate([[1.0], rng.normal(0, 0.02, 3)])
        q /= np.linalg.norm(q)
        poses[c, :4], poses[c, 4:] = q, -synthetic.quat_to_rot(q) @ centre
        start = c < NUM_START
        rec.images[c] = Image(c, 0, q if start else np.array([1.0, 0, 0, 0]), poses[c, 4:] if start else np.zeros(3))
        rec.images[c].registered = start

    def line(c, X, miss):
        Xc = synthetic.quat_to_rot(poses[c, :4]) @ X + poses[c, 4:]
        assert Xc[2] > 1.0
        x = np.array([Xc[0] / Xc[2], Xc[1] / Xc[2], 1.0])
        while True:
            l = rng.normal(size=3) if miss else np.cross(x, rng.uniform(-1, 1, 3))
            l /= np.linalg.norm(l[:2])
            if not miss or abs(l @ x) >= 0.2:
                return l

    windows = []
    for p in range(NUM_POINTS):
        X = np.array([rng.uniform(-2.0, 2.0), rng.uniform(-1.5, 1.5), rng.uniform(5.0, 9.0)])
        length = int(rng.integers(4, 7))
        first = int(rng.integers(0, NUM_IMAGES - length + 1))
        windows.append((first, length))
        els = []
        for c in range(first, first + length):
            rec.images[c].lines.append(FeatureLine(line(c, X, spoil_image == c and first <= 1)))
            els.append((c, len(rec.images[c].lines) - 1))
        for a in els:
            for b in els:
                if a != b:
                    graph.AddCorrespondence(a[0], a[1], b[0], b[1])
        track = [el for el in els if el[0] < NUM_START]
        if len(track) >= 2:
            rec.points3D[p] = Point3D(X, track)
            for (c, idx) in track:
                rec.images[c].lines[idx].point3D_id = p
    return rec, graph, dict(poses=poses, windows=windows)


def tracks_of(rec):
    """{point id: its track} and the point of every line: what two runs must agree on"""
    return ({p: list(pt.track) for p, pt in rec.points3D.items()},
            {(i, idx): l.Point3DId() for i, im in rec.images.items() for idx, l in enumerate(im.lines) if l.HasPoint3D()})
