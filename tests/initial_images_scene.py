"""The scene of the RegisterInitialLineImages tests - TEST INFRASTRUCTURE, shared by the CPU check of the scene and the GPU test.

7 UPRIGHT cameras (rotation about y only, so the gravity direction R[:, 1] is (0, 1, 0) in every camera frame) on a line of camera centres, one camera
model as in incremental_registration_scene.py.  Points in front of them, each seen by a window of 4-6 consecutive images (three in ten of them by images
0-3 exactly: FIRST_WINDOW_SHARE) on EXACT lines, inside every image of its window; about half of the points are observed as gravity-aligned lines
normalize(x~ x g), as synthetic.make_init_scene draws them, the others as a random line through the projection.  The correspondence graph joins every two
lines of one point.  ALL images start unregistered at the identity and no point exists: the reconstruction starts from zero.

`few_aligned`: only that many points are observed as aligned lines, so that no image set reaches the 20 aligned tracks the search asks for."""
import numpy as np

from privacy_preserving_sfm_amd.bundle_adjustment import Camera, FeatureLine, Image, Reconstruction
from privacy_preserving_sfm_amd.incremental_triangulator import CorrespondenceGraph

NUM_IMAGES, NUM_POINTS, SEED = 7, 200, 1
FIRST_WINDOW_SHARE = 0.3      # of the points are seen by images 0-3 exactly, the others by a random window: the set (0, 1, 2, 3) leads, and a point seen by
                              # images 3-6 has ONE registered view until image 4 is registered - TriangulateImage has points left to create then
MIN_NUM_INLIERS = 15      # abs_pose_min_num_inliers of the registration that follows the initialisation (incremental_registration_scene.py's)


def rot_y(a):
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def make_world(seed=SEED, num_points=NUM_POINTS, few_aligned=None):
    """-> (rec, graph, info): info["R"] [7, 3, 3] and info["t"] [7, 3] the true poses, info["line_point"] {(image_id, line_idx): point number},
    info["aligned"] [num_points] flags"""
    rng = np.random.default_rng(seed)
    rec, graph = Reconstruction(), CorrespondenceGraph()
    rec.cameras[0] = Camera(0, 2, np.array([1000.0, 640.0, 480.0, 0.0]), width=1280, height=960)
    R, t = np.zeros((NUM_IMAGES, 3, 3)), np.zeros((NUM_IMAGES, 3))
    for c in range(NUM_IMAGES):
        centre = np.array([-1.5 + 0.5 * c, rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)])
        R[c] = rot_y(rng.uniform(-0.15, 0.15))
        t[c] = -R[c] @ centre
        rec.images[c] = Image(c, 0, np.array([1.0, 0, 0, 0]), np.zeros(3), gravity=R[c][:, 1])
        rec.images[c].registered = False
    num_aligned = num_points // 2 if few_aligned is None else few_aligned
    aligned = rng.permutation(num_points) < num_aligned
    line_point = {}
    for p in range(num_points):
        length = int(rng.integers(4, 7))
        first = int(rng.integers(0, NUM_IMAGES - length + 1))
        if rng.random() < FIRST_WINDOW_SHARE:
            first, length = 0, 4
        while True:      # inside every image of the window
            X = np.array([rng.uniform(-2.5, 2.5), rng.uniform(-1.5, 1.5), rng.uniform(3.0, 6.0)])
            Xc = [R[c] @ X + t[c] for c in range(first, first + length)]
            if all(abs(x[0] / x[2]) < 0.6 and abs(x[1] / x[2]) < 0.45 for x in Xc):
                break
        els = []
        for c, x in zip(range(first, first + length), Xc):
            xh = np.array([x[0] / x[2], x[1] / x[2], 1.0])
            l = np.cross(xh, rec.images[c].gravity if aligned[p] else rng.uniform(-1, 1, 3))
            rec.images[c].lines.append(FeatureLine(l / np.linalg.norm(l[:2]), bool(aligned[p])))
            els.append((c, len(rec.images[c].lines) - 1))
            line_point[els[-1]] = p
        for a in els:
            for b in els:
                if a != b:
                    graph.AddCorrespondence(a[0], a[1], b[0], b[1])
    return rec, graph, dict(R=R, t=t, line_point=line_point, aligned=aligned)


def flat_scene(rec, graph, check_images=None, subset=None, **options):
    """the world as a scene of initial_sets_scenes.py / initial_sets_reference.py (image ids 0..C-1 are their own indices); returns (scene, line_ref)"""
    image_ids = sorted(rec.images)
    assert image_ids == list(range(len(image_ids)))
    offset, line_ref = {}, []
    for i in image_ids:
        offset[i] = len(line_ref)
        line_ref.extend((i, idx) for idx in range(len(rec.images[i].lines)))
    opts = dict(min_num_aligned_tracks=20, min_num_random_tracks=20, max_num_sets=10)
    opts.update(options)
    scene = dict(num_images=len(image_ids), line_image=[i for i, _ in line_ref], line_aligned=[int(rec.images[i].lines[idx].IsAligned()) for i, idx in line_ref],
                 corr=[[offset[i2] + x2 for (i2, x2) in graph.FindCorrespondences(i, idx)] for i, idx in line_ref],
                 check_images=image_ids if check_images is None else list(check_images), subset=subset, options=opts)
    return scene, line_ref


def relative_poses(R, t, image_ids):
    """the poses of `image_ids` relative to the first of them, translations scaled by |t_1|: the gauge initialize_reconstruction's result is compared in"""
    R0, t0 = R[image_ids[0]], t[image_ids[0]]
    rel = []
    for i in image_ids:
        Rr = R[i] @ R0.T
        rel.append(np.hstack([Rr, (t[i] - Rr @ t0)[:, None]]))
    rel = np.array(rel)
    rel[:, :, 3] /= np.linalg.norm(rel[1][:, 3])
    return rel
