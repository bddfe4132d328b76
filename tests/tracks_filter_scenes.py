"""Scenes of the tracks-filter tests - TEST INFRASTRUCTURE, shared by the CPU reference test, the host replay test and the GPU test.

A scene is (rec, graph, ops, expect): `ops` a list of tracks_filter_reference.run_op entries run one after the other on ONE reconstruction (one live handle),
`expect` per op the hand-written outcome (None for the synthetic worlds, where the reference alone says what happens): dict(events, num_filtered[, filtered]).
Hand-built: tracks_image_scenes.World - exact lines through the projections, on a ring of 24 images of radius 4 that look at the origin (field of view
about +-32 degrees; image c stands at the angle 15 c degrees, so the images 10..14 alone see a far point on the +x axis, and 23, 0, 1 have (6, 0, 0) behind
them).  Thresholds: 4 px and 1.5 degrees unless an op says otherwise.
Synthetic: tracks_image_scenes.synthetic_world, corrupted as _filter_scene of tests/test_gpu_bundle_adjustment.py corrupts its scene: far points, points
behind cameras, spoiled line offsets, aligned-only tracks.  (A moved point's lines no longer pass through it, so it goes by the track rule, as in that test;
the angle rule on exact lines is the hand-built scenes'.)"""
import numpy as np

from tracks_image_scenes import World, synthetic_world

from privacy_preserving_sfm_amd.bundle_adjustment import Camera

X, Y, Z = np.array([0.1, -0.2, 0.3]), np.array([-0.4, 0.3, 0.1]), np.array([0.3, 0.25, -0.2])
FAR = np.array([300.0, 0.0, 0.0])       # seen by the images 10..14 only, which subtend at most 0.77 degrees there
BEHIND = np.array([6.0, 0.0, 0.0])      # behind the images 23, 0, 1; in front of and inside 9..15


def _point(w, pid, at, cams, bad=(), aligned=(), through=None):
    """point `pid` at `at`; one exact line per image of `cams` (through `through`, default `at`), except in the images of `bad`: a line through a place 0.5
    away, tens of pixels off; the images of `aligned` get their line flagged aligned.  -> the track"""
    through = at if through is None else through
    w.add_point(pid, through, [], at=at)
    return [w.add_line(c, through + (np.array([0.35, -0.3, 0.2]) if c in bad else 0.0), pid, aligned=c in aligned) for c in cams]


def _scene(w, ops, expect):
    return w.rec, w.graph, ops, expect


def aligned_only_track():
    """point 0: five aligned lines and nothing else -> deleted, counted with its length; point 1: one line of five is not aligned -> kept, error set"""
    w = World(24)
    _point(w, 0, X, [0, 4, 8, 12, 16], aligned=[0, 4, 8, 12, 16])
    _point(w, 1, Y, [1, 5, 9, 13, 17], aligned=[1, 5, 9, 13])
    return _scene(w, [("points", {})], [dict(events=[(0, None)], num_filtered=5, errors=[1])])


def short_tracks():
    """point 0: an exact track of 3 (0 >= 3 - 3: deleted, counted 3); point 1: a track of 4 with one bad element (1 >= 4 - 3: deleted, counted 4)"""
    w = World(24)
    _point(w, 0, X, [0, 6, 12])
    _point(w, 1, Y, [0, 6, 12, 18], bad=[12])
    return _scene(w, [("points", {})], [dict(events=[(0, None), (1, None)], num_filtered=7, errors=[])])


def one_bad_of_five():
    """a track of 5 with one bad element (1 < 5 - 3): the element goes, the point stays with its error set"""
    w = World(24)
    t = _point(w, 0, X, [0, 4, 8, 12, 16], bad=[8])
    return _scene(w, [("points", {})], [dict(events=[(0, t[2])], num_filtered=1, errors=[0])])


def far_point():
    """point 0 at (300, 0, 0): every line exact, every pair of its five images below 1.5 degrees -> deleted, counted once; point 1 near the origin stays"""
    w = World(24)
    _point(w, 0, FAR, [10, 11, 12, 13, 14])
    _point(w, 1, X, [10, 11, 12, 13, 14])
    return _scene(w, [("points", {})], [dict(events=[(0, None)], num_filtered=1, errors=[1], by_angle=1)])


def angle_needs_deleted_element():
    """min_tri_angle 1 degree.  The point at (300, 0, 0) has exact lines in 10, 11, 13, 14 (at most 0.77 degrees apart) and an element in image 6, a quarter
    turn away: (6, 14) subtend 1.15 degrees - the only sufficient pair - but the point lies outside image 6, so that element is deleted first: the point
    goes, counted 1 (the element) + 1 (the point).  Point 1, the same five images around the origin, stays whole."""
    w = World(24)
    _point(w, 0, FAR, [10, 11, 6, 13, 14])
    _point(w, 1, X, [10, 11, 6, 13, 14])
    return _scene(w, [("points", dict(min_tri_angle=1.0))], [dict(events=[(0, None)], num_filtered=2, errors=[1], by_angle=1)])


def behind_and_outside():
    """the point at (6, 0, 0): exact lines in 10..14, an element in image 0 (the point is behind it) and one in image 18 (in front, outside the image): the two
    go (2 < 7 - 3), the point stays"""
    w = World(24)
    t = _point(w, 0, BEHIND, [10, 11, 0, 12, 13, 18, 14])
    return _scene(w, [("points", {})], [dict(events=[(0, t[2]), (0, t[5])], num_filtered=2, errors=[0])])


def point_subset():
    """two tracks of 3 (both would go); the subset names point 1 only"""
    w = World(24)
    _point(w, 0, X, [0, 6, 12])
    _point(w, 1, Y, [3, 9, 15])
    return _scene(w, [("points", dict(point3D_ids=[1]))], [dict(events=[(1, None)], num_filtered=3, errors=[])])


def image_subset():
    """FilterPoints3DInImages({17}): point 1 has an element there (a track of 5 with a bad element in image 9), point 0 (a track of 3) has none and is left alone"""
    w = World(24)
    _point(w, 0, X, [0, 6, 12])
    t = _point(w, 1, Y, [1, 5, 9, 13, 17], bad=[9])
    return _scene(w, [("points", dict(image_ids=[17]))], [dict(events=[(1, t[2])], num_filtered=1, errors=[1])])


def deleted_point_in_subset():
    """the first filter deletes point 0; the second one names 0 (gone: skipped) and 1 (a track of 5 with a bad element)"""
    w = World(24)
    _point(w, 0, X, [0, 6, 12])
    t = _point(w, 1, Y, [1, 5, 9, 13, 17], bad=[13])
    _point(w, 2, Z, [2, 8, 14])
    return _scene(w, [("points", dict(point3D_ids=[0])), ("points", dict(point3D_ids=[0, 1]))],
                  [dict(events=[(0, None)], num_filtered=3, errors=[]), dict(events=[(1, t[3])], num_filtered=1, errors=[1])])


def depth_track3_one_flag():
    """negative depth: a track of 3 with one element behind its image: DeleteObservation deletes the whole point; counted 1"""
    w = World(24)
    _point(w, 0, BEHIND, [0, 11, 13])
    return _scene(w, [("depth", {})], [dict(events=[(0, None)], num_filtered=1)])


def depth_track3_two_flags():
    """a track of 3 with two elements behind their images: the first takes the point, the second finds no point and is not counted"""
    w = World(24)
    _point(w, 0, BEHIND, [0, 1, 12])
    return _scene(w, [("depth", {})], [dict(events=[(0, None)], num_filtered=1)])


def depth_track4_two_flags():
    """a track of 4 with two flags: the first element goes alone, the second finds a track of 3 and takes the point; counted 2"""
    w = World(24)
    t = _point(w, 0, BEHIND, [0, 1, 11, 13])
    return _scene(w, [("depth", {})], [dict(events=[(0, t[0]), (0, None)], num_filtered=2)])


def registration_order():
    """image 0 was registered last (reg_index 7), so image 1 comes first: point 1's element there goes before point 0's in image 0; and point 2, a track
    of 4 flagged in both, loses the element of image 1 first and goes at image 0"""
    w = World(24)
    a = _point(w, 0, BEHIND, [0, 10, 11, 12, 13])
    b = _point(w, 1, BEHIND, [1, 10, 11, 12, 13])
    c = _point(w, 2, BEHIND, [0, 1, 12, 14])
    w.rec.images[0].reg_index = 7
    return _scene(w, [("depth", {})], [dict(events=[(1, b[0]), (2, c[1]), (0, a[0]), (2, None)], num_filtered=4)])


def long_tracks():
    """a ring of 130 images: point 0 has 65 elements (two lane passes; bad: positions 3 and 64), point 1 has 130 (three passes; bad: 0, 63, 64, 65, 128)"""
    w = World(130)
    t0 = _point(w, 0, X, list(range(65)), bad=[3, 64])
    t1 = _point(w, 1, Y, list(range(130)), bad=[0, 63, 64, 65, 128])
    return _scene(w, [("points", {})], [dict(events=[(0, t0[3]), (0, t0[64])] + [(1, t1[i]) for i in (0, 63, 64, 65, 128)], num_filtered=7, errors=[0, 1])])


def many_pairs():
    """a ring of 120 images, the point at (300, 0, 0) with 23 exact elements (253 pairs: four chunks of 64 lanes), every pair below 0.87 degrees.  The
    widest pair, images 48 and 71 (0.863 degrees; the next one 0.829), holds the LAST two places of the track: pair index 252.  First filter, min_tri_angle
    0.845: that one pair alone is sufficient, found in the last chunk - the point stays, its error set.  Second filter, 1.5 degrees: no pair in any chunk -
    the point goes by the angle rule, counted once."""
    w = World(120)
    _point(w, 0, FAR, list(range(50, 71)) + [48, 71])
    return _scene(w, [("points", dict(min_tri_angle=0.845)), ("points", {})],
                  [dict(events=[], num_filtered=0, errors=[0]), dict(events=[(0, None)], num_filtered=1, errors=[], by_angle=1)])


def filter_images():
    """a ring of 8 images.  Image 6 has a line but no point; image 7 has a camera of its own with a bogus focal length and sees point 0 (a track of 5: the
    element goes) and point 1 (a track of 3: the point goes); every other image keeps a point.  Both are de-registered, 6 first (registration order = id order)."""
    w = World(8)
    w.rec.cameras[1] = Camera(1, 2, np.array([1e6, 640.0, 480.0, 0.0]), width=1280, height=960)
    w.rec.images[7].camera_id = 1
    a = _point(w, 0, X, [0, 1, 2, 3, 7])
    _point(w, 1, Y, [4, 5, 7])
    _point(w, 2, Z, [0, 1, 2, 3, 4, 5])
    w.add_line(6, X)
    return _scene(w, [("images", {})], [dict(events=[(0, a[4]), (1, None)], num_filtered=2, filtered=[6, 7])])


HAND_BUILT = [aligned_only_track, short_tracks, one_bad_of_five, far_point, angle_needs_deleted_element, behind_and_outside, point_subset, image_subset,
              deleted_point_in_subset, depth_track3_one_flag, depth_track3_two_flags, depth_track4_two_flags, registration_order, long_tracks, many_pairs, filter_images]

# Corrupted synthetic worlds.  seed / image: tracks_image_scenes.SYNTHETIC's (the small world keeps every observation on its point, withheld=0: with a quarter
# withheld its tracks are 3 and 4 long, and no element can go while its point stays); `corrupt`: the seed of the corruption below, picked on the CPU with the reference
# alone so that every tested pixel error and angle keeps a relative margin above 1e-6 from its threshold; the measured margins are recorded beside it.
SYNTHETIC = [dict(cfg=(8, 60, 6), seed=6, image=3, scene_kw=dict(withheld=0.0), corrupt=1, margin_error=6.689e-2, margin_angle=2.765),
             dict(cfg=(12, 120, 8), seed=1, image=5, scene_kw={}, corrupt=1, margin_error=2.007e-3, margin_angle=8.409e-2)]


def corrupted_world(spec):
    """-> (rec, graph, ops, None).  Of the points: the first tenth moved 40 times as far out (small angles), the next tenth mirrored behind the cameras,
    the next tenth with aligned lines only; a twelfth of all lines of points get their offset spoiled.  ops: negative depth, the points of three images,
    a subset of the points, all points, then FilterImages."""
    rec, graph = synthetic_world(spec["cfg"], spec["seed"], spec["image"], **spec["scene_kw"])
    rng = np.random.default_rng(spec["corrupt"])
    ids = sorted(rec.points3D)
    n = max(len(ids) // 10, 2)
    for pid in ids[:n]:
        rec.points3D[pid].xyz = rec.points3D[pid].xyz * 40.0
    for pid in ids[n:2 * n]:
        rec.points3D[pid].xyz = -rec.points3D[pid].xyz - np.array([0.0, 0.0, 12.0])
    for pid in ids[2 * n:3 * n]:
        for (iid, idx) in rec.points3D[pid].track:
            rec.images[iid].lines[idx]._aligned = True
    obs = [(iid, idx) for pid in ids for (iid, idx) in rec.points3D[pid].track]
    for k in rng.choice(len(obs), len(obs) // 12, replace=False):
        fl = rec.images[obs[k][0]].lines[obs[k][1]]
        fl._line = fl._line + np.array([0.0, 0.0, rng.normal(0, 0.02)])
    image_ids = sorted(rec.images)
    ops = [("depth", {}), ("points", dict(image_ids=image_ids[:3])), ("points", dict(point3D_ids=ids[::3])), ("points", {}), ("images", {})]
    return rec, graph, ops, None


def all_scenes():
    """[(name, builder)]: builder() -> (rec, graph, ops, expect)"""
    out = [(f.__name__, f) for f in HAND_BUILT]
    for spec in SYNTHETIC:
        out.append(("corrupted_%dx%dx%d" % spec["cfg"], (lambda s=spec: corrupted_world(s))))
    return out
