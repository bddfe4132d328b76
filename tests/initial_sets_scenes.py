"""Correspondence graphs for the image-set search of RegisterInitialLineImages (pp_tracks_find_initial_sets) - TEST INFRASTRUCTURE, shared by the CPU tests
(initial_sets_reference.py, the replay driver) and the GPU test: hand-built graphs, the smallest that can go wrong, a seeded fuzz and the synthetic graph
of the measurement in DESIGN.md.

A scene: dict(num_images, line_image [L], line_aligned [L], corr [L] lists of line numbers (DIRECTED: corr[a] holds b when a -> b), check_images,
subset (image indices or None), options (the three thresholds)).  Lines are numbered image by image, as IncrementalTriangulator.flatten numbers them."""
import numpy as np


class Builder:
    def __init__(self, num_images):
        self.num_images = num_images
        self.lines = [[] for _ in range(num_images)]      # per image: the alignment flag of each line
        self.edges = []                                   # ((image, idx), (image, idx)), directed, in insertion order

    def line(self, image, aligned):
        self.lines[image].append(bool(aligned))
        return (image, len(self.lines[image]) - 1)

    def edge(self, a, b, both=True):
        self.edges.append((a, b))
        if both:
            self.edges.append((b, a))

    def clique(self, images, aligned):
        """one line in each image, all matched to each other: one 4-view track per four of them"""
        members = [self.line(c, aligned) for c in images]
        for a in members:
            for b in members:
                if a != b:
                    self.edge(a, b, both=False)
        return members

    def scene(self, check_images, subset=None, **options):
        offset = np.concatenate([[0], np.cumsum([len(l) for l in self.lines])]).astype(int)
        line_image = [c for c, l in enumerate(self.lines) for _ in l]
        line_aligned = [int(f) for l in self.lines for f in l]
        corr = [[] for _ in line_image]
        for (a, b) in self.edges:
            corr[offset[a[0]] + a[1]].append(int(offset[b[0]] + b[1]))
        opts = dict(min_num_aligned_tracks=20, min_num_random_tracks=20, max_num_sets=10)
        opts.update(options)
        return dict(num_images=self.num_images, line_image=line_image, line_aligned=line_aligned, corr=corr, check_images=list(check_images),
                    subset=None if subset is None else list(subset), options=opts)


def to_flat(scene):
    """the flat dict of device.TracksProblem for a scene: one camera, every image unregistered at the identity, NO points (P = 0)"""
    C, L = scene["num_images"], len(scene["line_image"])
    corr_start = np.concatenate([[0], np.cumsum([len(c) for c in scene["corr"]])]).astype(np.int32)
    return dict(poses=np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (C, 1)), pose_camera=np.zeros(C, dtype=np.int32), camera_model=np.array([2], dtype=np.int32),
                intr=np.array([[1000.0, 640.0, 480.0, 0.0] + [0.0] * 8]), cam_size=np.array([[1280, 960]], dtype=np.int32), camera_skip=np.zeros(1, dtype=np.uint8),
                image_registered=np.zeros(C, dtype=np.uint8), lines=np.tile(np.array([1.0, 0.0, 0.0]), (L, 1)), line_image=np.array(scene["line_image"], dtype=np.int32),
                line_point=np.full(L, -1, dtype=np.int32), corr_start=corr_start, corr_line=np.array([n for c in scene["corr"] for n in c], dtype=np.int32),
                points=np.zeros((0, 3)), track_start=np.zeros(1, dtype=np.int32), track_line=np.zeros(0, dtype=np.int32),
                line_aligned=np.array(scene["line_aligned"], dtype=np.uint8))


ONE = dict(min_num_aligned_tracks=1, min_num_random_tracks=1)


def _star(neighbour_images, neighbour_aligned=None, num_images=5, both=True):
    """line r (aligned, image 0) matched to one new line in each of `neighbour_images`"""
    b = Builder(num_images)
    r = b.line(0, True)
    for k, c in enumerate(neighbour_images):
        b.edge(r, b.line(c, True if neighbour_aligned is None else neighbour_aligned[k]), both=both)
    return b


def two_neighbours():
    return _star([1, 2]).scene([0], **ONE)


def three_neighbours():
    return _star([1, 2, 3]).scene([0], **ONE)


def two_neighbours_in_one_image():
    return _star([1, 1, 2, 3]).scene([0], **ONE)


def neighbour_in_own_image():
    return _star([0, 1, 2, 3]).scene([0], **ONE)


def neighbour_of_other_alignment():
    return _star([1, 2, 3, 4], [True, True, True, False]).scene([0], **ONE)


def neighbour_outside_subset():
    return _star([1, 2, 3, 4]).scene([0], subset=[0, 1, 2, 3], **ONE)


def one_directional():
    return _star([1, 2, 3], both=False).scene([0, 1, 2, 3], **ONE)


def shared_track(num_check):
    """one aligned and one unaligned track, each reachable from all four of its members"""
    b = Builder(4)
    b.clique([0, 1, 2, 3], True)
    b.clique([0, 1, 2, 3], False)
    return b.scene(list(range(num_check)), **ONE)


def _sets(spec, num_images, **options):
    """spec: [(images, aligned tracks, unaligned tracks)] - every track its own clique"""
    b = Builder(num_images)
    for images, na, nr in spec:
        for _ in range(na):
            b.clique(images, True)
        for _ in range(nr):
            b.clique(images, False)
    return b.scene(list(range(num_images)), **options)


def thresholds():
    """min 3 / 3: (0,1,2,3) sits exactly on both, (0,1,2,4) is one aligned track short, (0,1,3,4) one unaligned track short, (0,2,3,4) has no unaligned at all"""
    return _sets([((0, 1, 2, 3), 3, 3), ((0, 1, 2, 4), 2, 3), ((0, 1, 3, 4), 3, 2), ((0, 2, 3, 4), 5, 0)], 5, min_num_aligned_tracks=3, min_num_random_tracks=3)


def tied_sets():
    """(1,2,3,4) leads; (0,1,2,4) and (0,1,2,3) tie on the aligned count and differ in the unaligned one, which must not matter"""
    return _sets([((0, 1, 2, 4), 3, 5), ((1, 2, 3, 4), 4, 2), ((0, 1, 2, 3), 3, 2)], 5, min_num_aligned_tracks=2, min_num_random_tracks=2)


def more_sets_than_returned():
    """all 15 quadruples of 6 images qualify; the aligned counts 2..6 repeat, so the cut at ten sets falls inside a group of ties"""
    from itertools import combinations
    spec = [(images, 2 + k % 5, 2) for k, images in enumerate(combinations(range(6), 4))]
    return _sets(spec, 6, min_num_aligned_tracks=2, min_num_random_tracks=2)


def long_list():
    """80 images of two lines each, the aligned lines all matched to each other and the unaligned ones too: the 79 neighbours of a line are more than a
    wavefront and more than the on-chip list.  One check image: C(79, 3) tracks per class, every set with one of each."""
    b = Builder(80)
    b.clique(list(range(80)), True)
    b.clique(list(range(80)), False)
    return b.scene([0], **ONE)


def fuzz(seed):
    """6-12 images, 5-40 lines each, random flags; "points" seen in 3-7 images (now and then twice in one) whose lines are matched with dropped and
    one-directional edges, and random edges on top; a random subset and random check images in it; thresholds of 2-3"""
    rng = np.random.default_rng(1000 + seed)
    C = int(rng.integers(6, 13))
    b = Builder(C)
    per_image = [int(rng.integers(5, 41)) for _ in range(C)]
    lines = [[b.line(c, rng.random() < 0.5) for _ in range(per_image[c])] for c in range(C)]
    for _ in range(int(sum(per_image) * 0.6)):
        images = rng.choice(C, int(rng.integers(3, min(C, 7) + 1)), replace=rng.random() < 0.15)
        members = [lines[c][int(rng.integers(0, per_image[c]))] for c in images]
        if rng.random() < 0.7:      # mostly of one flag, so that tracks survive the alignment filter
            flag = b.lines[members[0][0]][members[0][1]]
            members = [m for m in members if b.lines[m[0]][m[1]] == flag]
        for a in members:
            for other in members:
                if a != other and rng.random() < 0.85:
                    b.edge(a, other, both=False)
    for _ in range(int(sum(per_image) * 0.3)):
        c1, c2 = rng.integers(0, C, 2)
        b.edge(lines[c1][int(rng.integers(0, per_image[c1]))], lines[c2][int(rng.integers(0, per_image[c2]))], both=rng.random() < 0.5)
    subset = None if rng.random() < 0.3 else sorted(int(c) for c in rng.choice(C, max(4, C - int(rng.integers(1, 3))), replace=False))
    pool = list(range(C)) if subset is None else subset
    check = sorted(int(c) for c in rng.choice(pool, int(rng.integers(1, len(pool) + 1)), replace=False))
    return b.scene(check, subset=subset, min_num_aligned_tracks=int(rng.integers(2, 4)), min_num_random_tracks=int(rng.integers(2, 4)),
                   max_num_sets=int(rng.integers(3, 11)))


def timing_scene(num_check=10, lines_per_image=2000, num_images=16, seed=0):
    """the synthetic size of the measurement: `num_images` images of `lines_per_image` lines; line k of every image belongs to "point" k, which is seen in a
    random 9-13 of the images (so a line has 8-12 neighbours of its own flag); the first `num_check` images are the check images"""
    rng = np.random.default_rng(seed)
    b = Builder(num_images)
    for k in range(lines_per_image):
        flag = k % 2 == 0
        members = [b.line(c, flag) for c in range(num_images)]
        seen = [members[c] for c in sorted(rng.choice(num_images, int(rng.integers(9, 14)), replace=False))]
        for a in seen:
            for other in seen:
                if a != other:
                    b.edge(a, other, both=False)
    return b.scene(list(range(num_check)))


HAND_BUILT = [("two_neighbours", two_neighbours), ("three_neighbours", three_neighbours), ("two_neighbours_in_one_image", two_neighbours_in_one_image),
              ("neighbour_in_own_image", neighbour_in_own_image), ("neighbour_of_other_alignment", neighbour_of_other_alignment),
              ("neighbour_outside_subset", neighbour_outside_subset), ("one_directional", one_directional),
              ("shared_track_1", lambda: shared_track(1)), ("shared_track_2", lambda: shared_track(2)), ("shared_track_4", lambda: shared_track(4)),
              ("thresholds", thresholds), ("tied_sets", tied_sets), ("more_sets_than_returned", more_sets_than_returned), ("long_list", long_list)]
NUM_FUZZ = 20


def all_scenes():
    return HAND_BUILT + [("fuzz_%02d" % s, (lambda s=s: fuzz(s))) for s in range(NUM_FUZZ)]
