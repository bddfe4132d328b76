"""Host mirror of the reference's track completion and merging (sfm/incremental_triangulator.{h,cc}: `CompleteTracks`, `CompleteAllTracks`,
`MergeTracks`, `MergeAllTracks`, `GetModifiedPoints3D`, `ClearModifiedPoints3D`) and of the `CorrespondenceGraph` query they read
(base/correspondence_graph.h `FindCorrespondences`), on top of pp_tracks_* (include/ppsfm_hip.h).

Each call flattens the reconstruction (`flatten`), hands it to the device and applies what comes back through `Reconstruction.AddObservation` /
`Reconstruction.MergePoints3D` - unless a `Session` is active (`with triangulator.Session(options):`), in which case ONE handle serves every call until the
block ends, the mapper's filters and de-registration included (pp_tracks_filter_*).  The reference visits the points in the order of an unordered_set; here the order is ASCENDING POINT ID.
`TriangulateImage` and `CompleteImage` (the two places where the reference creates points) visit the lines of the image in ascending index, as the
reference does.  `Retriangulate` (commented out in the reference) is not mirrored."""
import numpy as np

from . import _capi
from .bundle_adjustment import Camera, FeatureLine, Image, Point3D, Reconstruction
from .device import TracksProblem, tracks_image_options, tracks_options


class CorrespondenceGraph:
    """The part of base/correspondence_graph.h the triangulator reads: per (image, line) the corresponding (image, line) pairs, in a fixed order."""

    def __init__(self):
        self._corrs = {}

    def AddCorrespondence(self, image_id1, line_idx1, image_id2, line_idx2):
        self._corrs.setdefault((image_id1, line_idx1), []).append((image_id2, line_idx2))

    def FindCorrespondences(self, image_id, line_idx):
        return self._corrs.get((image_id, line_idx), [])

    def FindTransitiveCorrespondences(self, image_id, line_idx, transitivity):
        """base/correspondence_graph.cc:166-224: the direct list for transitivity 1; otherwise level by level, a line collected on first sight, and at
        the end the query (the first element) is overwritten by the LAST element - so the order is not plain breadth-first order"""
        if transitivity == 1:
            return list(self.FindCorrespondences(image_id, line_idx))
        if not self.FindCorrespondences(image_id, line_idx):
            return []
        found, seen = [(image_id, line_idx)], {(image_id, line_idx)}
        begin, end = 0, 1
        for _ in range(transitivity):
            for ref in found[begin:end]:
                for corr in self.FindCorrespondences(*ref):
                    if corr not in seen:
                        seen.add(corr)
                        found.append(corr)
            begin, end = end, len(found)
            if begin == end:
                break
        found[0] = found[-1]
        found.pop()
        return found

    def IsTwoViewObservation(self, image_id, line_idx):
        """base/correspondence_graph.cc:252-263"""
        corrs = self.FindCorrespondences(image_id, line_idx)
        return len(corrs) == 1 and len(self.FindCorrespondences(*corrs[0])) == 1

    # the per-image and per-pair queries of base/correspondence_graph.h:40-74, as they answer after Finalize

    def NumObservationsForImage(self, image_id):
        """lines of the image with at least one correspondence"""
        return sum(1 for (i, _), c in self._corrs.items() if i == image_id and c)

    def ExistsImage(self, image_id):
        """Finalize erases an image without an observation (base/correspondence_graph.cc:56-71)"""
        return self.NumObservationsForImage(image_id) > 0

    def NumCorrespondencesForImage(self, image_id):
        return sum(len(c) for (i, _), c in self._corrs.items() if i == image_id)

    def FindCorrespondencesBetweenImages(self, image_id1, image_id2):
        """base/correspondence_graph.cc:226-250 -> [(line_idx1, line_idx2)], ascending in line_idx1"""
        lines = sorted(x for (i, x) in self._corrs if i == image_id1)
        return [(x1, x2) for x1 in lines for (i2, x2) in self._corrs[(image_id1, x1)] if i2 == image_id2]

    def NumCorrespondencesBetweenImages(self, image_id1, image_id2):
        return len(self.FindCorrespondencesBetweenImages(image_id1, image_id2))


class FlatCorrespondenceGraph:
    """The same graph as arrays, the form pp_corr_graph_build leaves it in (include/ppsfm_hip.h, K18): the images in ascending id with their line counts,
    line x of the k-th image is global line line_start[k] + x, and the correspondences of global line l are corr_line[corr_start[l] : corr_start[l + 1]] in
    the order AddCorrespondences appended them.  Every query answers what CorrespondenceGraph answers, in the same order."""

    def __init__(self, image_ids, num_lines, corr_start, corr_line, image_connected=None):
        self.image_ids = [int(i) for i in image_ids]
        if sorted(set(self.image_ids)) != self.image_ids:
            raise ValueError("image_ids must ascend")
        self.num_lines = np.asarray(num_lines, dtype=np.int64).reshape(-1)
        self.line_start = np.zeros(len(self.image_ids) + 1, dtype=np.int64)
        self.line_start[1:] = np.cumsum(self.num_lines)
        self.corr_start = np.asarray(corr_start, dtype=np.int64).reshape(-1)
        self.corr_line = np.asarray(corr_line, dtype=np.int64).reshape(-1)
        if len(self.num_lines) != len(self.image_ids) or len(self.corr_start) != self.line_start[-1] + 1 or self.corr_start[-1] != len(self.corr_line):
            raise ValueError("the arrays do not describe one graph")
        self.image_connected = None if image_connected is None else np.asarray(image_connected, dtype=bool).reshape(-1)
        self._index = {i: k for k, i in enumerate(self.image_ids)}

    @classmethod
    def from_graph(cls, graph, num_lines_by_image):
        """the arrays of a CorrespondenceGraph over the images of {image_id: number of lines}"""
        image_ids = sorted(num_lines_by_image)
        offset, total = {}, 0
        for i in image_ids:
            offset[i] = total
            total += num_lines_by_image[i]
        corr_start, corr_line = np.zeros(total + 1, dtype=np.int64), []
        for i in image_ids:
            for x in range(num_lines_by_image[i]):
                corr_line.extend(offset[i2] + x2 for (i2, x2) in graph.FindCorrespondences(i, x))
                corr_start[offset[i] + x + 1] = len(corr_line)
        return cls(image_ids, [num_lines_by_image[i] for i in image_ids], corr_start, corr_line)

    def _line(self, image_id, line_idx):
        k = self._index.get(image_id)
        if k is None or not 0 <= line_idx < self.num_lines[k]:
            return -1
        return int(self.line_start[k]) + int(line_idx)

    def _refs(self, lines):
        """global lines -> [(image_id, line_idx)]"""
        lines = np.asarray(lines, dtype=np.int64)
        k = np.searchsorted(self.line_start, lines, side="right") - 1      # (an image without lines shares its start with the next: the last one wins)
        return [(self.image_ids[int(a)], int(b)) for a, b in zip(k, lines - self.line_start[k])]

    def FindCorrespondences(self, image_id, line_idx):
        l = self._line(image_id, line_idx)
        if l < 0:
            return []
        return self._refs(self.corr_line[self.corr_start[l]:self.corr_start[l + 1]])

    FindTransitiveCorrespondences = CorrespondenceGraph.FindTransitiveCorrespondences
    IsTwoViewObservation = CorrespondenceGraph.IsTwoViewObservation

    def NumObservationsForImage(self, image_id):
        k = self._index.get(image_id)
        if k is None:
            return 0
        s = self.corr_start[self.line_start[k]:self.line_start[k + 1] + 1]
        return int(np.count_nonzero(s[1:] > s[:-1]))

    def ExistsImage(self, image_id):
        return self.NumObservationsForImage(image_id) > 0

    def NumCorrespondencesForImage(self, image_id):
        k = self._index.get(image_id)
        if k is None:
            return 0
        return int(self.corr_start[self.line_start[k + 1]] - self.corr_start[self.line_start[k]])

    def FindCorrespondencesBetweenImages(self, image_id1, image_id2):
        k1, k2 = self._index.get(image_id1), self._index.get(image_id2)
        if k1 is None or k2 is None:
            return []
        l0, l1 = self.line_start[k1], self.line_start[k1 + 1]
        e0, e1 = self.corr_start[l0], self.corr_start[l1]
        nb = self.corr_line[e0:e1]
        owner = np.repeat(np.arange(l0, l1), np.diff(self.corr_start[l0:l1 + 1]))
        keep = (nb >= self.line_start[k2]) & (nb < self.line_start[k2 + 1])
        return [(int(a), int(b)) for a, b in zip(owner[keep] - l0, nb[keep] - self.line_start[k2])]

    def NumCorrespondencesBetweenImages(self, image_id1, image_id2):
        return len(self.FindCorrespondencesBetweenImages(image_id1, image_id2))

    def remapped_csr(self, image_ids, num_lines):
        """(corr_start [L' + 1], corr_line) int32 in the line numbering of ANOTHER image list (ascending ids, their line counts): a line of an image this
        graph does not hold has no neighbour, a neighbour in an image the list does not hold is dropped.  Vectorised: no loop over lines."""
        num_lines = np.asarray(num_lines, dtype=np.int64).reshape(-1)
        start = np.zeros(len(image_ids) + 1, dtype=np.int64)
        start[1:] = np.cumsum(num_lines)
        there = np.array([self._index.get(i, -1) for i in image_ids], dtype=np.int64)      # position here of every image of the list
        both = there >= 0
        if (num_lines[both] != self.num_lines[there[both]]).any():
            raise ValueError("an image has another number of lines than the correspondence graph was built with")
        # their line -> ours, our line -> theirs (-1: not held)
        to_ours = np.full(int(start[-1]), -1, dtype=np.int64)
        to_theirs = np.full(int(self.line_start[-1]), -1, dtype=np.int64)
        image_of = np.repeat(np.arange(len(image_ids)), num_lines)
        held = both[image_of]
        mine = np.arange(int(start[-1]))[held]
        ours = mine - start[image_of[held]] + self.line_start[there[image_of[held]]]
        to_ours[mine], to_theirs[ours] = ours, mine
        src = np.where(to_ours >= 0, to_ours, 0)
        degree = np.where(to_ours >= 0, self.corr_start[src + 1] - self.corr_start[src], 0)
        owner = np.repeat(np.arange(int(start[-1])), degree)
        first = np.cumsum(degree) - degree
        entry = self.corr_start[src][owner] + (np.arange(int(degree.sum())) - first[owner])
        nb = to_theirs[self.corr_line[entry]]
        keep = nb >= 0
        corr_start = np.zeros(int(start[-1]) + 1, dtype=np.int32)
        corr_start[1:] = np.cumsum(np.bincount(owner[keep], minlength=int(start[-1])))
        return corr_start, nb[keep].astype(np.int32)


class IncrementalTriangulator:
    class Options:
        """incremental_triangulator.h:37-90, the reference's defaults"""

        def __init__(self):
            self.max_transitivity = 1
            self.create_max_angle_error = 2.0
            self.continue_max_angle_error = 2.0
            self.merge_max_reproj_error = 4.0
            self.complete_max_reproj_error = 4.0
            self.complete_max_transitivity = 5
            self.re_max_angle_error = 5.0
            self.re_min_ratio = 0.2
            self.re_max_trials = 1
            self.min_angle = 1.5
            self.ignore_two_view_tracks = True
            self.min_focal_length_ratio = 0.1
            self.max_focal_length_ratio = 10.0
            self.max_extra_param = 1.0

        def Check(self):
            return (self.merge_max_reproj_error >= 0 and self.complete_max_reproj_error >= 0 and self.complete_max_transitivity >= 0 and
                    self.min_focal_length_ratio > 0 and self.max_focal_length_ratio > 0 and self.max_extra_param >= 0)

    def __init__(self, correspondence_graph, reconstruction, device=0):
        self.correspondence_graph_, self.reconstruction_, self.device_ = correspondence_graph, reconstruction, device
        self.modified_point3D_ids_ = set()
        self.last_reports = []      # the pp_tracks_report of every device call of the last driver call
        self._live = None           # the session of an active `with self.Session(...)`

    def AddModifiedPoint3D(self, point3D_id):
        self.modified_point3D_ids_.add(point3D_id)

    def GetModifiedPoints3D(self):
        rec = self.reconstruction_
        return set(p for p in self.modified_point3D_ids_ if p in rec.points3D)      # "assume that all other points were deleted"

    def ClearModifiedPoints3D(self):
        self.modified_point3D_ids_.clear()

    def flatten(self, options=None):
        """-> (flat dict for device.TracksProblem, point_ids [P], line_ref [L] = (image_id, line_idx)).  flat["line_aligned"] [L] holds
        FeatureLine.IsAligned (pp_tracks_triangulate_image's argument; not part of pp_tracks_desc).  Host only.  Lines are numbered image by
        image in id order; camera_skip is HasCameraBogusParams per camera (decided once per camera, :767-779)."""
        options = options or self.Options()
        rec, graph = self.reconstruction_, self.correspondence_graph_
        image_ids, point_ids, cam_ids = sorted(rec.images), sorted(rec.points3D), sorted(rec.cameras)
        unsized = [c for c in cam_ids if not hasattr(rec.cameras[c], "width")]
        if unsized:      # the line error's in-image gate and HasBogusParams both read the image size (Camera(..., width=, height=))
            raise ValueError("IncrementalTriangulator needs the width and height of every camera; missing for camera ids %s" % unsized)
        cam_index = {c: k for k, c in enumerate(cam_ids)}
        point_index = {p: k for k, p in enumerate(point_ids)}
        offset, line_ref = {}, []
        for iid in image_ids:
            offset[iid] = len(line_ref)
            line_ref.extend((iid, idx) for idx in range(len(rec.images[iid].lines)))
        L = len(line_ref)
        lines, line_image, line_point = np.zeros((L, 3)), np.zeros(L, dtype=np.int32), np.full(L, -1, dtype=np.int32)
        line_aligned = np.zeros(L, dtype=np.uint8)
        corr_start, corr_line = np.zeros(L + 1, dtype=np.int32), []
        flat_graph = isinstance(graph, FlatCorrespondenceGraph)      # the arrays are taken as they are, remapped to this reconstruction's images
        for c, iid in enumerate(image_ids):
            for idx, fl in enumerate(rec.images[iid].lines):
                l = offset[iid] + idx
                lines[l], line_image[l], line_aligned[l] = fl.Line(), c, fl.IsAligned()
                if fl.HasPoint3D():
                    line_point[l] = point_index[fl.Point3DId()]
                if not flat_graph:
                    corr_line.extend(offset[i2] + x2 for (i2, x2) in graph.FindCorrespondences(iid, idx) if i2 in offset)
                    corr_start[l + 1] = len(corr_line)
        if flat_graph:
            corr_start, corr_line = graph.remapped_csr(image_ids, [len(rec.images[i].lines) for i in image_ids])
        track_start, track_line = np.zeros(len(point_ids) + 1, dtype=np.int32), []
        for k, pid in enumerate(point_ids):
            track_line.extend(offset[iid] + idx for (iid, idx) in rec.points3D[pid].track)
            track_start[k + 1] = len(track_line)
        intr = np.zeros((len(cam_ids), _capi.CAM_STRIDE))
        for cid, k in cam_index.items():
            intr[k, : rec.cameras[cid].NumParams()] = rec.cameras[cid].params
        flat = dict(poses=np.array([np.concatenate([rec.images[i].qvec, rec.images[i].tvec]) for i in image_ids]).reshape(-1, 7),
                    pose_camera=np.array([cam_index[rec.images[i].camera_id] for i in image_ids], dtype=np.int32),
                    camera_model=np.array([rec.cameras[c].model_id for c in cam_ids], dtype=np.int32), intr=intr,
                    cam_size=np.array([[rec.cameras[c].width, rec.cameras[c].height] for c in cam_ids], dtype=np.int32).reshape(-1, 2),
                    camera_skip=np.array([rec.cameras[c].HasBogusParams(options.min_focal_length_ratio, options.max_focal_length_ratio, options.max_extra_param)
                                          for c in cam_ids], dtype=np.uint8),
                    image_registered=np.array([getattr(rec.images[i], "registered", True) for i in image_ids], dtype=np.uint8),
                    lines=lines, line_image=line_image, line_point=line_point, corr_start=corr_start, corr_line=np.array(corr_line, dtype=np.int32),
                    points=np.array([rec.points3D[p].xyz for p in point_ids]).reshape(-1, 3), track_start=track_start,
                    track_line=np.array(track_line, dtype=np.int32), line_aligned=line_aligned)
        return flat, point_ids, line_ref

    @staticmethod
    def device_options(options):
        return tracks_options(merge_max_reproj_error=options.merge_max_reproj_error, complete_max_reproj_error=options.complete_max_reproj_error,
                              complete_max_transitivity=options.complete_max_transitivity)

    def _open(self, options):
        """-> _TracksSession: ONE TracksProblem over the flattened reconstruction, on which several operations run one after the other (each applies
        its result to the reconstruction at once); close() it when done.  Internal: _run / _run_image and bundle_adjustment.AdjustLocalBundle."""
        assert options.Check()
        if self._live is not None:
            return self._live.reopen(options)
        return _TracksSession(self, options)

    def Session(self, options=None):
        """`with triangulator.Session(options) as ses:` - ONE TracksProblem for everything inside the block: while it is active `_open` hands out this live
        session (brought up to date with the reconstruction's poses, positions and intrinsics first) and the inner close() calls do nothing, so
        FindNextImages, RegisterNextImage, TriangulateImage, the local and global refinement and the mapper's filters run on one handle, from the first
        images of a reconstruction to its last.  Inside the block the points and observations of the reconstruction change through this module,
        bundle_adjustment's refinement functions (which find the active session through the reconstruction, with or without `triangulator=`) and the mapper
        only: a direct `Reconstruction.Filter*` / `DeleteObservation` / `DeletePoint3D` call would change the model behind the handle's back.
        EVERY `_open` inside the block still costs O(images + points) on the host: `update()` compares every pose, position and intrinsic parameter with what
        the handle holds and sends the ones that differ.
        A call whose options differ from the session's in a field the handle baked in (the camera_skip thresholds) raises ValueError."""
        return _LiveSession(self, options or self.Options())

    def _run(self, options, point3D_ids, complete, merge):
        assert options.Check()
        rec = self.reconstruction_
        self.last_reports = []
        if not rec.points3D:
            return 0, 0, [], []
        completed, merged, num_completed, num_merged = [], [], 0, 0
        ses = self._open(options)
        try:
            if complete:
                num_completed, completed = ses.complete(point3D_ids)
            if merge:
                num_merged, merged = ses.merge(point3D_ids)
        finally:
            ses.close()
        return num_completed, num_merged, completed, merged

    @staticmethod
    def device_image_options(options):
        return tracks_image_options(create_max_angle_error=options.create_max_angle_error, continue_max_angle_error=options.continue_max_angle_error,
                                    complete_max_reproj_error=options.complete_max_reproj_error, min_angle=options.min_angle,
                                    max_transitivity=options.max_transitivity, complete_max_transitivity=options.complete_max_transitivity,
                                    ignore_two_view_tracks=int(bool(options.ignore_two_view_tracks)))

    def _run_image(self, options, image_id, complete):
        assert options.Check()
        self.last_reports = []
        ses = self._open(options)
        try:
            return ses.complete_image(image_id) if complete else ses.triangulate_image(image_id)
        finally:
            ses.close()

    def TriangulateImage(self, options, image_id):
        """sfm/incremental_triangulator.cc:63-121 (Find, Continue, Create) -> num_tris"""
        return self._run_image(options, image_id, False)

    def CompleteImage(self, options, image_id):
        """sfm/incremental_triangulator.cc:123-235 -> num_tris"""
        return self._run_image(options, image_id, True)

    def CompleteTracks(self, options, point3D_ids):
        return self._run(options, point3D_ids, True, False)[0]

    def CompleteAllTracks(self, options):
        return self._run(options, None, True, False)[0]

    def MergeTracks(self, options, point3D_ids):
        return self._run(options, point3D_ids, False, True)[1]

    def MergeAllTracks(self, options):
        return self._run(options, None, False, True)[1]

    def CompleteAndMergeAllTracks(self, options):
        """CompleteAllTracks then MergeAllTracks (controllers/incremental_mapper.cc:160-172) on ONE device handle:
        -> (num_completed, num_merged, [(point id, (image_id, line_idx))], [(id a, id b, new id)])"""
        return self._run(options, None, True, True)


class _TracksSession:
    """One open TracksProblem of an IncrementalTriangulator (IncrementalTriangulator._open): the flattening's id maps, and per operation the device call
    and its application to the reconstruction.  `ids` maps a device point index to its point id; new points are appended as they are created."""

    def __init__(self, triangulator, options):
        self.t, self.options = triangulator, options
        self.rec = triangulator.reconstruction_
        self.flat, point_ids, self.line_ref = triangulator.flatten(options)
        self.ids = list(point_ids)
        self.image_ids = sorted(self.rec.images)
        self.cam_ids = sorted(self.rec.cameras)
        self.pb = TracksProblem(self.flat, device=triangulator.device_)

    live = False      # True: the session of a `with triangulator.Session(...)`, which outlives the call that opened it

    def close(self):
        self.pb.close()

    def _apply_deletions(self, events):
        """the events of a pp_tracks_filter_* call on the reconstruction: (p, -1) deletes the point, (p, l) removes that one element"""
        rec = self.rec
        for p, l in events:
            if l < 0:
                rec.DeletePoint3D(self.ids[int(p)])
            else:
                rec.DeleteObservation(*self.line_ref[int(l)])

    def filter_points(self, max_reproj_error, min_tri_angle, point3D_ids=None, image_ids=None):
        """Reconstruction::FilterPoints3D (point3D_ids) / FilterPoints3DInImages (image_ids) / FilterAllPoints3D (neither) on the handle and, through its
        events, on the reconstruction; Point3D.error is set on the points the filter kept -> num_filtered"""
        assert point3D_ids is None or image_ids is None
        images = None if image_ids is None else np.array([i in set(image_ids) for i in self.image_ids], dtype=np.uint8)
        rep, events, point_error = self.pb.filter_points(max_reproj_error, min_tri_angle, self.flat["line_aligned"], self._subset(point3D_ids), images)
        self.t.last_reports.append(rep)
        self._apply_deletions(events)
        for k in np.flatnonzero(point_error != -1.0):
            self.rec.points3D[self.ids[int(k)]].error = float(point_error[k])
        return int(rep.num_filtered)

    def _image_order(self):
        index = {i: c for c, i in enumerate(self.image_ids)}
        return [index[i] for i in self.rec.RegImageIds()]

    def filter_negative_depth(self):
        """Reconstruction::FilterObservationsWithNegativeDepth, the images in rec.RegImageIds() order -> num_filtered"""
        rep, events = self.pb.filter_negative_depth(self._image_order())
        self.t.last_reports.append(rep)
        self._apply_deletions(events)
        return int(rep.num_filtered)

    def filter_images(self):
        """Reconstruction::FilterImages with the thresholds of the session's options -> the ids of the de-registered images, in order"""
        rep, events, filtered = self.pb.filter_images(self._image_order())
        self.t.last_reports.append(rep)
        self._apply_deletions(events)
        out = [self.image_ids[int(c)] for c in filtered]
        for c, image_id in zip(filtered, out):
            self.rec.DeRegisterImage(image_id)
            self.flat["image_registered"][int(c)] = 0
        return out

    def _subset(self, point3D_ids):
        if point3D_ids is None:
            return None
        wanted = set(point3D_ids)
        return np.array([p in wanted for p in self.ids], dtype=np.uint8)

    def complete(self, point3D_ids=None):
        """CompleteTracks / CompleteAllTracks (None) -> (num_completed, [(point id, (image_id, line_idx))])"""
        rec, t = self.rec, self.t
        rep, pairs = self.pb.complete(t.device_options(self.options), self._subset(point3D_ids))
        t.last_reports.append(rep)
        completed = []
        for p, l in pairs:
            rec.AddObservation(self.ids[p], self.line_ref[l])
            t.modified_point3D_ids_.add(self.ids[p])
            completed.append((self.ids[p], self.line_ref[l]))
        return int(rep.num_changed), completed

    def merge(self, point3D_ids=None):
        """MergeTracks / MergeAllTracks (None) -> (num_merged, [(id a, id b, new id)])"""
        rec, t, ids = self.rec, self.t, self.ids
        rep, merges = self.pb.merge(t.device_options(self.options), self._subset(point3D_ids))
        t.last_reports.append(rep)
        merged = []
        for a, b, m in merges:
            new_id = rec.MergePoints3D(ids[a], ids[b])
            assert m == len(ids)
            t.modified_point3D_ids_.discard(ids[a]); t.modified_point3D_ids_.discard(ids[b])
            t.modified_point3D_ids_.add(new_id)
            merged.append((ids[a], ids[b], new_id))
            ids.append(new_id)
        return int(rep.num_changed), merged

    def _image(self, image_id, complete):
        rec, t, ids, line_ref = self.rec, self.t, self.ids, self.line_ref
        image = self.image_ids.index(image_id)
        o = t.device_image_options(self.options)
        rep, events = self.pb.complete_image(image, o) if complete else self.pb.triangulate_image(image, o, self.flat["line_aligned"])
        points = self.pb.state()["points"] if rep.points_created else None
        t.last_reports.append(rep)
        k = 0
        while k < len(events):
            p, l = int(events[k][0]), int(events[k][1])
            if p < len(ids):
                rec.AddObservation(ids[p], line_ref[l])
                t.modified_point3D_ids_.add(ids[p])
                k += 1
                continue
            assert p == len(ids)      # AddPoint3D: the whole track of the new point follows in track order
            k1 = k
            while k1 < len(events) and int(events[k1][0]) == p:
                k1 += 1
            new_id = rec.AddPoint3D(points[p], [line_ref[int(e[1])] for e in events[k:k1]])
            ids.append(new_id)
            t.modified_point3D_ids_.add(new_id)
            k = k1
        return int(rep.num_changed)

    def triangulate_image(self, image_id):
        return self._image(image_id, False)

    def complete_image(self, image_id):
        return self._image(image_id, True)

    def find_local_bundle(self, image_id, options):
        """FindLocalBundle -> (report, image ids in the reference's order)"""
        rep, bundle, _ = self.pb.find_local_bundle(self.image_ids.index(image_id), options)
        self.t.last_reports.append(rep)
        return rep, [self.image_ids[int(c)] for c in bundle]

    def find_next_images(self, options, num_reg_trials=None, filtered_images=()):
        """FindNextImages on the handle -> (report, image ids: first bucket, then second bucket).  options: a device.next_image_options;
        num_reg_trials {image id: trials}, filtered_images: ids (the mapper's num_reg_trials_ / filtered_images_)"""
        trials = np.array([(num_reg_trials or {}).get(i, 0) for i in self.image_ids], dtype=np.int32)
        filtered = np.array([i in filtered_images for i in self.image_ids], dtype=np.uint8)
        rep, ranked, _, _ = self.pb.find_next_images(options, trials, filtered)
        self.t.last_reports.append(rep)
        return rep, [self.image_ids[int(c)] for c in ranked]

    def find_initial_sets(self, options, check_image_ids, subset_image_ids=None):
        """The image-set search of RegisterInitialLineImages on the handle -> (report, sets: best first, each dict(image_ids [4] ascending, num_aligned,
        num_random, aligned, random: per track its four (image_id, line_idx) in the order of image_ids)).  options: a device.init_sets_options;
        subset_image_ids: the reference's aligned_db_cache (None: every image).  Nothing changes."""
        index = {i: c for c, i in enumerate(self.image_ids)}
        subset = None if subset_image_ids is None else np.array([i in set(subset_image_ids) for i in self.image_ids], dtype=np.uint8)
        rep, found = self.pb.find_initial_sets(self.flat["line_aligned"], [index[i] for i in check_image_ids], subset, options)
        self.t.last_reports.append(rep)
        sets = []
        for s in found:
            tracks = {name: [[self.line_ref[int(l)] for l in track] for track in s[name]] for name in ("aligned", "random")}
            sets.append(dict(image_ids=[self.image_ids[int(c)] for c in s["images"]], num_aligned=s["num_aligned"], num_random=s["num_random"], **tracks))
        return rep, sets

    def _point_indices(self):
        """{point id: handle index}; `ids` only grows, so the map is extended by what was appended since the last call"""
        index = self.__dict__.setdefault("_index_of_point", {})
        done = self.__dict__.get("_index_of_point_len", 0)
        for k in range(done, len(self.ids)):
            index[self.ids[k]] = k
        self._index_of_point_len = len(self.ids)
        return index

    def bundle_setup(self, config, options):
        """BundleAdjuster::SetUp on the handle (pp_tracks_bundle_setup) for a BundleAdjustmentConfig and BundleAdjustmentOptions
        -> (report, arrays as TracksProblem.bundle_setup's, pose image ids, point ids, camera ids - each in problem order).  The point lists go sorted
        by point id, as BundleAdjuster.flatten visits them.  The handle must hold the reconstruction's current positions (`update()`)."""
        rec = self.rec
        image_index = {i: c for c, i in enumerate(self.image_ids)}
        flags, tmask = np.zeros(len(self.image_ids), dtype=np.uint8), np.zeros(len(self.image_ids), dtype=np.uint8)
        for iid in config.Images():
            c = image_index[iid]
            flags[c] = _capi.PP_BUNDLE_IMAGE | (_capi.PP_BUNDLE_CONST_POSE if (not options.refine_extrinsics) or config.HasConstantPose(iid) else 0)
            if config.HasConstantTvec(iid):
                tmask[c] = sum(1 << i for i in config.ConstantTvec(iid))
        camera_const = np.array([config.IsConstantCamera(cid) for cid in self.cam_ids], dtype=np.uint8)
        subset = None
        if options.refine_focal_length or options.refine_principal_point or options.refine_extra_params:
            subset = np.zeros(len(self.cam_ids), dtype=np.uint16)
            for k, cid in enumerate(self.cam_ids):
                cam = rec.cameras[cid]
                idxs = ([] if options.refine_focal_length else list(cam.FocalLengthIdxs())) + \
                       ([] if options.refine_principal_point else list(cam.PrincipalPointIdxs())) + \
                       ([] if options.refine_extra_params else list(cam.ExtraParamsIdxs()))
                subset[k] = sum(1 << i for i in idxs)
        point_index = self._point_indices()
        variable = [point_index[p] for p in sorted(config.VariablePoints())]
        constant = [point_index[p] for p in sorted(config.ConstantPoints())]
        rep, out = self.pb.bundle_setup(flags, tmask, camera_const, subset, variable, constant)
        self.last_bundle_setup_report = rep      # (kept apart from the triangulator's last_reports, whose sequence per driver call is fixed)
        return (rep, out, [self.image_ids[int(c)] for c in out["pose_image"]], [self.ids[int(p)] for p in out["point_index"]],
                [self.cam_ids[int(k)] for k in out["camera_index"]])

    def estimate_image_pose(self, image_id, options, ransac):
        """RegisterNextImage up to the pose refinement -> (report, pose [7], corrs [n, 2] (handle line, handle point), inlier_mask [n],
        lines2D [n, 3], points3D [n, 3]: the arrays RefineAbsolutePoseFromLines takes).  The reconstruction does not change."""
        rep, pose, corrs, mask = self.pb.estimate_image_pose(self.image_ids.index(image_id), ransac, options, self.flat["line_aligned"])
        self.t.last_reports.append(rep)
        lines2D = self.flat["lines"][corrs[:, 0]].reshape(-1, 3)
        points3D = np.array([self.rec.points3D[self.ids[int(p)]].xyz for p in corrs[:, 1]], dtype=np.float64).reshape(-1, 3)
        return rep, pose, corrs, mask, lines2D, points3D

    def register_image(self, image_id, qvec, tvec, corrs, inlier_mask):
        """the commit of RegisterNextImage on the handle AND the reconstruction: the image registered at (qvec, tvec), one AddObservation per event
        -> [(point id, (image_id, line_idx))]"""
        rec, t = self.rec, self.t
        c = self.image_ids.index(image_id)
        pose = np.concatenate([np.asarray(qvec, dtype=np.float64), np.asarray(tvec, dtype=np.float64)])
        events = self.pb.register_image(c, pose, corrs, inlier_mask)
        image = rec.images[image_id]
        image.qvec, image.tvec, image.registered = pose[:4].copy(), pose[4:].copy(), True
        self.flat["poses"][c] = pose
        self.flat["image_registered"][c] = 1
        out = []
        for p, l in events:
            rec.AddObservation(self.ids[int(p)], self.line_ref[int(l)])
            t.AddModifiedPoint3D(self.ids[int(p)])      # (:754)
            out.append((self.ids[int(p)], self.line_ref[int(l)]))
        return out

    def update(self):
        """what a bundle adjustment changed in the reconstruction since the flattening (or the last update) goes to the handle: poses, positions of the
        points that still exist, intrinsics with camera_skip decided again"""
        rec, flat, o = self.rec, self.flat, self.options
        poses = np.array([np.concatenate([rec.images[i].qvec, rec.images[i].tvec]) for i in self.image_ids]).reshape(-1, 7)
        changed = (poses != flat["poses"]).any(axis=1)
        if self.live:      # (a failed RegisterNextImage may leave a non-finite pose on its unregistered image, pose.cc:86-89: no kernel reads it, the handle refuses it)
            changed &= np.isfinite(poses).all(axis=1) | flat["image_registered"].astype(bool)
        ii = np.flatnonzero(changed).astype(np.int32)
        live = [(k, pid) for k, pid in enumerate(self.ids) if pid in rec.points3D]
        npts = max(len(self.ids), flat["points"].shape[0])
        if flat["points"].shape[0] < npts:      # points created since: their positions came from the handle itself
            flat["points"] = np.concatenate([flat["points"].reshape(-1, 3), np.array([rec.points3D[pid].xyz if pid in rec.points3D else np.zeros(3)
                                                                                       for pid in self.ids[flat["points"].shape[0]:]]).reshape(-1, 3)])
        pi = np.array([k for k, pid in live if (rec.points3D[pid].xyz != flat["points"][k]).any()], dtype=np.int32)
        xyz = np.array([rec.points3D[self.ids[k]].xyz for k in pi]).reshape(-1, 3)
        intr = np.zeros_like(flat["intr"])
        for k, cid in enumerate(self.cam_ids):
            intr[k, : rec.cameras[cid].NumParams()] = rec.cameras[cid].params
        skip = None
        if (intr != flat["intr"]).any():
            skip = np.array([rec.cameras[c].HasBogusParams(o.min_focal_length_ratio, o.max_focal_length_ratio, o.max_extra_param) for c in self.cam_ids], dtype=np.uint8)
        else:
            intr = None
        self.pb.update(ii, poses[ii], pi, xyz, intr, skip)
        flat["poses"] = poses
        for k, x in zip(pi, xyz):
            flat["points"][k] = x
        if intr is not None:
            flat["intr"], flat["camera_skip"] = intr, skip


class _LiveTracksSession(_TracksSession):
    live = True

    def close(self):      # (the inner calls' close(): the handle lives until the `with` block ends)
        pass

    def reopen(self, options):
        baked = ("min_focal_length_ratio", "max_focal_length_ratio", "max_extra_param")
        if any(getattr(options, f) != getattr(self.baked_options, f) for f in baked):
            raise ValueError("the options differ from the session's in %s, which the handle's camera_skip was decided with" %
                             [f for f in baked if getattr(options, f) != getattr(self.baked_options, f)])
        self.options = options
        self.update()      # what changed in the reconstruction's values since the last call (a bundle adjustment, Normalize, a camera reset)
        return self


class _LiveSession:
    """the context manager of IncrementalTriangulator.Session"""

    def __init__(self, triangulator, options):
        assert options.Check()
        self.t, self.options, self.ses = triangulator, options, None

    def __enter__(self):
        assert self.t._live is None, "a Session is active already"
        self.ses = _LiveTracksSession(self.t, self.options)
        self.ses.baked_options = self.options
        self.t._live = self.ses
        self.t.reconstruction_._session_triangulator = self.t      # (bundle_adjustment's refinement functions find the session without being handed it)
        return self.ses

    def __exit__(self, *exc):
        self.t._live = None
        self.t.reconstruction_._session_triangulator = None
        self.ses.pb.close()
        return False


def reconstruction_from_completion_scene(scene):
    """(Reconstruction, CorrespondenceGraph) of synthetic.make_completion_scene: image ids 0..C-1, point ids 0..P'-1, the cameras sized by `cam_size`"""
    rec, graph = Reconstruction(), CorrespondenceGraph()
    for k in range(scene["intr"].shape[0]):
        m = int(scene["camera_model"][k])
        rec.cameras[k] = Camera(k, m, scene["intr"][k, : _capi.lib().pp_camera_num_params(m)], width=int(scene["cam_size"][k, 0]), height=int(scene["cam_size"][k, 1]))
    for c in range(scene["poses"].shape[0]):
        rec.images[c] = Image(c, int(scene["pose_camera"][c]), scene["poses"][c, :4], scene["poses"][c, 4:])
    for p in range(scene["points"].shape[0]):
        rec.points3D[p] = Point3D(scene["points"][p])
    ref = []
    for l in range(len(scene["line_image"])):
        c, p = int(scene["line_image"][l]), int(scene["line_point"][l])
        rec.images[c].lines.append(FeatureLine(scene["line_xyz"][l], False, p))
        ref.append((c, len(rec.images[c].lines) - 1))
        if p >= 0:
            rec.points3D[p].track.append(ref[-1])
    cs, cl = scene["corr_start"], scene["corr_line"]
    for l in range(len(ref)):
        for e in range(cs[l], cs[l + 1]):
            graph.AddCorrespondence(ref[l][0], ref[l][1], ref[cl[e]][0], ref[cl[e]][1])
    return rec, graph
