"""From keypoints to line features: the part of the reference's feature extraction that is not image processing.

`FeatureKeypoint` (feature/types.cc:38-105), `ScaleKeypoints` / `MaskKeypoints` (feature/extraction.cc:49-85), `LoadSiftFeaturesFromTextFile`
(feature/sift.cc:902-955) and the line generation of LineFeatureWriterThread::Run (feature/extraction.cc:437-505): every keypoint is undistorted with its
image's camera and gets a line through it - gravity-aligned for a share `aligned_line_ratio` of the features of an image that has a gravity direction,
of random direction otherwise - divided by the norm of its first two components.  The keypoints and descriptors themselves come from
`ExtractSiftFeatures` (ExtractSiftFeaturesCPU, feature/sift.cc:399-573, on the device: K21, csrc/sift_extract.hip), and `extract_features_to_lines`
runs both steps over a list of images.

`generate_line_features` is the numpy host mirror (ImageToWorld with the reference's Newton iteration restated literally, the counter-based generator
of csrc/line_features_replay.hpp restated in uint64 arithmetic), `generate_line_features_on_device` the same through pp_line_features_from_keypoints
(K19, csrc/line_features.hip).  Both fill `image.lines` with `FeatureLine(line, aligned, -1)`; line index = keypoint index = descriptor row, which is
what lets the matches of the descriptor matcher be line indices of the correspondence graph.
"""
import math

import numpy as np

from . import _capi
from .bundle_adjustment import FeatureLine, kInvalidPoint3DId

DEFAULT_ALIGNED_LINE_RATIO = 0.5      # feature/extraction.cc:160-162
_EPS = float(np.finfo(np.float64).eps)
_U64 = np.uint64
_f32 = np.float32


class FeatureKeypoint:
    """feature/types.h:44-78 / types.cc:38-105: location and the 2 x 2 affine shape, all float32."""

    def __init__(self, x=0.0, y=0.0, *shape):
        self.x, self.y = _f32(x), _f32(y)
        if len(shape) == 0:
            shape = (1, 0, 0, 1)
        if len(shape) == 2:
            scale, orientation = _f32(shape[0]), _f32(shape[1])
            if not scale >= 0.0:
                raise ValueError("CHECK_GE(scale, 0.0)")
            c, s = _f32(scale * _f32(np.cos(orientation))), _f32(scale * _f32(np.sin(orientation)))
            shape = (c, -s, s, c)
        if len(shape) != 4:
            raise TypeError("FeatureKeypoint(x, y), (x, y, scale, orientation) or (x, y, a11, a12, a21, a22)")
        self.a11, self.a12, self.a21, self.a22 = (_f32(v) for v in shape)

    @staticmethod
    def FromParameters(x, y, scale_x, scale_y, orientation, shear):
        scale_x, scale_y, orientation, shear = _f32(scale_x), _f32(scale_y), _f32(orientation), _f32(shear)
        return FeatureKeypoint(x, y, scale_x * np.cos(orientation), -scale_y * np.sin(_f32(orientation + shear)),
                               scale_x * np.sin(orientation), scale_y * np.cos(_f32(orientation + shear)))

    def Rescale(self, scale_x, scale_y=None):
        scale_y = scale_x if scale_y is None else scale_y
        scale_x, scale_y = _f32(scale_x), _f32(scale_y)
        if not (scale_x > 0 and scale_y > 0):
            raise ValueError("CHECK_GT(scale, 0)")
        self.x, self.y = _f32(self.x * scale_x), _f32(self.y * scale_y)
        self.a11, self.a12 = _f32(self.a11 * scale_x), _f32(self.a12 * scale_y)
        self.a21, self.a22 = _f32(self.a21 * scale_x), _f32(self.a22 * scale_y)

    def ComputeScale(self):
        return _f32((self.ComputeScaleX() + self.ComputeScaleY()) / _f32(2.0))

    def ComputeScaleX(self):
        return _f32(np.sqrt(_f32(self.a11 * self.a11 + self.a21 * self.a21)))

    def ComputeScaleY(self):
        return _f32(np.sqrt(_f32(self.a12 * self.a12 + self.a22 * self.a22)))

    def ComputeOrientation(self):
        return _f32(np.arctan2(self.a21, self.a11))

    def ComputeShear(self):
        return _f32(_f32(np.arctan2(-self.a12, self.a22)) - self.ComputeOrientation())


def FeatureKeypointsToPointsVector(keypoints):
    """feature/utils.cc: [N, 2] float32 (x, y) of a list of FeatureKeypoint (or of an array, whose first two columns are taken)"""
    if isinstance(keypoints, np.ndarray):
        if keypoints.size == 0:
            return np.zeros((0, 2), dtype=np.float32)
        return np.ascontiguousarray(keypoints.reshape(len(keypoints), -1)[:, :2], dtype=np.float32)
    return np.array([[k.x, k.y] for k in keypoints], dtype=np.float32).reshape(-1, 2)


def ScaleKeypoints(bitmap_size, camera, keypoints):
    """extraction.cc:49-59: bitmap_size = (width, height) of the image the keypoints were found in; rescaled in place to the camera's size"""
    bw, bh = int(bitmap_size[0]), int(bitmap_size[1])
    if bw != camera.width or bh != camera.height:
        scale_x, scale_y = _f32(_f32(camera.width) / _f32(bw)), _f32(_f32(camera.height) / _f32(bh))
        for k in keypoints:
            k.Rescale(scale_x, scale_y)


def MaskKeypoints(mask, keypoints, descriptors):
    """extraction.cc:61-85: mask [H, W] (or [H, W, 3]: its red channel); a keypoint whose coordinates, truncated to int, fall outside the mask or on a
    zero pixel is dropped -> (keypoints, descriptors), the descriptors row-aligned with the keypoints that stay"""
    mask = np.asarray(mask)
    if mask.ndim == 3:
        mask = mask[:, :, 0]
    h, w = mask.shape
    keep = []
    for i, k in enumerate(keypoints):
        x, y = int(k.x), int(k.y)      # static_cast<int>: towards zero
        if 0 <= x < w and 0 <= y < h and mask[y, x] != 0:
            keep.append(i)
    descriptors = np.asarray(descriptors)
    return [keypoints[i] for i in keep], np.ascontiguousarray(descriptors[keep].reshape(len(keep), descriptors.shape[1]))


def LoadSiftFeaturesFromTextFile(path):
    """sift.cc:902-955: "N 128", then per feature "x y scale orientation d_0 .. d_127" -> (keypoints, descriptors [N, 128] uint8)"""
    with open(path) as f:
        header = f.readline().split()
        num_features, dim = int(header[0]), int(header[1])
        if dim != 128:
            raise ValueError("SIFT features must have 128 dimensions")
        keypoints, descriptors = [], np.zeros((num_features, dim), dtype=np.uint8)
        for i in range(num_features):
            items = f.readline().split()
            if len(items) < 4 + dim:
                raise ValueError("feature %d: %d values, %d expected" % (i, len(items), 4 + dim))
            keypoints.append(FeatureKeypoint(float(items[0]), float(items[1]), float(items[2]), float(items[3])))
            values = np.array([float(v) for v in items[4:4 + dim]], dtype=np.float32)
            if np.any(values < 0) or np.any(values > 255):
                raise ValueError("CHECK_GE(value, 0); CHECK_LE(value, 255)")
            descriptors[i] = values.astype(np.uint8)      # TruncateCast<float, uint8_t>
    return keypoints, descriptors


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# camera models: the mirror of csrc/camera_models.hpp (Distortion, IterativeUndistortion, ImageToWorld)

_ONE_FOCAL = (0, 2, 3, 8, 9)
UNDISTORT_MAX_ITERATIONS = 100


def _fisheye(k, u, v):
    r = np.sqrt(u * u + v * v)
    ok = r > _EPS
    rs = np.where(ok, r, 1.0)
    theta = np.arctan(rs)
    t2 = theta * theta
    series = 1.0 + k[0] * t2
    if len(k) >= 2:
        t4 = t2 * t2
        series = series + k[1] * t4
        if len(k) >= 4:
            series = series + k[2] * (t4 * t2) + k[3] * (t4 * t4)
    thetad = theta * series
    return np.where(ok, u * thetad / rs - u, 0.0), np.where(ok, v * thetad / rs - v, 0.0)


def distortion(model, p, u, v):
    """CameraModel::Distortion by model id on arrays; p the whole parameter row (FOV: the distorted point itself, as in the reference)"""
    if model == 2 or model == 3:
        r2 = u * u + v * v
        radial = p[3] * r2 + (p[4] * r2 * r2 if model == 3 else 0.0)
        return u * radial, v * radial
    if model == 4:
        u2, uv, v2 = u * u, u * v, v * v
        r2 = u2 + v2
        radial = p[4] * r2 + p[5] * r2 * r2
        return (u * radial + 2.0 * p[6] * uv + p[7] * (r2 + 2.0 * u2), v * radial + 2.0 * p[7] * uv + p[6] * (r2 + 2.0 * v2))
    if model == 5:
        return _fisheye(p[4:8], u, v)
    if model == 6:
        u2, uv, v2 = u * u, u * v, v * v
        r2 = u2 + v2
        r4 = r2 * r2
        r6 = r4 * r2
        radial = (1.0 + p[4] * r2 + p[5] * r4 + p[8] * r6) / (1.0 + p[9] * r2 + p[10] * r4 + p[11] * r6)
        return (u * radial + 2.0 * p[6] * uv + p[7] * (r2 + 2.0 * u2) - u, v * radial + 2.0 * p[7] * uv + p[6] * (r2 + 2.0 * v2) - v)
    if model == 7:
        omega = p[4]
        radius2, omega2 = u * u + v * v, omega * omega
        if omega2 < 1e-4:
            factor = (omega2 * radius2) / 3.0 - omega2 / 12.0 + 1.0
        else:
            th = math.tan(omega / 2.0)
            small = radius2 < 1e-4
            radius = np.sqrt(np.where(small, 1.0, radius2))
            factor = np.where(small, (-2.0 * th * (4.0 * radius2 * th * th - 3.0)) / (3.0 * omega), np.arctan(radius * 2.0 * th) / (radius * omega))
        return u * factor, v * factor
    if model == 8:
        return _fisheye(p[3:4], u, v)
    if model == 9:
        return _fisheye(p[3:5], u, v)
    if model == 10:
        u2, uv, v2 = u * u, u * v, v * v
        r2 = u2 + v2
        r4 = r2 * r2
        r6 = r4 * r2
        r8 = r6 * r2
        radial = p[4] * r2 + p[5] * r4 + p[8] * r6 + p[9] * r8
        return (u * radial + 2.0 * p[6] * uv + p[7] * (r2 + 2.0 * u2) + p[10] * r2, v * radial + 2.0 * p[7] * uv + p[6] * (r2 + 2.0 * v2) + p[11] * r2)
    raise ValueError("camera model %d has no distortion" % model)


def iterative_undistortion(model, p, u, v, max_iterations=UNDISTORT_MAX_ITERATIONS, extra_iterations=0):
    """BaseCameraModel::IterativeUndistortion (camera_models.h:547-588) per element of u, v -> (u, v, iterations [N]).  extra_iterations: every element goes
    on for that many Newton steps after it met the stopping rule (a test's probe of how far the rule stops from the fixed point)."""
    x0, y0 = np.array(u, dtype=np.float64), np.array(v, dtype=np.float64)
    x, y = x0.copy(), y0.copy()
    iterations = np.zeros(x.shape, dtype=np.int64)
    met = np.zeros(x.shape, dtype=bool)                      # the stopping rule (or the iteration limit) has been met
    extra_left = np.full(x.shape, int(extra_iterations), dtype=np.int64)
    active = np.ones(x.shape, dtype=bool)
    with np.errstate(all="ignore"):
        while active.any():
            a = np.nonzero(active)[0]
            xa, ya = x[a], y[a]
            s0 = np.maximum(_EPS, np.abs(1e-6 * xa))
            s1 = np.maximum(_EPS, np.abs(1e-6 * ya))
            dx, dy = distortion(model, p, xa, ya)
            bx0, by0 = distortion(model, p, xa - s0, ya)
            fx0, fy0 = distortion(model, p, xa + s0, ya)
            bx1, by1 = distortion(model, p, xa, ya - s1)
            fx1, fy1 = distortion(model, p, xa, ya + s1)
            j00 = 1 + (fx0 - bx0) / (2 * s0)
            j01 = (fx1 - bx1) / (2 * s1)
            j10 = (fy0 - by0) / (2 * s0)
            j11 = 1 + (fy1 - by1) / (2 * s1)
            inv_det = 1.0 / (j00 * j11 - j01 * j10)
            rx, ry = xa + dx - x0[a], ya + dy - y0[a]
            step_x = (j11 * inv_det) * rx + (-j01 * inv_det) * ry
            step_y = (-j10 * inv_det) * rx + (j00 * inv_det) * ry
            x[a], y[a] = xa - step_x, ya - step_y
            was_met = met[a]
            iterations[a] += ~was_met
            extra_left[a] -= was_met
            met[a] = was_met | (step_x * step_x + step_y * step_y < 1e-10) | (iterations[a] >= int(max_iterations))
            active[a] = ~met[a] | (extra_left[a] > 0)
    return x, y, iterations


def image_to_world(model, params, xy, extra_iterations=0):
    """every model's ImageToWorld on [N, 2] pixels -> (uv [N, 2], iterations [N]: Newton steps, 0 for the closed forms)"""
    model = int(model)
    p = np.asarray(params, dtype=np.float64)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    if model in _ONE_FOCAL:
        u, v = (xy[:, 0] - p[1]) / p[0], (xy[:, 1] - p[2]) / p[0]
    else:
        u, v = (xy[:, 0] - p[2]) / p[0], (xy[:, 1] - p[3]) / p[1]
    iterations = np.zeros(len(xy), dtype=np.int64)
    with np.errstate(all="ignore"):
        if model in (0, 1):
            pass
        elif model == 7:
            omega = p[4]
            radius2, omega2 = u * u + v * v, omega * omega
            if omega2 < 1e-4:
                factor = (omega2 * radius2) / 3.0 - omega2 / 12.0 + 1.0
            else:
                small = radius2 < 1e-4
                radius = np.sqrt(np.where(small, 1.0, radius2))
                factor = np.where(small, (omega * (omega * omega * radius2 + 3.0)) / (6.0 * math.tan(omega / 2.0)),
                                  np.tan(radius * omega) / (radius * 2.0 * math.tan(omega / 2.0)))
            u, v = u * factor, v * factor
        elif 2 <= model <= 10:
            u, v, iterations = iterative_undistortion(model, p, u, v, extra_iterations=extra_iterations)
            if model == 10:
                theta = np.sqrt(u * u + v * v)
                tc = theta * np.cos(theta)
                scale = np.where(tc > _EPS, np.sin(theta) / np.where(tc > _EPS, tc, 1.0), 1.0)
                u, v = np.where(tc > _EPS, u * scale, u), np.where(tc > _EPS, v * scale, v)
        else:
            raise ValueError("camera model %d does not exist" % model)
    return np.stack([u, v], axis=1), iterations


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the generator: csrc/line_features_replay.hpp in uint64 arithmetic

def _mix(z):
    z = np.asarray(z, dtype=_U64)
    with np.errstate(over="ignore"):
        z = z ^ (z >> _U64(30))
        z = z * _U64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> _U64(27))
        z = z * _U64(0x94D049BB133111EB)
        z = z ^ (z >> _U64(31))
    return z


def image_state(seed, image_id):
    with np.errstate(over="ignore"):
        s = np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=_U64) + _U64(0x9E3779B97F4A7C15)
    return _mix(_mix(s) ^ _U64(int(image_id) & 0xFFFFFFFF))[0]


def _hash(state, index, component):
    index = np.asarray(index, dtype=np.int64).astype(np.uint32).astype(_U64)
    return _mix(_U64(state) ^ ((index << _U64(2)) | _U64(component)))


def draws(seed, image_id, index):
    """the random direction of the features `index` of an image: [N, 3] in [-1, 1)"""
    state = image_state(seed, image_id)
    k = np.stack([(_hash(state, index, c) >> _U64(10)).astype(np.int64) - (1 << 53) for c in range(3)], axis=-1)
    return k.astype(np.float64) * 2.0 ** -53


def align_keys(seed, image_id, index):
    state = image_state(seed, image_id)
    index = np.asarray(index, dtype=np.int64)
    return (_hash(state, index, 3) & _U64(0xFFFFFFFF00000000)) | index.astype(np.uint32).astype(_U64)


def aligned_count(N, ratio):
    """the size the reference's set reaches (extraction.cc:454-458): its loop, literally, on the counts"""
    ratio = float(ratio)
    if not (0.0 <= ratio <= 1.0):
        raise ValueError("aligned_line_ratio %r is outside [0, 1]: the reference's loop would not end" % ratio)
    n, Nd = 0, float(N)
    with np.errstate(all="ignore"):
        while np.float64(n) / np.float64(Nd) < ratio:
            n += 1
    return n


def aligned_flags(seed, image_id, N, ratio, has_gravity=True):
    """[N] bool: the aligned_count features with the smallest key; none without gravity"""
    n = aligned_count(N, ratio) if has_gravity else 0
    if not (0.0 <= float(ratio) <= 1.0):
        raise ValueError("aligned_line_ratio %r is outside [0, 1]" % ratio)
    if n == 0:
        return np.zeros(N, dtype=bool)
    keys = align_keys(seed, image_id, np.arange(N))
    return keys <= np.sort(keys)[n - 1]


# ---------------------------------------------------------------------------------------------------------------------------------------------------

def _batch(images, cameras, keypoints):
    cameras = cameras if isinstance(cameras, dict) else {c.camera_id: c for c in cameras}
    kps = [FeatureKeypointsToPointsVector(keypoints[im.image_id]) for im in images]
    return cameras, kps


def _report(**kw):
    return dict(num_lines=0, num_aligned=0, num_images_without_gravity=0, num_degenerate=0, num_newton_exhausted=0, **kw)


def generate_line_features(images, cameras, keypoints, aligned_line_ratio=DEFAULT_ALIGNED_LINE_RATIO, seed=0, fill=True):
    """The host mirror.  images: bundle_adjustment.Image objects (image_id, camera_id, gravity); cameras: {camera_id: Camera} or a list of Camera;
    keypoints: {image_id: [N, 2+] float32 array or list of FeatureKeypoint}.  Fills image.lines -> report dict with the counts of
    pp_line_features_report and, per image id, `lines` [N, 3], `aligned` [N] bool, `dirs` [N, 3], `uv` [N, 2], `head` [N] (the norm divided by).
    fill=False leaves image.lines alone: the arrays of the report are the result."""
    aligned_count(0, aligned_line_ratio)      # refuses a bad ratio
    cameras, kps = _batch(images, cameras, keypoints)
    rep = _report(lines={}, aligned={}, dirs={}, uv={}, head={}, device_ms=0.0)
    for im, kp in zip(images, kps):
        cam = cameras[im.camera_id]
        if not np.all(np.isfinite(cam.params)):
            raise ValueError("camera %r has a non-finite parameter" % (cam.camera_id,))
        N = len(kp)
        uv, iterations = image_to_world(cam.model_id, cam.params, kp.astype(np.float64))      # float32 -> double: exact
        aligned = aligned_flags(seed, im.image_id, N, aligned_line_ratio, im.HasGravity())
        dirs = draws(seed, im.image_id, np.arange(N)).reshape(N, 3)
        if im.HasGravity():
            dirs[aligned] = np.asarray(im.GravityDirection(), dtype=np.float64)
        u, v = uv[:, 0], uv[:, 1]
        with np.errstate(all="ignore"):
            line = np.stack([dirs[:, 1] - dirs[:, 2] * v, dirs[:, 2] * u - dirs[:, 0], dirs[:, 0] * v - dirs[:, 1] * u], axis=1)
            head = np.sqrt(line[:, 0] * line[:, 0] + line[:, 1] * line[:, 1])
            line = line / head[:, None]
        if fill:
            im.lines = [FeatureLine(line[i], bool(aligned[i]), kInvalidPoint3DId) for i in range(N)]
        k = im.image_id
        rep["lines"][k], rep["aligned"][k], rep["dirs"][k], rep["uv"][k], rep["head"][k] = line, aligned, dirs, uv, head
        rep["num_lines"] += N
        rep["num_aligned"] += int(aligned.sum())
        rep["num_images_without_gravity"] += int(not im.HasGravity())
        rep["num_degenerate"] += int(np.sum(~(head > 0.0) | ~np.isfinite(head)))
        rep["num_newton_exhausted"] += int(np.sum(iterations >= UNDISTORT_MAX_ITERATIONS))
    return rep


def generate_line_features_on_device(images, cameras, keypoints, aligned_line_ratio=DEFAULT_ALIGNED_LINE_RATIO, seed=0, device=0, generator=None, fill=True):
    """generate_line_features through pp_line_features_from_keypoints: the same arguments, the same report (without `uv` and `head`)."""
    from .device import LineFeatureGenerator
    cameras, kps = _batch(images, cameras, keypoints)
    cam_ids = sorted(cameras, key=lambda c: (str(type(c)), c))
    cam_index = {c: i for i, c in enumerate(cam_ids)}
    intr = np.zeros((len(cam_ids), _capi.CAM_STRIDE))
    for c in cam_ids:
        intr[cam_index[c], :len(cameras[c].params)] = cameras[c].params
    kp_start = np.zeros(len(images) + 1, dtype=np.int64)
    kp_start[1:] = np.cumsum([len(k) for k in kps], dtype=np.int64)
    gen = generator or LineFeatureGenerator(device=device)
    out = gen.generate(image_ids=[im.image_id for im in images], kp_start=kp_start,
                       keypoints=np.concatenate(kps) if kps else np.zeros((0, 2), dtype=np.float32),
                       image_camera=[cam_index[im.camera_id] for im in images], camera_model=[cameras[c].model_id for c in cam_ids], intr=intr,
                       has_gravity=[im.HasGravity() for im in images],
                       gravity=[im.GravityDirection() if im.HasGravity() else np.zeros(3) for im in images],
                       aligned_line_ratio=aligned_line_ratio, seed=seed)
    r = out["report"]
    rep = dict(num_lines=int(r.num_lines), num_aligned=int(r.num_aligned), num_images_without_gravity=int(r.num_images_without_gravity),
               num_degenerate=int(r.num_degenerate), num_newton_exhausted=int(r.num_newton_exhausted), device_ms=float(r.device_ms),
               lines={}, aligned={}, dirs={})
    for k, im in enumerate(images):
        a, b = int(kp_start[k]), int(kp_start[k + 1])
        line, aligned = out["lines"][a:b], out["aligned"][a:b].astype(bool)
        if fill:
            im.lines = [FeatureLine(line[i], bool(aligned[i]), kInvalidPoint3DId) for i in range(b - a)]
        rep["lines"][im.image_id], rep["aligned"][im.image_id], rep["dirs"][im.image_id] = line, aligned, out["dirs"][a:b]
    return rep


# ---------------------------------------------------------------------------------------------------------------------------------------------------

class SiftExtractionOptions:
    """feature/sift.h:46-113 with its defaults.  num_threads, use_gpu, gpu_index and max_image_size are carried and not used (one image, one device, the
    caller supplies the array at the size it wants); darkness_adaptivity is ignored as the reference's CPU path ignores it; estimate_affine_shape and
    domain_size_pooling are refused."""
    L1_ROOT, L2 = "L1_ROOT", "L2"
    _FIELDS = dict(num_threads=-1, use_gpu=True, gpu_index="-1", max_image_size=3200, max_num_features=8192, first_octave=-1, num_octaves=4,
                   octave_resolution=3, peak_threshold=None, edge_threshold=10.0, estimate_affine_shape=False, max_num_orientations=2, upright=False,
                   darkness_adaptivity=False, domain_size_pooling=False, dsp_min_scale=1.0 / 6.0, dsp_max_scale=3.0, dsp_num_scales=10,
                   normalization="L1_ROOT")

    def __init__(self, **kw):
        for k in kw:
            if k not in self._FIELDS:
                raise AttributeError(k)
        for k, v in self._FIELDS.items():
            setattr(self, k, kw.get(k, v))
        if self.peak_threshold is None:
            self.peak_threshold = 0.02 / self.octave_resolution if self.octave_resolution > 0 else 0.02 / 3      # (Check() refuses the resolution)

    def Check(self):
        """SiftExtractionOptions::Check (sift.cc:371-387)"""
        ok = self.max_image_size > 0 and self.max_num_features > 0 and self.octave_resolution > 0 and self.peak_threshold > 0.0
        ok = ok and self.edge_threshold > 0.0 and self.max_num_orientations > 0
        if self.domain_size_pooling:
            ok = ok and self.dsp_min_scale > 0 and self.dsp_max_scale >= self.dsp_min_scale and self.dsp_num_scales > 0
        return bool(ok)

    def device_options(self, phase_timings=False):
        """-> pp_sift_extract_options"""
        from .device import sift_extract_options
        if self.estimate_affine_shape or self.domain_size_pooling:
            raise ValueError("estimate_affine_shape and domain_size_pooling belong to the covariant extractor, which is absent")
        if self.normalization not in (self.L1_ROOT, self.L2):
            raise ValueError("normalization is L1_ROOT or L2")
        return sift_extract_options(max_num_features=int(self.max_num_features), first_octave=int(self.first_octave), num_octaves=int(self.num_octaves),
                                    octave_resolution=int(self.octave_resolution), peak_threshold=float(self.peak_threshold),
                                    edge_threshold=float(self.edge_threshold), max_num_orientations=int(self.max_num_orientations),
                                    upright=int(bool(self.upright)), normalization=_capi.SIFT_L2 if self.normalization == self.L2 else _capi.SIFT_L1_ROOT,
                                    phase_timings=int(bool(phase_timings)))


def ExtractSiftFeatures(image_uint8, options=None, device=0, extractor=None, as_arrays=False):
    """ExtractSiftFeaturesCPU for one grey image on the device -> (FeatureKeypoints: a list of FeatureKeypoint, descriptors [N, 128] uint8 in UBC order).
    as_arrays: the keypoints as the [N, 4] float32 array (x, y, scale, orientation) the device returns.  extractor: a device.SiftExtractor to reuse."""
    from .device import SiftExtractor
    options = options or SiftExtractionOptions()
    if not options.Check():
        raise ValueError("SiftExtractionOptions.Check() failed")
    o = options.device_options()
    ex = extractor or SiftExtractor(device=device)
    try:
        kp, desc, _ = ex.extract(image_uint8, o)
    finally:
        if extractor is None:
            ex.close()
    if as_arrays:
        return kp, desc
    return [FeatureKeypoint(r[0], r[1], r[2], r[3]) for r in kp], desc


def ExtractSiftFeaturesBatch(images_uint8, options=None, device=0, extractor=None, as_arrays=False):
    """ExtractSiftFeatures for a sequence of grey images of any sizes in one device call (SiftExtractor.extract_batch) -> a list of what
    ExtractSiftFeatures returns, image by image, with the same values."""
    from .device import SiftExtractor
    options = options or SiftExtractionOptions()
    if not options.Check():
        raise ValueError("SiftExtractionOptions.Check() failed")
    o = options.device_options()
    ex = extractor or SiftExtractor(device=device)
    try:
        results = ex.extract_batch(images_uint8, o)
    finally:
        if extractor is None:
            ex.close()
    if as_arrays:
        return [(kp, desc) for kp, desc, _ in results]
    return [([FeatureKeypoint(r[0], r[1], r[2], r[3]) for r in kp], desc) for kp, desc, _ in results]


def extract_features_to_lines(images, cameras, bitmaps, options=None, aligned_line_ratio=DEFAULT_ALIGNED_LINE_RATIO, seed=0, device=0, batched=True,
                              to_matcher=False):
    """Image arrays to what the matcher and the graph builder take.  images: bundle_adjustment.Image objects; cameras as for generate_line_features;
    bitmaps: {image_id: [H, W] uint8}.  ExtractSiftFeaturesBatch over the images (batched=False: ExtractSiftFeatures image by image - the same arrays),
    then generate_line_features_on_device over all of them (it fills image.lines).
    -> dict(keypoints {image_id: [N, 4] float32}, descriptors {image_id: [N, 128] uint8}, num_lines {image_id: N}, lines: the line report).
    Line index = keypoint index = descriptor row.
    to_matcher: the descriptors stay on the device (SiftExtractor.extract_to_matcher) and the dict holds matcher=, a feature_matching.FeatureMatcher
    over the images' ids under the default SiftMatchingOptions (the caller closes it), in place of descriptors=."""
    from .device import SiftExtractor
    ex = SiftExtractor(device=device)
    keypoints, descriptors, sift_matcher = {}, {}, None
    try:
        if to_matcher:
            options = options or SiftExtractionOptions()
            if not options.Check():
                raise ValueError("SiftExtractionOptions.Check() failed")
            found, _, _, sift_matcher = ex.extract_to_matcher([bitmaps[im.image_id] for im in images], options.device_options())
            for im, kp in zip(images, found):
                keypoints[im.image_id] = kp
        elif batched and len(images) > 0:
            found = ExtractSiftFeaturesBatch([bitmaps[im.image_id] for im in images], options, extractor=ex, as_arrays=True)
            for im, (kp, desc) in zip(images, found):
                keypoints[im.image_id], descriptors[im.image_id] = kp, desc
        else:
            for im in images:
                keypoints[im.image_id], descriptors[im.image_id] = ExtractSiftFeatures(bitmaps[im.image_id], options, extractor=ex, as_arrays=True)
    finally:
        ex.close()
    if not to_matcher:
        rep = generate_line_features_on_device(images, cameras, keypoints, aligned_line_ratio=aligned_line_ratio, seed=seed, device=device)
        return dict(keypoints=keypoints, descriptors=descriptors, num_lines={k: len(v) for k, v in keypoints.items()}, lines=rep)
    from .feature_matching import FeatureMatcher, SiftMatchingOptions
    try:
        rep = generate_line_features_on_device(images, cameras, keypoints, aligned_line_ratio=aligned_line_ratio, seed=seed, device=device)
        matcher = FeatureMatcher.from_matcher(SiftMatchingOptions(), [im.image_id for im in images], sift_matcher, device=device)
    except Exception:
        sift_matcher.close()
        raise
    return dict(keypoints=keypoints, matcher=matcher, num_lines={k: len(v) for k, v in keypoints.items()}, lines=rep)
