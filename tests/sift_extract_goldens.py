"""The recorded reference of SIFT extraction (tests/golden/sift, see its README.md) and what the tests of K21 share: the cases, the parser of the
host driver's dump, the comparison of a result with a recording, and the project's rule for the last normalisation restated in numpy."""
import hashlib
import json
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sift")
OPTION_ORDER = ("max_num_features", "first_octave", "num_octaves", "octave_resolution", "peak_threshold", "edge_threshold", "max_num_orientations",
                "upright", "normalization")

_listing = json.load(open(os.path.join(GOLDEN, "cases.json")))
CASES = _listing["cases"]
CASE_NAMES = [c["name"] for c in CASES]
CHAIN = _listing["chain"]
_recordings = {}


def case(name):
    return CASES[CASE_NAMES.index(name)]


def image(c):
    return np.fromfile(os.path.join(GOLDEN, c["image"]), dtype=np.uint8).reshape(c["height"], c["width"])


def recording(c):
    """the arrays recorded from the reference for the case's scale space and features (shared, read once, never changed)"""
    stem = c["golden"]
    if stem not in _recordings:
        with np.load(os.path.join(GOLDEN, stem + ".npz")) as z:
            _recordings[stem] = {k: z[k] for k in z.files}
        for a in _recordings[stem].values():
            a.setflags(write=False)
    return _recordings[stem]


def option_words(o):
    """the options as the host driver reads them"""
    return " ".join(float(o[k]).hex() if k.endswith("threshold") else str(int(o[k])) for k in OPTION_ORDER)


def parse_dump(path):
    """{name: bytes} of the records the host driver wrote"""
    b = open(path, "rb").read()
    p, out = 0, {}
    while p < len(b):
        n, = struct.unpack_from("<I", b, p)
        name = b[p + 4:p + 4 + n].decode()
        e, c = struct.unpack_from("<IQ", b, p + 4 + n)
        p += 16 + n
        out[name] = b[p:p + e * c]
        p += e * c
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    differing = int(np.count_nonzero(bits(got) != bits(want)))
    assert differing == 0, "%s: %d of %d values differ" % (what, differing, want.size)


def check_stage(rec, name, level, sampled):
    """one Gaussian / DoG / gradient level ([h, w] or [h, w, 2] float32) against its recorded digest and rows"""
    names = list(rec["stage_names"])
    level = np.ascontiguousarray(level, dtype=np.float32)
    rows = level.reshape(level.shape[0], -1)
    if "rows|" + name in rec:
        h = rows.shape[0]
        assert_same_bits(rows[[h // 3, h - 1]], rec["rows|" + name], name + " (sampled rows)")
    else:
        assert not sampled
    assert hashlib.sha256(level.tobytes()).hexdigest() == str(rec["stage_sha256"][names.index(name)]), name


def stage_names(rec):
    """(name, kind, octave, level) of every recorded level"""
    out = []
    for n in rec["stage_names"]:
        kind, o, s = str(n).split()
        out.append((str(n), kind, int(o), int(s)))
    return out


def sequential_sum(a):
    """the float32 sum over the last axis from the first entry to the last, one addition per entry"""
    acc = np.zeros(a.shape[:-1], dtype=np.float32)
    for k in range(a.shape[-1]):
        acc = (acc + a[..., k]).astype(np.float32)
    return acc


def finish_descriptors(raw, normalization):
    """The project's rule for the reference's last steps (sift.cc:509-520 and 569): raw [N, 128] float32 in VLFeat's order -> [N, 128] uint8 in UBC
    order.  L1-root (0): v / sum |v|, then the square root; L2 (1): v / sqrt(sum v^2); the sums sequential in float32; round(512 v) cut to 255; a zero
    norm gives zeros."""
    raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1, 128)
    if normalization == 0:
        norm = sequential_sum(np.abs(raw))
    else:
        norm = np.sqrt(sequential_sum((raw * raw).astype(np.float32))).astype(np.float32)
    with np.errstate(all="ignore"):
        v = (raw / norm[:, None]).astype(np.float32)
        if normalization == 0:
            v = np.sqrt(v).astype(np.float32)
    v[~(norm > 0)] = 0
    x = (np.float32(512.0) * v).astype(np.float32)
    t = np.trunc(x)
    scaled = np.where(x - t >= np.float32(0.5), t + 1, t)
    vl = np.minimum(scaled, 255).astype(np.uint8)
    q = np.array([0, 7, 6, 5, 4, 3, 2, 1])
    ubc = np.zeros_like(vl)
    for k in range(8):
        ubc[:, q[k]::8] = vl[:, k::8]
    return ubc


def check_result(c, keypoints, descriptors, all_raw, all_octave_level, all_angles, first_level_to_keep):
    """What an extraction of case c returned (the kept features) and found (every feature before the cut) against the recording, with no tolerance."""
    rec = recording(c)
    first, start, count = c["cut"]
    assert first_level_to_keep == first
    assert_same_bits(np.asarray(all_octave_level, dtype=np.int32).reshape(-1, 2), rec["octave_level"], "(octave, level) per feature")
    assert_same_bits(np.asarray(all_angles, dtype=np.float64), rec["angles"], "angles")
    assert_same_bits(np.asarray(all_raw, dtype=np.float32).reshape(-1, 128), rec["raw"], "raw descriptors")
    assert start + count == len(rec["keypoints"])
    assert_same_bits(np.asarray(keypoints, dtype=np.float32).reshape(-1, 4), rec["keypoints"][start:start + count], "keypoints")
    want = finish_descriptors(rec["raw"], c["options"]["normalization"])[start:start + count]
    assert np.array_equal(np.asarray(descriptors, dtype=np.uint8).reshape(-1, 128), want), "uint8 descriptors"
