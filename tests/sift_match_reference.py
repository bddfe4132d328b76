"""The rule of MatchSiftFeaturesCPUBruteForce (reference src/feature/sift.cc:54-143, 170-203, 957-970) in plain Python / numpy, the yardstick of the
K17 tests.  The products are an int64 matrix product.  The two float rules are evaluated in float32 with acosf taken from THIS PROCESS's libm through
ctypes - never numpy's arccos, which rounds differently from glibc's acosf on a third of the integers around the distance threshold and would decide
boundary cases differently from the reference on the same host.  Helper module, not a test."""
import ctypes
import ctypes.util
import functools

import numpy as np

CLAMP = 512 * 512
MAX_DIST = 128 * 255 * 255


def _libm():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.acosf.restype = ctypes.c_float
    m.acosf.argtypes = [ctypes.c_float]
    return m


@functools.lru_cache(maxsize=None)
def angles():
    """a(d) = acosf(min(kDistNorm * d, 1.0f)) for d = 0 .. 262144, float32 (a(d) = a(262144) = 0 beyond)"""
    acosf = _libm().acosf
    k = np.float32(1.0) / (np.float32(512.0) * np.float32(512.0))
    x = np.minimum(k * np.arange(CLAMP + 1, dtype=np.float32), np.float32(1.0))      # exact: a power of two times an integer below 2^24
    a = np.array([acosf(float(v)) for v in x], dtype=np.float32)
    a.setflags(write=False)
    return a


def angle(d):
    return angles()[np.minimum(np.asarray(d, dtype=np.int64), CLAMP)]


def accept(best, second, max_ratio=0.8, max_distance=0.7):
    """the two rules of :84-99 as the reference states them, element-wise, for best >= 1"""
    r, d = np.float32(max_ratio), np.float32(max_distance)
    ab, asec = angle(best), angle(second)
    rejected = (ab > d) | (ab >= r * asec)      # float32 * float32 -> float32, one rounding, as in C
    return ~rejected


def dist_matrix(d1, d2):
    return np.asarray(d1, dtype=np.int64).reshape(-1, 128) @ np.asarray(d2, dtype=np.int64).reshape(-1, 128).T


def top2(dists):
    """-> (best_j, best, second) int32 per row, order-free: the maximum, the lowest index that attains it (-1 when no dist is positive), the second
    largest value with multiplicity"""
    n1, n2 = dists.shape
    if n2 == 0:
        return np.full(n1, -1, dtype=np.int32), np.zeros(n1, dtype=np.int32), np.zeros(n1, dtype=np.int32)
    best = dists.max(axis=1)
    best_j = np.where(best > 0, dists.argmax(axis=1), -1)      # (argmax: the first occurrence)
    second = np.sort(dists, axis=1)[:, -2] if n2 >= 2 else np.zeros(n1, dtype=np.int64)
    return best_j.astype(np.int32), best.astype(np.int32), second.astype(np.int32)


def top2_sequential(dists):
    """the scan as :64-77 writes it (slow; the cross-check of top2 on small inputs)"""
    out = []
    for row in dists:
        bj, b, s = -1, 0, 0
        for j, d in enumerate(row):
            if d > b:
                bj, s, b = j, b, d
            elif d > s:
                s = d
        out.append((bj, b, s))
    a = np.array(out, dtype=np.int32).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2]


def one_way(dists, max_ratio=0.8, max_distance=0.7):
    """-> m [n1]: the match of every row or -1"""
    bj, b, s = top2(dists)
    ok = (bj >= 0) & accept(np.maximum(b, 1), s, max_ratio, max_distance)
    return np.where(ok, bj, -1).astype(np.int32)


def match(d1, d2, max_ratio=0.8, max_distance=0.7, cross_check=True):
    """FindBestMatchesBruteForce: -> [n, 2] int32, ascending in the first column"""
    dists = dist_matrix(d1, d2)
    m12 = one_way(dists, max_ratio, max_distance)
    keep = m12 >= 0
    if cross_check:
        m21 = one_way(dists.T, max_ratio, max_distance)
        keep = keep & (m21[np.maximum(m12, 0)] == np.arange(len(m12))) if len(m21) else np.zeros(len(m12), dtype=bool)
    i = np.flatnonzero(keep)
    return np.stack([i, m12[i]], axis=1).astype(np.int32).reshape(-1, 2)


def match_pair_rule(d1, d2, min_num_matches=15, **kw):
    """with the pair rule of SiftFeatureMatcher::Match (feature/matching.cc:414-416)"""
    m = match(d1, d2, **kw)
    return m if len(m) >= min_num_matches else np.zeros((0, 2), dtype=np.int32)


def thresholds(max_ratio=0.8, max_distance=0.7):
    """-> (d_min, table): the distance rule passes iff best >= d_min, the ratio rule iff min(second, CLAMP) <= table[min(best, CLAMP) - d_min] (-1: never).
    Straight from the definitions: for every best the largest second that passes, found by evaluating the rule, not by assuming how it was built."""
    a = angles()
    r = np.float32(max_ratio) * a
    assert np.all(np.diff(a) <= 0) and np.all(np.diff(r) <= 0)      # what makes thresholds possible at all
    passes = np.flatnonzero(~(a > np.float32(max_distance)))
    d_min = int(passes[0])
    # seconds s with a(b) < r(s): r is non-increasing, so they are a prefix; its length by binary search on the reversed (ascending) array
    asc = r[::-1]
    count = len(r) - np.searchsorted(asc, a[d_min:], side="right")
    return d_min, (count - 1).astype(np.int32)
