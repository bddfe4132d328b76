"""CPU-only checks of the C ABI of K24 (pp_sift_extract_to_matcher, pp_sift_get_descriptors): the symbols are exported and declared, and every
argument pp_sift_extract_batch refuses is refused here as well - PP_ERR_INVALID, an error code and not an abort, before a handle is read, with the
outputs untouched and *matcher NULL.  Everything that needs a device runs in tests/test_gpu_sift_extract_to_matcher.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from privacy_preserving_sfm_amd import _capi, device, feature_extraction as fe
from test_sift_extract_capi_host import BAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["pp_sift_extract_to_matcher", "pp_sift_get_descriptors"]
BOGUS = C.c_void_p(1)      # never dereferenced: every case below is refused on the other arguments first
STALE = 0x5A5A      # what *matcher holds before a call


def test_the_symbols_are_exported_and_declared():
    L = _capi.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppsfm_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert name in _capi.exported_symbols() and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, text), name


class _Call:
    """the arguments of one call, pre-filled so that a write shows"""

    def __init__(self, sizes=((16, 12), (16, 12), (16, 12))):
        self.n = len(sizes)
        self.greys = [np.zeros(max(w * h, 1) if 0 < w * h < 1 << 20 else 1, dtype=np.uint8) for w, h in sizes]
        self.images = (_capi.SiftBatchImage * self.n)()
        for i, (w, h) in enumerate(sizes):
            self.images[i].width, self.images[i].height, self.images[i].grey = w, h, _capi.ptr(self.greys[i], _capi.c_u8p)
        self.options = device.sift_extract_options()
        self.batch_report = _capi.SiftBatchReport()
        self.reports = (_capi.SiftExtractReport * self.n)()
        for r in self.reports:
            r.num_features = 77
        self.kp = np.full((4, 4), 7.0, dtype=np.float32)
        self.offsets = np.full(self.n + 1, -5, dtype=np.int64)
        self.matcher = C.c_void_p(STALE)
        self.capacity, self.workspace_bytes, self.num_images, self.handle = 4, 0, self.n, BOGUS

    def run(self, **replaced):
        a = dict(h=self.handle, options=C.byref(self.options), num_images=self.num_images, images=self.images, workspace_bytes=self.workspace_bytes,
                 batch_report=C.byref(self.batch_report), reports=self.reports, capacity=self.capacity, keypoints=_capi.ptr(self.kp, C.POINTER(C.c_float)),
                 offsets=_capi.ptr(self.offsets, C.POINTER(C.c_int64)), matcher=C.byref(self.matcher))
        a.update(replaced)
        return _capi.lib().pp_sift_extract_to_matcher(*[a[k] for k in ("h", "options", "num_images", "images", "workspace_bytes", "batch_report", "reports", "capacity",
                                                                       "keypoints", "offsets", "matcher")])

    def untouched(self):
        return (all(r.num_features == 77 for r in self.reports) and np.all(self.offsets == -5) and np.all(self.kp == 7.0)
                and self.batch_report.num_images == 0)


def test_null_arguments_and_bad_counts_are_refused_before_a_handle_is_read():
    L = _capi.lib()
    for name in ("options", "images", "batch_report", "reports", "keypoints", "offsets"):
        c = _Call()
        assert c.run(**{name: None}) == _capi.PP_ERR_INVALID, name
        assert b"pp_sift_extract_to_matcher" in L.pp_last_error()
        assert c.untouched() and c.matcher.value is None, name
    c = _Call()
    assert c.run(matcher=None) == _capi.PP_ERR_INVALID and c.untouched() and c.matcher.value == STALE      # nowhere to put the handle
    c = _Call()
    c.images[1].grey = None      # a null image
    assert c.run() == _capi.PP_ERR_INVALID and b"image 1" in L.pp_last_error() and c.untouched() and c.matcher.value is None
    for field, value in (("num_images", 0), ("num_images", -1), ("capacity", -1), ("workspace_bytes", -1)):
        c = _Call()
        setattr(c, field, value)
        assert c.run() == _capi.PP_ERR_INVALID, (field, value)
        assert c.untouched() and c.matcher.value is None, (field, value)
    c = _Call()
    assert c.run(h=None) == _capi.PP_ERR_INVALID      # good arguments, no handle
    assert b"null handle" in L.pp_last_error() and c.untouched() and c.matcher.value is None


@pytest.mark.parametrize("field,value", BAD)
def test_bad_options_are_refused(field, value):
    c = _Call()
    c.options = device.sift_extract_options(**{field: value})
    assert c.run() == _capi.PP_ERR_INVALID      # before the handle is read
    assert c.untouched() and c.matcher.value is None


@pytest.mark.parametrize("w,h", [(0, 12), (16, -3), (20000, 14000), (2 ** 20, 2)])
def test_a_bad_size_names_its_image(w, h):
    c = _Call(sizes=((16, 12), (16, 12), (w, h)))
    assert c.run() == _capi.PP_ERR_INVALID
    message = _capi.lib().pp_last_error()
    assert b"image 2" in message and b"image 0" not in message and b"image 1" not in message, message
    assert c.untouched() and c.matcher.value is None


def test_the_descriptor_reader_refuses_a_null_handle():
    L = _capi.lib()
    out, num = np.full((2, 128), 9, dtype=np.uint8), C.c_int64(-5)
    assert L.pp_sift_get_descriptors(None, 0, _capi.ptr(out, _capi.c_u8p), 2, C.byref(num)) == _capi.PP_ERR_INVALID
    assert b"pp_sift_get_descriptors" in L.pp_last_error() and num.value == -5 and np.all(out == 9)
    assert L.pp_sift_get_descriptors(BOGUS, 0, _capi.ptr(out, _capi.c_u8p), 2, None) == _capi.PP_ERR_INVALID      # (refused before the handle is read)


def test_no_cpu_path_without_a_device():
    n = C.c_int()
    _capi.lib().pp_device_count(C.byref(n))
    if n.value:
        return      # (tests/test_gpu_sift_extract_to_matcher.py runs the calls)
    with pytest.raises(_capi.PPError) as e:
        device.SiftExtractor()
    assert e.value.code == _capi.PP_ERR_HIP
    with pytest.raises(_capi.PPError) as e:
        device.SiftMatcher([np.zeros((3, 128), dtype=np.uint8)])
    assert e.value.code == _capi.PP_ERR_HIP
    with pytest.raises(_capi.PPError) as e:
        fe.extract_features_to_lines([], {}, {}, to_matcher=True)
    assert e.value.code == _capi.PP_ERR_HIP
