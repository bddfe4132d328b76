"""CPU-only checks of the C ABI of K23 (pp_sift_extract_batch, pp_sift_extract_batch_features): the symbols are exported and declared, the two structs
have the layout the header states, and null arguments, bad counts, every option and every size the check refuses are PP_ERR_INVALID - an error code,
not an abort - before a handle is read and with the outputs untouched; the message names the offending image.  Everything that needs a device runs in
tests/test_gpu_sift_extract_batch.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from privacy_preserving_sfm_amd import _capi, device, feature_extraction as fe
from test_sift_extract_capi_host import BAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["pp_sift_extract_batch", "pp_sift_extract_batch_features"]
BOGUS = C.c_void_p(1)      # never dereferenced: every case below is refused on the other arguments first


def test_the_symbols_are_exported_and_declared():
    L = _capi.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppsfm_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert name in _capi.exported_symbols() and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert "pp_sift_batch_image" in text and "pp_sift_batch_report" in text


def test_the_struct_sizes_and_offsets_match_the_header():
    assert C.sizeof(_capi.SiftBatchImage) == 16
    assert (_capi.SiftBatchImage.width.offset, _capi.SiftBatchImage.height.offset, _capi.SiftBatchImage.grey.offset) == (0, 4, 8)
    R = _capi.SiftBatchReport
    assert C.sizeof(R) == 2 * 4 + 2 * 8 + 7 * 8
    assert (R.num_images.offset, R.num_sub_batches.offset, R.num_features.offset, R.workspace_bytes.offset) == (0, 4, 8, 16)
    assert (R.phase_ms.offset, R.device_ms.offset, R.total_ms.offset) == (24, 64, 72)


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
        self.desc = np.full((4, 128), 9, dtype=np.uint8)
        self.offsets = np.full(self.n + 1, -5, dtype=np.int64)
        self.capacity, self.workspace_bytes, self.num_images, self.handle = 4, 0, self.n, BOGUS

    def args(self, **none):
        a = dict(h=self.handle, options=C.byref(self.options), num_images=self.num_images, images=self.images, workspace_bytes=self.workspace_bytes,
                 batch_report=C.byref(self.batch_report), reports=self.reports, capacity=self.capacity, keypoints=_capi.ptr(self.kp, C.POINTER(C.c_float)),
                 descriptors=_capi.ptr(self.desc, _capi.c_u8p), offsets=_capi.ptr(self.offsets, C.POINTER(C.c_int64)))
        a.update(none)
        return [a[k] for k in ("h", "options", "num_images", "images", "workspace_bytes", "batch_report", "reports", "capacity", "keypoints", "descriptors", "offsets")]

    def run(self, **none):
        return _capi.lib().pp_sift_extract_batch(*self.args(**none))

    def untouched(self):
        return (all(r.num_features == 77 for r in self.reports) and np.all(self.offsets == -5) and np.all(self.kp == 7.0) and np.all(self.desc == 9)
                and self.batch_report.num_images == 0)


def test_null_arguments_and_bad_counts_are_refused_before_a_handle_is_read():
    L = _capi.lib()
    for name in ("options", "images", "batch_report", "reports", "keypoints", "offsets"):
        c = _Call()
        assert c.run(**{name: None}) == _capi.PP_ERR_INVALID, name
        assert b"pp_sift_extract_batch" in L.pp_last_error()
        assert c.untouched(), name
    c = _Call()
    c.images[1].grey = None      # a null image
    assert c.run() == _capi.PP_ERR_INVALID and b"image 1" in L.pp_last_error() and c.untouched()
    for field, value in (("num_images", 0), ("num_images", -1), ("capacity", -1), ("workspace_bytes", -1)):
        c = _Call()
        setattr(c, field, value)
        assert c.run() == _capi.PP_ERR_INVALID, (field, value)
        assert c.untouched(), (field, value)
    c = _Call()
    assert c.run(h=None, descriptors=None) == _capi.PP_ERR_INVALID      # good arguments, no handle
    assert b"null handle" in L.pp_last_error() and c.untouched()
    num = C.c_int64(-5)
    assert L.pp_sift_extract_batch_features(None, 0, None, None, None, 0, C.byref(num)) == _capi.PP_ERR_INVALID and num.value == -5


@pytest.mark.parametrize("field,value", BAD)
def test_bad_options_are_refused(field, value):
    c = _Call()
    c.options = device.sift_extract_options(**{field: value})
    assert c.run() == _capi.PP_ERR_INVALID      # before the handle is read
    assert c.untouched()


@pytest.mark.parametrize("w,h", [(0, 12), (16, -3), (20000, 14000), (2 ** 20, 2)])
def test_a_bad_size_names_its_image(w, h):
    c = _Call(sizes=((16, 12), (16, 12), (w, h)))
    assert c.run() == _capi.PP_ERR_INVALID
    message = _capi.lib().pp_last_error()
    assert b"image 2" in message and b"image 0" not in message and b"image 1" not in message, message
    assert c.untouched()


def test_no_cpu_path_without_a_device():
    n = C.c_int()
    _capi.lib().pp_device_count(C.byref(n))
    if n.value:
        return      # (tests/test_gpu_sift_extract_batch.py runs the calls)
    with pytest.raises(_capi.PPError) as e:
        device.SiftExtractor()
    assert e.value.code == _capi.PP_ERR_HIP
    with pytest.raises(_capi.PPError):
        fe.ExtractSiftFeaturesBatch([np.zeros((16, 16), dtype=np.uint8)])
