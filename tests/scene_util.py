"""TEST INFRASTRUCTURE ONLY: pictures for the scene tests and the emulated kernels (tests/scene_emul/libscene_emul.so: the SOURCE of
turbo-metrics_amd/csrc/tm_scene_kernels.h run lane by lane on the CPU).  The plane arrays of the four layouts come from
tests/motion_util.luma_plane, dirty bits included."""
import ctypes as C
import os
import subprocess

import numpy as np

from tm_pkg import tm
from tests import motion_util

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_EMUL_DIR = os.path.join(_HERE, "scene_emul")
_EMUL_LIB = os.path.join(_EMUL_DIR, "libscene_emul.so")
_EMUL_SRCS = [os.path.join(_EMUL_DIR, "scene_emul.cpp"), os.path.join(_HERE, "emul", "hip_emul.h")] + [
    os.path.join(_ROOT, "turbo-metrics_amd", "csrc", f) for f in ("tm_scene_kernels.h", "tm_sample_load.h", "tm_p10.h", "tm_platform.h", "tm_geom.h")]
LAYOUT = tm.scene.LAYOUTS
CASES = motion_util.CASES
luma_plane = motion_util.luma_plane
KINDS = ("noise", "smooth", "extreme", "flat")


def picture(w, h, bits, kind, seed=0):
    """one luma plane of sample values (int64, depth `bits`):
      noise    independent uniform samples over the whole range
      smooth   a gradient plus a little noise
      extreme  every sample 0 or 2^D - 1 at random
      flat     one value everywhere (the value depends on the seed)"""
    rng = np.random.default_rng([0x5CE7E, seed, w, h, bits])
    M = (1 << bits) - 1
    if kind == "noise":
        p = rng.integers(0, M + 1, (h, w), dtype=np.int64)
    elif kind == "extreme":
        p = rng.integers(0, 2, (h, w), dtype=np.int64) * M
    elif kind == "flat":
        p = np.full((h, w), int(rng.integers(0, M + 1)), np.int64)
    elif kind == "smooth":
        y, x = np.indices((h, w))
        p = ((x * 7 + y * 3 + seed * 11) * max(1, M // 255) + rng.integers(0, max(1, M // 32), (h, w))) % (M + 1)
    else:
        raise ValueError(kind)
    return p.astype(np.int64)


def build_emul():
    if os.path.exists(_EMUL_LIB) and all(os.path.getmtime(s) <= os.path.getmtime(_EMUL_LIB) for s in _EMUL_SRCS):
        return _EMUL_LIB
    # the flags tests/emul/emul.py builds the engine's emulated kernels with
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-pthread",
                           "-Wno-unknown-pragmas", "-I", os.path.join(_HERE, "emul"), "-o", _EMUL_LIB, _EMUL_SRCS[0]])
    return _EMUL_LIB


class _Desc(C.Structure):
    _fields_ = [("p", C.c_void_p), ("pitch", C.c_ulonglong), ("vec", C.c_int), ("pad_", C.c_int)]


def bands(w, h, layout, bits):
    """workgroups per picture of this geometry (0: refused)"""
    return int(C.CDLL(build_emul()).se_bands(w, h, LAYOUT.get(layout, layout), bits))


def emulate(w, h, layout, bits, batches, planes, cap=None, vec=None):
    """the emulated kernels over plane arrays (luma_plane): compute c takes the next batches[c] planes as its slots 0 .. batches[c]-1
    of ONE library object with `cap` slots (default: the largest batch), whose buffers are reused from compute to compute.
    vec=False: the sample-by-sample path everywhere.  -> one uint32[256] per plane, or None for a geometry the library refuses"""
    L = C.CDLL(build_emul())
    assert L.se_desc_size() == C.sizeof(_Desc)
    n = len(planes)
    assert sum(batches) == n
    desc = (_Desc * n)()
    keep = []
    for f, p in enumerate(planes):
        if p.strides[1] != p.itemsize:
            p = np.ascontiguousarray(p)
        keep.append(p)
        desc[f].p, desc[f].pitch = p.ctypes.data, p.strides[0]
    out = np.zeros((n, 256), np.uint32)
    bt = (C.c_int * len(batches))(*batches)
    rc = L.se_run(w, h, LAYOUT.get(layout, layout), bits, cap or max(batches), len(batches), bt, desc, -1 if vec is None else int(bool(vec)),
                  out.ctypes.data_as(C.c_void_p))
    if rc == -1:
        return None
    assert rc == 0, rc
    return [out[i].copy() for i in range(n)]


def aligned_copy(p, pad_elems=0):
    """the same plane in memory whose base and pitch are 16-byte aligned (the wide-load path), rows padded with garbage"""
    rows, cols = p.shape
    pitch = ((cols + pad_elems) * p.itemsize + 15) // 16 * 16 // p.itemsize
    raw = np.empty(rows * pitch * p.itemsize + 16, np.uint8)
    raw[:] = np.random.default_rng(7).integers(0, 256, raw.size, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    buf = raw[off:off + rows * pitch * p.itemsize].view(p.dtype).reshape(rows, pitch)
    buf[:, :cols] = p
    return buf[:, :cols]
