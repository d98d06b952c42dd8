"""TEST INFRASTRUCTURE ONLY: the luma planes of the motion tests in the four layouts of include/turbo_metrics_motion.h, and the
emulated kernel (tests/motion_emul/libmotion_emul.so: the SOURCE of turbo-metrics_amd/csrc/tm_motion_kernels.h run lane by lane on
the CPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tm_pkg import tm
from tests import xpsnr_util

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_EMUL_DIR = os.path.join(_HERE, "motion_emul")
_EMUL_LIB = os.path.join(_EMUL_DIR, "libmotion_emul.so")
_EMUL_SRCS = [os.path.join(_EMUL_DIR, "motion_emul.cpp"), os.path.join(_HERE, "emul", "hip_emul.h")] + [
    os.path.join(_ROOT, "turbo-metrics_amd", "csrc", f) for f in ("tm_motion_kernels.h", "tm_sample_load.h", "tm_p10.h", "tm_platform.h", "tm_geom.h")]
LAYOUT = tm.motion.LAYOUTS
# the luma plane of each motion layout is the first plane of one of the XPSNR test layouts
_XPSNR_LAYOUT = {"y8": "nv12", "y16_msb": "p016", "y16_low": "i420", "y10_packed": "i420p10"}
CASES = (("y8", 8), ("y16_msb", 10), ("y16_msb", 12), ("y16_msb", 16), ("y16_low", 10), ("y16_low", 12), ("y16_low", 16), ("y10_packed", 10))


def sequence(w, h, n, bits, kind="random", seed=0):
    """n luma planes (int64 sample values of depth `bits`):
      random   independent uniform samples over the whole range
      smooth   a drifting gradient plus a little noise (what a real picture looks like to a low-pass)
      extreme  every sample 0 or 2^D - 1 at random"""
    rng = np.random.default_rng([0x307104, seed, w, h, bits])
    M = (1 << bits) - 1
    out = []
    for i in range(n):
        if kind == "random":
            p = rng.integers(0, M + 1, (h, w), dtype=np.int64)
        elif kind == "extreme":
            p = rng.integers(0, 2, (h, w), dtype=np.int64) * M
        else:
            y, x = np.indices((h, w))
            p = ((x * 7 + y * 3 + i * 11) * (M // 255) + rng.integers(0, max(1, M // 32), (h, w))) % (M + 1)
        out.append(p.astype(np.int64))
    return out


def luma_plane(layout, Y, bits, pad=0, dirty=None):
    """sample values -> the plane array of `layout` (rows padded by `pad` elements); dirty=<seed> fills every bit the kernel must
    ignore with garbage: tests/xpsnr_util.layout_planes"""
    h, w = Y.shape
    cw, ch = (w + 1) // 2, (h + 1) // 2
    z = np.zeros((ch, cw), np.int64)
    return xpsnr_util.layout_planes(_XPSNR_LAYOUT[layout], (Y, z, z), w, h, bits, pad=pad, dirty=dirty)[0]


def build_emul():
    if os.path.exists(_EMUL_LIB) and all(os.path.getmtime(s) <= os.path.getmtime(_EMUL_LIB) for s in _EMUL_SRCS):
        return _EMUL_LIB
    # the flags tests/emul/emul.py builds the engine's emulated kernels with
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-pthread",
                           "-Wno-unknown-pragmas", "-I", os.path.join(_HERE, "emul"), "-o", _EMUL_LIB, _EMUL_SRCS[0]])
    return _EMUL_LIB


class _Desc(C.Structure):
    _fields_ = [("p", C.c_void_p), ("pitch", C.c_ulonglong), ("vec", C.c_int), ("pad_", C.c_int)]


def emulate(w, h, layout, bits, batches, planes, want_blur=False):
    """the emulated kernel over a sequence of plane arrays (luma_plane), split into launches of `batches` slots (a negative entry: a
    reset, then a batch of that many); -> [sad] per picture (and the last blurred plane), or None for a geometry the library refuses"""
    L = C.CDLL(build_emul())
    assert L.me_desc_size() == C.sizeof(_Desc)
    n = len(planes)
    assert sum(abs(b) for b in batches) == n
    desc = (_Desc * n)()
    keep = []
    for f, p in enumerate(planes):
        if not p.flags["C_CONTIGUOUS"] and p.strides[1] != p.itemsize:
            p = np.ascontiguousarray(p)
        keep.append(p)
        desc[f].p, desc[f].pitch = p.ctypes.data, p.strides[0]
    out = np.zeros(n, np.uint64)
    blurred = np.zeros((h, w), np.uint16)
    bt = (C.c_int * len(batches))(*batches)
    rc = L.me_sequence(w, h, LAYOUT.get(layout, layout), bits, len(batches), bt, desc, out.ctypes.data_as(C.c_void_p),
                       blurred.ctypes.data_as(C.c_void_p) if want_blur else None)
    if rc != 0:
        return None
    sads = [int(v) for v in out]
    return (sads, blurred.astype(np.int64)) if want_blur else sads
