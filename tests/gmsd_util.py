"""TEST INFRASTRUCTURE ONLY: pictures and tolerances of the GMSD tests and the emulated kernels (tests/gmsd_emul/libgmsd_emul.so: the
SOURCE of turbo-metrics_amd/csrc/tm_gmsd_kernels.h run lane by lane on the CPU).  The plane arrays of the four luma layouts come from
tests/motion_util.luma_plane, dirty bits included."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from tests import hvs_util, motion_util

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_EMUL_DIR = os.path.join(_HERE, "gmsd_emul")
_EMUL_LIB = os.path.join(_EMUL_DIR, "libgmsd_emul.so")
_EMUL_SRCS = [os.path.join(_EMUL_DIR, "gmsd_emul.cpp"), os.path.join(_HERE, "emul", "hip_emul.h")] + [
    os.path.join(_ROOT, "turbo-metrics_amd", "csrc", f) for f in ("tm_gmsd_kernels.h", "tm_sample_load.h", "tm_p10.h", "tm_platform.h", "tm_geom.h")]
LAYOUT = {"y8": 0, "y16_msb": 1, "y16_low": 2, "y10_packed": 3}
# the four layouts at b = 8, 10, 12, 16 (what each carries)
CASES = (("y8", 8), ("y16_msb", 10), ("y16_msb", 12), ("y16_msb", 16), ("y16_low", 10), ("y16_low", 12), ("y16_low", 16), ("y10_packed", 10))
KINDS = ("noise", "flat_noise", "ramp_one", "checker", "near_peak", "blur", "identical")

# The emulated kernel (every f32 operation the kernel's own) against the float64 restatement in the paper's form: the largest absolute
# error of gmsd and of gmsm (both live in [0, 1]) that tests/test_gmsd_cpu.py::test_emulation_against_restatement measures over every
# shape, CASE and KIND is 1.5e-8 / 1.6e-8 (it prints both); the tolerance is the larger times 4 (FLIP's margin, for pictures outside the
# measured set).  The condition the issue sets, not a measurement: the measured figure may not exceed 1e-5 (GMSD is published to four
# decimals).
MEASURED_ABS = 1.6e-8
ABS_TOL = 4 * MEASURED_ABS
assert MEASURED_ABS <= 1e-5

luma_plane = motion_util.luma_plane  # sample values -> the plane array of a layout, optionally padded and with dirty bits
aligned_copy = hvs_util.aligned_copy
planes_of = hvs_util.planes_of       # [(ref, dis) sample values] -> [(ref plane array, dis plane array)] of a layout


def pair(w, h, bits, kind, seed=0):
    """(ref, dis) sample values (int64) of depth `bits`:
      noise       independent uniform samples on both sides
      flat_noise  a flat reference (no gradient away from the border) against noise
      ramp_one    a ramp, and the same ramp with one sample off by one code
      checker     3 x 3 cells of code 0 and code 2^b - 1, against the inverse in the lower half and itself above
      near_peak   a slow ramp just below 2^b - 1, and a copy that differs by one code in a quarter of the samples
      blur        smooth texture plus noise, and its 3 x 3 box blur
      identical   noise against itself"""
    rng = np.random.default_rng([0x6D5D, seed, w, h, bits, KINDS.index(kind)])
    M = (1 << bits) - 1
    y, x = np.indices((h, w))
    if kind == "noise":
        ref, dis = rng.integers(0, M + 1, (h, w)), rng.integers(0, M + 1, (h, w))
    elif kind == "flat_noise":
        ref, dis = np.full((h, w), M // 3), rng.integers(0, M + 1, (h, w))
    elif kind == "ramp_one":
        ref = ((x * 5 + y * 3 + seed) * max(1, M // 255)) % (M + 1)
        dis = ref.copy()
        px, py = int(rng.integers(0, w)), int(rng.integers(0, h))
        dis[py, px] += 1 if dis[py, px] < M else -1
    elif kind == "checker":
        ref = ((x // 3 + y // 3) % 2) * M
        dis = ((x // 3 + y // 3 + (y >= h // 2)) % 2) * M
    elif kind == "near_peak":
        ref = M - ((x + 2 * y) // 4) % 8
        dis = ref - (rng.integers(0, 4, (h, w)) == 0)
    elif kind == "blur":
        ref = np.clip((np.sin(x / 3.0) * np.cos(y / 5.0) * 0.4 + 0.5) * M + rng.integers(-(M // 16), M // 16 + 1, (h, w)), 0, M).astype(np.int64)
        p = np.pad(ref, 1, mode="edge")
        dis = sum(p[i:i + h, j:j + w] for i in range(3) for j in range(3)) // 9
    elif kind == "identical":
        ref = rng.integers(0, M + 1, (h, w))
        dis = ref.copy()
    else:
        raise ValueError(kind)
    return ref.astype(np.int64), dis.astype(np.int64)


def build_emul():
    if os.path.exists(_EMUL_LIB) and all(os.path.getmtime(s) <= os.path.getmtime(_EMUL_LIB) for s in _EMUL_SRCS):
        return _EMUL_LIB
    # the flags tests/emul/emul.py builds the engine's emulated kernels with
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-pthread",
                           "-Wno-unknown-pragmas", "-I", os.path.join(_HERE, "emul"), "-o", _EMUL_LIB, _EMUL_SRCS[0]])
    return _EMUL_LIB


class _Desc(C.Structure):
    _fields_ = [("p", C.c_void_p * 2), ("pitch", C.c_ulonglong * 2), ("vec", C.c_int), ("pad_", C.c_int)]


_lib = None


def emul_lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build_emul())
        assert L.ge_desc_size() == C.sizeof(_Desc)
        L.ge_e_of.restype = C.c_float
        L.ge_e_of.argtypes = [C.c_ulonglong] * 3
        _lib = L
    return _lib


def tile():
    """(TW, TH): decimated positions per tile edge"""
    L = emul_lib()
    return int(L.ge_tile_w()), int(L.ge_tile_h())


def shapes():
    """the sizes the issue names, from the kernel's tile"""
    tw, th = tile()
    return ((4, 4), (5, 7), (2 * tw - 1, 2 * th + 1), (2 * tw, 2 * th), (2 * tw + 1, 2 * th - 1), (2 * tw + 2, 2 * th + 3), (4 * tw + 1, 2 * th))


def geom(w, h, layout, bits, maps=False):
    """(w2, h2, cells, C) per slot, or None where the library refuses"""
    out = (C.c_ulonglong * 5)()
    if emul_lib().ge_geom(w, h, LAYOUT.get(layout, layout), bits, int(maps), out):
        return None
    return int(out[0]), int(out[1]), int(out[2]), int(out[3])


def kernel_e(ar, ad, c):
    """the kernel's f32 expression e of one position from the exact integers"""
    return float(emul_lib().ge_e_of(int(ar), int(ad), int(c)))


def emulate(w, h, layout, bits, batches, frames, cap=None, vec=None, maps=False):
    """the emulated kernels over pairs: frames = [(ref plane array, dis plane array)] (luma_plane); compute c takes the next batches[c]
    pairs as its slots 0 .. batches[c]-1 of ONE library object with `cap` slots (default: the largest batch), whose buffers are reused
    from compute to compute.  vec=False: the sample-by-sample path everywhere.  -> [(e1, e2, e_max, n)] per pair (maps: and the float32
    GMS maps [pair, h2, w2]), or None for a geometry the library refuses"""
    L = emul_lib()
    gm = geom(w, h, layout, bits)
    if gm is None:
        return None
    n = len(frames)
    assert sum(batches) == n
    desc = (_Desc * n)()
    keep = []
    for f, pr in enumerate(frames):
        for side, p in enumerate(pr):
            if p.strides[1] != p.itemsize:
                p = np.ascontiguousarray(p)
            keep.append(p)
            desc[f].p[side], desc[f].pitch[side] = p.ctypes.data, p.strides[0]
    res = np.zeros((n, 3), np.float64)
    mp = np.zeros((n, gm[1], gm[0]), np.float32) if maps else None
    bt = (C.c_int * len(batches))(*batches)
    rc = L.ge_run(w, h, LAYOUT[layout], bits, cap or max(batches), len(batches), bt, desc, -1 if vec is None else int(bool(vec)),
                  res.ctypes.data_as(C.c_void_p), mp.ctypes.data_as(C.c_void_p) if maps else None)
    assert rc == 0, rc
    out = [(float(res[i, 0]), float(res[i, 1]), float(res[i, 2]), gm[0] * gm[1]) for i in range(n)]
    return (out, mp) if maps else out


def score(e1, e2, n, population=False):
    """tm_gmsd_score restated in Python floats (the same double operations)"""
    if n < 2:
        return math.nan
    return math.sqrt(max(0.0, (e2 - e1 * e1 / n) / (n if population else n - 1)))


def mean(e1, n):
    return math.nan if n < 2 else 1.0 - e1 / n
