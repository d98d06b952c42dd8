"""TEST INFRASTRUCTURE ONLY: pictures and tolerances of the HaarPSI tests and the emulated kernels (tests/haarpsi_emul/libhaarpsi_emul.so:
the SOURCE of turbo-metrics_amd/csrc/tm_haarpsi_kernels.h run lane by lane on the CPU).  The plane arrays of the four luma layouts come
from tests/motion_util.luma_plane, dirty bits included; the picture kinds are those of the GMSD tests."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from tests import gmsd_util, hvs_util, motion_util

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_EMUL_DIR = os.path.join(_HERE, "haarpsi_emul")
_EMUL_LIB = os.path.join(_EMUL_DIR, "libhaarpsi_emul.so")
_EMUL_SRCS = [os.path.join(_EMUL_DIR, "haarpsi_emul.cpp"), os.path.join(_HERE, "emul", "hip_emul.h")] + [
    os.path.join(_ROOT, "turbo-metrics_amd", "csrc", f) for f in ("tm_haarpsi_kernels.h", "tm_sample_load.h", "tm_p10.h", "tm_platform.h", "tm_geom.h")]
LAYOUT = {"y8": 0, "y16_msb": 1, "y16_low": 2, "y10_packed": 3}
# the four layouts at b = 8, 10, 12, 16 (what each carries)
CASES = (("y8", 8), ("y16_msb", 10), ("y16_msb", 12), ("y16_msb", 16), ("y16_low", 10), ("y16_low", 12), ("y16_low", 16), ("y10_packed", 10))
KINDS = gmsd_util.KINDS

# The emulated kernel (every f32 operation the kernel's own) against the float64 restatement in the paper's form: the largest absolute
# error of the score (it lives in [0, 1]) that tests/test_haarpsi_cpu.py::test_emulation_against_restatement measures over every shape,
# CASE, KIND and both load paths is 6.1e-8 (it prints it); the tolerance is that times 4 (the project's margin for pictures outside the
# measured set).  The condition the issue sets, not a measurement: the measured figure may not exceed 1e-5 (HaarPSI is published to four
# decimals).
MEASURED_ABS = 6.1e-8
ABS_TOL = 4 * MEASURED_ABS
assert MEASURED_ABS <= 1e-5

ALPHA_F32 = float(np.float32(4.2))   # the alpha the device multiplies by and the host function divides by

luma_plane = motion_util.luma_plane  # sample values -> the plane array of a layout, optionally padded and with dirty bits
aligned_copy = hvs_util.aligned_copy
planes_of = hvs_util.planes_of       # [(ref, dis) sample values] -> [(ref plane array, dis plane array)] of a layout
pair = gmsd_util.pair                # (w, h, bits, kind, seed) -> (ref, dis) sample values


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
        assert L.he_desc_size() == C.sizeof(_Desc)
        L.he_e_of.restype = C.c_float
        L.he_e_of.argtypes = [C.c_int, C.c_int, C.c_ulonglong]
        for f in (L.he_exp_pos, L.he_q_of):
            f.restype = C.c_float
            f.argtypes = [C.c_float]
        L.he_alpha.restype = C.c_float
        _lib = L
    return _lib


def tile():
    """(TW, TH): decimated positions per tile edge"""
    L = emul_lib()
    return int(L.he_tile_w()), int(L.he_tile_h())


def shapes():
    """the sizes the issue names, from the kernel's tile: widths 4, 5, 7, 2 TW - 1, 2 TW, 2 TW + 1, 2 TW + 6, 2 TW + 8, 2 TW + 9 (the 3 / 4
    position halo crosses a tile edge and the picture edge together), 4 TW + 2, and the heights alike from TH: one sparse set of pairs
    in which every width and every height occurs"""
    tw, th = tile()
    return ((4, 4), (5, 7), (7, 5), (2 * tw - 1, 2 * th + 1), (2 * tw, 2 * th), (2 * tw + 1, 2 * th - 1), (2 * tw + 6, 2 * th + 9), (2 * tw + 8, 2 * th + 8),
            (2 * tw + 9, 2 * th + 6), (4 * tw + 2, 5), (7, 4 * th + 2), (4 * tw + 2, 4 * th + 2))


def geom(w, h, layout, bits, maps=False):
    """(w2, h2, cells, C_1, C_2) per slot, or None where the library refuses"""
    out = (C.c_ulonglong * 6)()
    if emul_lib().he_geom(w, h, LAYOUT.get(layout, layout), bits, int(maps), out):
        return None
    return tuple(int(v) for v in out[:5])


def kernel_e(hr, hd, c):
    """the kernel's f32 expression e_k of one position, orientation and scale from the exact integer coefficients"""
    return float(emul_lib().he_e_of(int(hr), int(hd), int(c)))


def kernel_exp(z):
    """the kernel's exp(z), z in [0, 4.2]"""
    return float(emul_lib().he_exp_pos(float(z)))


def kernel_q(s):
    """the kernel's q = 1 / (1 + exp(4.2f s))"""
    return float(emul_lib().he_q_of(float(s)))


def emulate(w, h, layout, bits, batches, frames, cap=None, vec=None, maps=False):
    """the emulated kernels over pairs: frames = [(ref plane array, dis plane array)] (luma_plane); compute c takes the next batches[c]
    pairs as its slots 0 .. batches[c]-1 of ONE library object with `cap` slots (default: the largest batch), whose buffers are reused
    from compute to compute.  vec=False: the sample-by-sample path everywhere.  -> [(q, ws)] per pair (maps: and the float32 local
    similarity maps [pair, h2, w2]), or None for a geometry the library refuses"""
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
    q = np.zeros(n, np.float64)
    ws = np.zeros(n, np.uint64)
    mp = np.zeros((n, gm[1], gm[0]), np.float32) if maps else None
    bt = (C.c_int * len(batches))(*batches)
    rc = L.he_run(w, h, LAYOUT[layout], bits, cap or max(batches), len(batches), bt, desc, -1 if vec is None else int(bool(vec)),
                  q.ctypes.data_as(C.c_void_p), ws.ctypes.data_as(C.c_void_p), mp.ctypes.data_as(C.c_void_p) if maps else None)
    assert rc == 0, rc
    out = [(float(q[i]), int(ws[i])) for i in range(n)]
    return (out, mp) if maps else out


def score(q, ws):
    """tm_haarpsi_score restated in Python floats (the same double operations)"""
    if ws == 0:
        return math.nan
    x = q / float(ws)
    s = math.log((1.0 - x) / x) / ALPHA_F32
    return s * s
