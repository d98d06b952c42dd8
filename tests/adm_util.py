"""TEST INFRASTRUCTURE ONLY: the luma planes of the ADM tests in the four layouts of include/turbo_metrics_adm.h, their contents, and
the emulated kernels (tests/adm_emul/libadm_emul.so: the SOURCE of turbo-metrics_amd/csrc/tm_adm_kernels.h run lane by lane on the
CPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import motion_util

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_EMUL_DIR = os.path.join(_HERE, "adm_emul")
_EMUL_LIB = os.path.join(_EMUL_DIR, "libadm_emul.so")
_EMUL_SRCS = [os.path.join(_EMUL_DIR, "adm_emul.cpp"), os.path.join(_HERE, "emul", "hip_emul.h")] + [
    os.path.join(_ROOT, "turbo-metrics_amd", "csrc", f) for f in ("tm_adm_kernels.h", "tm_sample_load.h", "tm_p10.h", "tm_platform.h", "tm_geom.h")]
LAYOUT = {"y8": 0, "y16_msb": 1, "y16_low": 2, "y10_packed": 3}
# the four layouts at D = 8, 10, 12, 16 (what each carries)
CASES = (("y8", 8), ("y16_msb", 10), ("y16_msb", 12), ("y16_msb", 16), ("y16_low", 10), ("y16_low", 12), ("y16_low", 16), ("y10_packed", 10))
CONTENTS = ("noise", "blurred", "noisy", "edges", "enhanced", "negative")

luma_plane = motion_util.luma_plane  # sample values -> the plane array of a layout, optionally padded and with dirty bits


def _smooth(rng, w, h, M):
    """a picture with structure at every scale: coarse noise enlarged and box-blurred, plus fine noise"""
    coarse = rng.integers(0, M + 1, ((h + 7) // 8 + 1, (w + 7) // 8 + 1)).astype(np.float64)
    img = np.kron(coarse, np.ones((8, 8)))[:h, :w]
    p = np.pad(img, 2, mode="edge")
    img = sum(p[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)) / 25.0
    return np.clip(img + rng.integers(-(M // 16), M // 16 + 1, (h, w)), 0, M).astype(np.int64)


def pair(w, h, bits, kind, seed=0):
    """(ref, dis) sample values (int64) of depth `bits`:
      noise      independent uniform samples (the angle test fails almost everywhere)
      blurred    a structured picture and a box-blurred copy of it (detail loss: 0 < k < 1)
      noisy      the structured picture plus noise (additive impairment: the masking threshold matters)
      edges      a full-scale checkerboard of 5 x 3 blocks and the same shifted by one column, one sample changed (large coefficients)
      enhanced   dis = ref with its contrast about mid-grey raised by 1.5 and clipped (the angle test passes: the gain limit)
      negative   dis = maximum - ref (k clamps at 0)"""
    rng = np.random.default_rng([0xAD3, seed, w, h, bits])
    M = (1 << bits) - 1
    if kind == "noise":
        ref, dis = rng.integers(0, M + 1, (h, w)), rng.integers(0, M + 1, (h, w))
    elif kind == "blurred":
        ref = _smooth(rng, w, h, M)
        p = np.pad(ref, 1, mode="edge")
        dis = (p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] + 4 * ref) // 8
    elif kind == "noisy":
        ref = _smooth(rng, w, h, M)
        dis = np.clip(ref + rng.integers(-(M // 32) - 1, M // 32 + 2, (h, w)), 0, M)
    elif kind == "edges":
        y, x = np.indices((h, w))
        ref = ((x // 5 + y // 3) % 2) * M
        dis = (((x + 1) // 5 + y // 3) % 2) * M
        dis[h // 2, w // 3] = M // 2
    elif kind == "enhanced":
        ref = _smooth(rng, w, h, M)
        dis = np.clip((ref - M // 2) * 3 // 2 + M // 2, 0, M)
    elif kind == "negative":
        ref = _smooth(rng, w, h, M)
        dis = M - ref
    else:
        raise ValueError(kind)
    return np.asarray(ref, np.int64), np.asarray(dis, np.int64)


def build_emul():
    if os.path.exists(_EMUL_LIB) and all(os.path.getmtime(s) <= os.path.getmtime(_EMUL_LIB) for s in _EMUL_SRCS):
        return _EMUL_LIB
    # the flags tests/emul/emul.py builds the engine's emulated kernels with
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-pthread",
                           "-Wno-unknown-pragmas", "-I", os.path.join(_HERE, "emul"), "-o", _EMUL_LIB, _EMUL_SRCS[0]])
    return _EMUL_LIB


class _Desc(C.Structure):
    _fields_ = [("p", C.c_void_p * 2), ("pitch", C.c_ulonglong * 2), ("vec", C.c_int * 2)]


def emul_lib():
    L = C.CDLL(build_emul())
    assert L.ae_desc_size() == C.sizeof(_Desc)
    return L


def filters():
    lo, hi = (C.c_float * 4)(), (C.c_float * 4)()
    emul_lib().ae_filters(lo, hi)
    return tuple(np.float32(v) for v in lo), tuple(np.float32(v) for v in hi)


def geom(w, h, layout="y8", bits=8):
    """the kernel's geometry: dict(sizes=[(w, h, bw, bh)], border=[(left, top, right, bottom)], rf=[(h, v, d)], cos2), or None for what
    the library refuses"""
    i4 = lambda: (C.c_int * 4)()
    ws, hs, bws, bhs, bd, rf, c2 = i4(), i4(), i4(), i4(), (C.c_int * 16)(), (C.c_float * 12)(), C.c_float()
    if emul_lib().ae_geom(w, h, LAYOUT.get(layout, layout), bits, ws, hs, bws, bhs, bd, rf, C.byref(c2)) != 0:
        return None
    return dict(sizes=[(ws[s], hs[s], bws[s], bhs[s]) for s in range(4)], border=[tuple(bd[4 * s:4 * s + 4]) for s in range(4)],
                rf=[tuple(np.float32(v) for v in rf[3 * s:3 * s + 3]) for s in range(4)], cos2=np.float32(c2.value))


def emulate(w, h, layout, bits, ref_plane, dis_plane, want_planes=True):
    """the emulated kernels over one pair of plane arrays (luma_plane) -> per scale dict(num=[3], den=[3], r=(h, v, d), add=(h, v, d),
    thr, a=(a_ref, a_dis)), or None for a geometry the library refuses"""
    L = emul_lib()
    g = geom(w, h, layout, bits)
    if g is None:
        return None
    d = _Desc()
    keep = []
    for i, p in enumerate((ref_plane, dis_plane)):
        if p.strides[1] != p.itemsize:
            p = np.ascontiguousarray(p)
        keep.append(p)
        d.p[i], d.pitch[i] = p.ctypes.data, p.strides[0]
    sums = np.zeros((4, 6), np.float64)
    planes = [np.full((9, g["sizes"][s][3], g["sizes"][s][2]), np.nan, np.float32) for s in range(4)]
    pp = (C.POINTER(C.c_float) * 4)(*[p.ctypes.data_as(C.POINTER(C.c_float)) for p in planes])
    rc = L.ae_pair(w, h, LAYOUT.get(layout, layout), bits, C.byref(d), sums.ctypes.data_as(C.c_void_p), pp if want_planes else None)
    assert rc == 0
    return [dict(num=[float(v) for v in sums[s, :3]], den=[float(v) for v in sums[s, 3:]], r=tuple(planes[s][0:3]), add=tuple(planes[s][3:6]),
                 thr=planes[s][6], a=(planes[s][7], planes[s][8])) for s in range(4)]
