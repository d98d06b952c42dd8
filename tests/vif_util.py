"""TEST INFRASTRUCTURE ONLY: the luma planes of the VIF tests in the four layouts of include/turbo_metrics_vif.h, their contents, and
the emulated kernels (tests/vif_emul/libvif_emul.so: the SOURCE of turbo-metrics_amd/csrc/tm_vif_kernels.h run lane by lane on the
CPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import motion_util

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_EMUL_DIR = os.path.join(_HERE, "vif_emul")
_EMUL_LIB = os.path.join(_EMUL_DIR, "libvif_emul.so")
_EMUL_SRCS = [os.path.join(_EMUL_DIR, "vif_emul.cpp"), os.path.join(_HERE, "emul", "hip_emul.h")] + [
    os.path.join(_ROOT, "turbo-metrics_amd", "csrc", f) for f in ("tm_vif_kernels.h", "tm_sample_load.h", "tm_p10.h", "tm_platform.h", "tm_geom.h")]
LAYOUT = {"y8": 0, "y16_msb": 1, "y16_low": 2, "y10_packed": 3}
# the four layouts at D = 8, 10, 12, 16 (what each carries)
CASES = (("y8", 8), ("y16_msb", 10), ("y16_msb", 12), ("y16_msb", 16), ("y16_low", 10), ("y16_low", 12), ("y16_low", 16), ("y10_packed", 10))
CONTENTS = ("noise", "blurred", "checker", "flat_ref", "identical", "negative")

luma_plane = motion_util.luma_plane  # sample values -> the plane array of a layout, optionally padded and with dirty bits


def pair(w, h, bits, kind, seed=0):
    """(ref, dis) sample values (int64) of depth `bits`:
      noise      independent uniform samples
      blurred    noise and a box-blurred copy of it plus a little noise (a positively correlated pair)
      checker    a full-scale checkerboard and its inverse shifted by one row (the largest accumulators)
      flat_ref   a flat reference, noise as distorted (variance of the reference below the noise floor, large B)
      identical  dis = ref
      negative   dis = maximum - ref (covariance <= 0)"""
    rng = np.random.default_rng([0x71F, seed, w, h, bits])
    M = (1 << bits) - 1
    ref = rng.integers(0, M + 1, (h, w), dtype=np.int64)
    if kind == "noise":
        dis = rng.integers(0, M + 1, (h, w), dtype=np.int64)
    elif kind == "blurred":
        p = np.pad(ref, 1, mode="edge")
        dis = (p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] + 4 * ref) // 8
        dis = np.clip(dis + rng.integers(-(M // 64) - 1, M // 64 + 2, (h, w)), 0, M)
    elif kind == "checker":
        y, x = np.indices((h, w))
        ref = ((x + y) % 2) * M
        dis = ((x + y + (y > h // 2)) % 2) * M
    elif kind == "flat_ref":
        dis, ref = ref, np.full((h, w), M // 3, np.int64)
    elif kind == "identical":
        dis = ref.copy()
    elif kind == "negative":
        dis = M - ref
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
    _fields_ = [("p", C.c_void_p * 2), ("pitch", C.c_ulonglong * 2), ("vec", C.c_int * 2)]


def emul_lib():
    L = C.CDLL(build_emul())
    assert L.ve_desc_size() == C.sizeof(_Desc)
    return L


def filters():
    L, out = emul_lib(), []
    for s in range(4):
        buf = (C.c_uint * 17)()
        out.append(tuple(buf[:L.ve_filter(s, buf)]))
    return tuple(out)


def emulate(w, h, layout, bits, ref_plane, dis_plane, want_planes=True):
    """the emulated kernels over one pair of plane arrays (luma_plane) -> [dict(num, den, planes=(s1, s2, s12))] per scale, or None
    for a geometry the library refuses"""
    L = emul_lib()
    ws, hs = (C.c_int * 4)(), (C.c_int * 4)()
    if L.ve_sizes(w, h, LAYOUT.get(layout, layout), bits, ws, hs) != 0:
        return None
    d = _Desc()
    keep = []
    for i, p in enumerate((ref_plane, dis_plane)):
        if p.strides[1] != p.itemsize:
            p = np.ascontiguousarray(p)
        keep.append(p)
        d.p[i], d.pitch[i] = p.ctypes.data, p.strides[0]
    nd = np.zeros((4, 2), np.float64)
    planes = [np.full((3, hs[s], ws[s]), -(1 << 31), np.int32) for s in range(4)]
    pp = (C.POINTER(C.c_int) * 4)(*[p.ctypes.data_as(C.POINTER(C.c_int)) for p in planes])
    rc = L.ve_pair(w, h, LAYOUT.get(layout, layout), bits, C.byref(d), nd.ctypes.data_as(C.c_void_p), pp if want_planes else None)
    assert rc == 0
    return [dict(num=float(nd[s, 0]), den=float(nd[s, 1]), planes=tuple(planes[s])) for s in range(4)]
