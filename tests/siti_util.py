"""TEST INFRASTRUCTURE ONLY: the luma planes of the SI / TI tests in the four layouts of include/turbo_metrics_siti.h, and the emulated
kernel (tests/siti_emul/libsiti_emul.so: the SOURCE of turbo-metrics_amd/csrc/tm_siti_kernels.h run lane by lane on the CPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import motion_util

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_EMUL_DIR = os.path.join(_HERE, "siti_emul")
_EMUL_LIB = os.path.join(_EMUL_DIR, "libsiti_emul.so")
_EMUL_SRCS = [os.path.join(_EMUL_DIR, "siti_emul.cpp"), os.path.join(_HERE, "emul", "hip_emul.h")] + [
    os.path.join(_ROOT, "turbo-metrics_amd", "csrc", f) for f in ("tm_siti_kernels.h", "tm_sample_load.h", "tm_p10.h", "tm_platform.h", "tm_geom.h")]
LAYOUT = {"y8": 0, "y16_msb": 1, "y16_low": 2, "y10_packed": 3}
CASES = (("y8", 8), ("y16_msb", 10), ("y16_msb", 16), ("y16_low", 12), ("y16_low", 16), ("y10_packed", 10))
ONE_PER_LAYOUT = (("y8", 8), ("y16_msb", 12), ("y16_low", 10), ("y10_packed", 10))
TW, TH = 120, 30  # the tile of k_siti (test_siti_cpu.py checks them against the kernel header)

sequence = motion_util.sequence      # n luma planes of sample values: random | smooth | extreme
luma_plane = motion_util.luma_plane  # sample values -> the plane array of a layout, padded, dirty bits filled with garbage


def edge_sizes():
    """the sizes at which the kernel takes another path: the smallest picture, one row / column of interior, the tile width and height
    each -1, +0, +1, +2, a width that is no multiple of 4"""
    out = [(3, 3), (3, 40), (40, 3), (37, 11)]
    out += [(TW + d, 7) for d in (-1, 0, 1, 2)]
    out += [(9, TH + d) for d in (-1, 0, 1, 2)]
    out += [(2 * TW + 1, 2 * TH + 1)]
    return out


P10_WIDTHS = (383, 384, 385, 769)  # cross a 384-sample block of the packed 10-bit row


def misaligned(plane):
    """the same plane at a base address that is no multiple of 16 (one element past one): the kernel's scalar load path"""
    esz = plane.itemsize
    h, n = plane.shape
    raw = np.zeros(h * n * esz + 64, np.uint8)
    off = (-raw.ctypes.data) % 16 + esz
    view = raw[off:off + h * n * esz].view(plane.dtype).reshape(h, n)
    view[...] = plane
    assert view.ctypes.data % 16 != 0
    return view


def build_emul():
    if os.path.exists(_EMUL_LIB) and all(os.path.getmtime(s) <= os.path.getmtime(_EMUL_LIB) for s in _EMUL_SRCS):
        return _EMUL_LIB
    # the flags tests/emul/emul.py builds the engine's emulated kernels with
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-pthread",
                           "-Wno-unknown-pragmas", "-I", os.path.join(_HERE, "emul"), "-o", _EMUL_LIB, _EMUL_SRCS[0]])
    return _EMUL_LIB


class _Desc(C.Structure):
    _fields_ = [("p", C.c_void_p), ("pitch", C.c_ulonglong), ("vec", C.c_int), ("pad_", C.c_int)]


def emul_lib():
    L = C.CDLL(build_emul())
    L.se_magnitude.restype = C.c_uint
    L.se_magnitude.argtypes = [C.c_ulonglong]
    return L


def emulate(w, h, layout, bits, batches, planes, want_last=False):
    """the emulated kernel over a sequence of plane arrays (luma_plane), split into launches of `batches` slots (a negative entry: a
    reset, then a batch of that many); -> [(s1, s2, t1, t2, ti_valid)] per picture as the library's get reports them (and the history
    plane after the last batch), or None for a geometry the library refuses"""
    L = emul_lib()
    assert L.se_desc_size() == C.sizeof(_Desc)
    n = len(planes)
    assert sum(abs(b) for b in batches) == n
    desc = (_Desc * n)()
    keep = []
    for f, p in enumerate(planes):
        if p.strides[1] != p.itemsize:
            p = np.ascontiguousarray(p)
        keep.append(p)
        desc[f].p, desc[f].pitch = p.ctypes.data, p.strides[0]
    out = np.zeros((n, 4), np.uint64)
    last = np.zeros((h, w), np.uint16)
    bt = (C.c_int * len(batches))(*batches)
    rc = L.se_sequence(w, h, LAYOUT.get(layout, layout), bits, len(batches), bt, desc, out.ctypes.data_as(C.c_void_p),
                       last.ctypes.data_as(C.c_void_p) if want_last else None)
    if rc != 0:
        return None
    starts, f0 = set(), 0
    for i, b in enumerate(batches):
        if i == 0 or b < 0:
            starts.add(f0)
        f0 += abs(b)
    t1 = out.view(np.int64)[:, 2]  # two's complement
    res = [(int(r[0]), int(r[1]), int(t1[f]), int(r[3]), 0 if f in starts else 1) for f, r in enumerate(out)]
    return (res, last.astype(np.int64)) if want_last else res


def y4m(path, frames, bits):
    """a 4:2:0 Y4M file of the luma planes (sample values); chroma is mid-grey"""
    h, w = frames[0].shape
    cw, ch = (w + 1) // 2, (h + 1) // 2
    tag = "C420jpeg" if bits == 8 else f"C420p{bits}"
    dt = np.uint8 if bits == 8 else np.dtype("<u2")
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 {tag}\n".encode())
        for Y in frames:
            f.write(b"FRAME\n")
            f.write(np.asarray(Y).astype(dt).tobytes())
            f.write(np.full(2 * cw * ch, 1 << (bits - 1), dt).tobytes())
