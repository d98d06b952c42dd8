"""TEST INFRASTRUCTURE ONLY: the pictures of the XPSNR tests in the four layouts of include/turbo_metrics_xpsnr.h, and the
emulated kernels (tests/xpsnr_emul/libxpsnr_emul.so: the SOURCE of turbo-metrics_amd/csrc/tm_xpsnr_kernels.h run lane by lane on
the CPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tm_pkg import tm

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_EMUL_DIR = os.path.join(_HERE, "xpsnr_emul")
_EMUL_LIB = os.path.join(_EMUL_DIR, "libxpsnr_emul.so")
_EMUL_SRCS = [os.path.join(_EMUL_DIR, "xpsnr_emul.cpp"), os.path.join(_HERE, "emul", "hip_emul.h")] + [
    os.path.join(_ROOT, "turbo-metrics_amd", "csrc", f) for f in ("tm_xpsnr_kernels.h", "tm_p10.h", "tm_platform.h", "tm_geom.h")]
LAYOUT = tm.xpsnr.LAYOUTS


def pictures(w, h, n, bits):
    """pair n of a moving synthetic sequence: ((Y, Cb, Cr), (Y, Cb, Cr)) int64 with D = bits (8, 10, or 11..16 from the 10-bit pair)"""
    ref, dis = tm.synth.yuv420_pair(w, h, n, 8 if bits == 8 else 10)
    if bits > 10:
        up = lambda p: (p << (bits - 10)) | (p & ((1 << (bits - 10)) - 1))
        ref, dis = tuple(up(p) for p in ref), tuple(up(p) for p in dis)
    return ref, dis


def layout_planes(layout, planes, w, h, bits, pad=0):
    """(Y, Cb, Cr) sample values -> the plane arrays one picture of `layout` is handed over as (rows padded by `pad` elements)"""
    Y, Cb, Cr = (np.asarray(p, np.int64) for p in planes)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if layout in ("nv12", "p016"):
        dt, sh = (np.uint8, 0) if layout == "nv12" else (np.uint16, 16 - bits)
        y = np.zeros((h, w + pad), dt)
        y[:, :w] = Y << sh
        c = np.zeros((ch, 2 * cw + pad), dt)
        c[:, 0:2 * cw:2] = Cb << sh
        c[:, 1:2 * cw:2] = Cr << sh
        return [y, c]
    if layout == "i420":
        dt = np.uint8 if bits == 8 else np.uint16
        out = []
        for p in (Y, Cb, Cr):
            a = np.zeros((p.shape[0], p.shape[1] + pad), dt)
            a[:, :p.shape[1]] = p
            out.append(a)
        return out
    assert layout == "i420p10" and bits == 10
    return [tm.synth.p10_pack_plane(p, tm.synth.p10_row_words(p.shape[1]) + pad) for p in (Y, Cb, Cr)]


def build_emul():
    if os.path.exists(_EMUL_LIB) and all(os.path.getmtime(s) <= os.path.getmtime(_EMUL_LIB) for s in _EMUL_SRCS):
        return _EMUL_LIB
    # the flags tests/emul/emul.py builds the engine's emulated kernels with
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-pthread",
                           "-Wno-unknown-pragmas", "-I", os.path.join(_HERE, "emul"), "-o", _EMUL_LIB, _EMUL_SRCS[0]])
    return _EMUL_LIB


class _Desc(C.Structure):
    _fields_ = [("p0", C.c_void_p), ("p1", C.c_void_p), ("p2", C.c_void_p), ("pitch", C.c_ulonglong), ("pitch2", C.c_ulonglong),
                ("vec", C.c_int), ("pad_", C.c_int)]


def emulate(w, h, layout, bits, fps, batches, frames):
    """the emulated kernels over a sequence: frames = [(ref plane arrays, dis plane arrays)] (layout_planes), split into launches of
    `batches` slots; -> [(wsse_y, wsse_cb, wsse_cr)] per frame, or None for a geometry the library refuses"""
    L = C.CDLL(build_emul())
    assert L.xe_desc_size() == C.sizeof(_Desc)
    n = len(frames)
    assert sum(batches) == n
    desc = (_Desc * (2 * n))()
    keep = []
    for f, pair in enumerate(frames):
        for side, planes in enumerate(pair):
            planes = [np.ascontiguousarray(p) for p in planes]
            keep.extend(planes)
            d = desc[2 * f + side]
            d.p0, d.p1 = planes[0].ctypes.data, planes[1].ctypes.data
            d.p2 = planes[2].ctypes.data if len(planes) > 2 else None
            d.pitch, d.pitch2 = planes[0].strides[0], planes[1].strides[0]
    out = np.zeros(3 * n, np.uint64)
    bt = (C.c_int * len(batches))(*batches)
    rc = L.xe_sequence(w, h, LAYOUT[layout], bits, fps[0], fps[1], len(batches), bt, desc, out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        return None
    return [tuple(int(v) for v in out[3 * f:3 * f + 3]) for f in range(n)]
