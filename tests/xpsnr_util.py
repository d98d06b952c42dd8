"""TEST INFRASTRUCTURE ONLY: the pictures of the XPSNR tests in the four layouts of include/turbo_metrics_xpsnr.h, and the
emulated kernels (tests/xpsnr_emul/libxpsnr_emul.so: the SOURCE of turbo-metrics_amd/csrc/tm_xpsnr_kernels.h run lane by lane on
the CPU)."""
import ctypes as C
import math
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


KINDS = ("synth", "checker", "stripes", "flat", "identical", "random", "steps")


def pictures(w, h, n, bits, kind="synth"):
    """pair n of a sequence of `kind`: ((Y, Cb, Cr), (Y, Cb, Cr)) int64 with D = bits, M = 2^D - 1:
      synth      the moving synthetic sequence (tm.synth.yuv420_pair; 11..16 bits widened from the 10-bit pair)
      checker    0 / M checkerboard (M where x + y is odd), the distorted picture M - it: the largest |f| and sse; the same every n
      stripes    period-4 columns (M where x % 4 < 2), the distorted picture M - it; the same every n
      flat       every sample n K (K = 2^(D-4), capped at M - 1), the distorted picture one more
      identical  the synthetic reference on both sides
      random     independent uniform samples over [0, M] on both sides (seed n)
      steps      a level per luma block of the definition's partition (and per chroma block), random over [0, M]; the distorted
                 picture another such step picture (seed n)"""
    M = (1 << bits) - 1
    cw, ch = (w + 1) // 2, (h + 1) // 2
    shapes = ((h, w), (ch, cw), (ch, cw))
    if kind in ("synth", "identical"):
        ref, dis = tm.synth.yuv420_pair(w, h, n, 8 if bits == 8 else 10)
        if bits > 10:
            up = lambda p: (p << (bits - 10)) | (p & ((1 << (bits - 10)) - 1))
            ref, dis = tuple(up(p) for p in ref), tuple(up(p) for p in dis)
        return (ref, ref) if kind == "identical" else (ref, dis)
    if kind in ("checker", "stripes"):
        def pat(sh):
            y, x = np.indices(sh)
            return np.where((x + y) % 2 == 1 if kind == "checker" else x % 4 < 2, M, 0).astype(np.int64)
        ref = tuple(pat(sh) for sh in shapes)
        return ref, tuple(M - p for p in ref)
    if kind == "flat":
        v = min(n * (1 << (bits - 4)), M - 1)
        return tuple(np.full(sh, v, np.int64) for sh in shapes), tuple(np.full(sh, v + 1, np.int64) for sh in shapes)
    rng = np.random.default_rng([0x5EED, n, w, h, bits, KINDS.index(kind)])
    if kind == "random":
        return tuple(tuple(rng.integers(0, M + 1, sh, dtype=np.int64) for sh in shapes) for _ in range(2))
    assert kind == "steps"
    b = max(4, _block(w, h))
    bx, by = max(1, b * cw // w), max(1, b * ch // h)

    def step(sh, sx, sy):
        lv = rng.integers(0, M + 1, (-(-sh[0] // sy), -(-sh[1] // sx)), dtype=np.int64)
        return np.repeat(np.repeat(lv, sy, 0), sx, 1)[:sh[0], :sh[1]]
    return tuple(tuple(step(sh, *((b, b) if i == 0 else (bx, by))) for i, sh in enumerate(shapes)) for _ in range(2))


def _block(w, h):
    return 4 * int(32 * math.sqrt(w * h / (3840 * 2160)) + 0.5)


def dirt_seed(frame, side):
    """the `dirty=` seed of one picture: a different fill for each frame and side"""
    return 0xD1E7 + 2 * frame + side


def layout_planes(layout, planes, w, h, bits, pad=0, dirty=None):
    """(Y, Cb, Cr) sample values -> the plane arrays one picture of `layout` is handed over as (rows padded by `pad` elements).
    dirty=None writes 0 into every byte the kernels must ignore; dirty=<seed> fills them with seeded garbage instead: the low 16 - D
    bits of P016 words, the bits above D of 16-bit I420 words, bits 30-31 of packed 10-bit words and the absent samples of a row's
    last packed run, and every padding element past a row's last sample."""
    Y, Cb, Cr = (np.asarray(p, np.int64) for p in planes)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    rng = None if dirty is None else np.random.default_rng([0xD127, dirty])

    def junk(shape, dt, bits_=None):
        if rng is None:
            return np.zeros(shape, dt)
        hi = 1 << (8 * np.dtype(dt).itemsize if bits_ is None else bits_)
        return rng.integers(0, hi, shape, dtype=np.uint64).astype(dt)

    def padded(vals, dt, n):
        a = junk((vals.shape[0], n + pad), dt)
        a[:, :n] = vals
        return a
    if layout in ("nv12", "p016"):
        dt, sh = (np.uint8, 0) if layout == "nv12" else (np.uint16, 16 - bits)
        low = lambda shape: junk(shape, np.int64, sh) if sh else 0
        y = padded((Y << sh) | low(Y.shape), dt, w)
        c = np.empty((ch, 2 * cw), np.int64)
        c[:, 0::2], c[:, 1::2] = Cb << sh, Cr << sh
        return [y, padded(c | low(c.shape), dt, 2 * cw)]
    if layout == "i420":
        if bits == 8:
            return [padded(p, np.uint8, p.shape[1]) for p in (Y, Cb, Cr)]
        high = lambda p: junk(p.shape, np.int64, 16 - bits) << bits if bits < 16 else 0
        return [padded(p | high(p), np.uint16, p.shape[1]) for p in (Y, Cb, Cr)]
    assert layout == "i420p10" and bits == 10
    out = []
    for p in (Y, Cb, Cr):
        words = tm.synth.p10_row_words(p.shape[1])
        full = junk((p.shape[0], 3 * words), np.int64, 10)  # the absent samples of the last run
        full[:, :p.shape[1]] = p
        a = padded(tm.synth.p10_pack_plane(full)[:, :words], np.uint32, words)
        a[:, :words] |= (junk((p.shape[0], words), np.uint32, 2) << np.uint32(30))
        out.append(a)
    return out


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
