"""TEST INFRASTRUCTURE ONLY: pictures and tolerances of the dE ITP tests and the emulated kernel (tests/itp_emul/libitp_emul.so: the
SOURCE of turbo-metrics_amd/csrc/tm_itp_kernels.h run lane by lane on the CPU).  The plane arrays of the four layouts come from
tests/xpsnr_util.layout_planes, dirty bits included."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

from tests import itp_ref as R
from tests import xpsnr_util

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_EMUL_DIR = os.path.join(_HERE, "itp_emul")
_EMUL_LIB = os.path.join(_EMUL_DIR, "libitp_emul.so")
_EMUL_SRCS = [os.path.join(_EMUL_DIR, "itp_emul.cpp"), os.path.join(_HERE, "emul", "hip_emul.h")] + [
    os.path.join(_ROOT, "turbo-metrics_amd", "csrc", f)
    for f in ("tm_itp_kernels.h", "tm_ciede_kernels.h", "tm_sample_load.h", "tm_p10.h", "tm_platform.h", "tm_geom.h")]
LAYOUT = {"nv12": 0, "p016": 1, "i420": 2, "i420p10": 3}
TRANSFER = {"pq": 0, "hlg": 1}
layout_planes = xpsnr_util.layout_planes
# every layout at the depths it carries
CASES = (("nv12", 8), ("p016", 10), ("p016", 12), ("p016", 16), ("i420", 8), ("i420", 10), ("i420", 12), ("i420", 16), ("i420p10", 10))
KINDS = ("noise", "primaries", "near_neutral", "near_black", "near_peak", "quadrant", "one_code")
# the exponents of the device's pow(): kernel_pow(x, which)
POW_EXPONENTS = (32 / 2523, 16384 / 2610, 2610 / 16384, 2523 / 32, 0.2)

# ---- tolerances: measured, not chosen ---------------------------------------------------------------------------------------------
# A position agrees when |got - want| <= ATOL + RTOL * want against the float64 restatement.  The figures are measured by
# tests/test_itp_cpu.py::test_emulation_against_restatement over every shape, CASE, KIND and transfer (it prints them): MEASURED_ATOL
# is the largest |got - want| over the positions with want < 1, MEASURED_RTOL the largest |got - want| / want over those with
# want >= 1, MEASURED_MEAN_REL the largest relative error of de_mean.  The tolerances are 4 times those (this project's margin,
# tests/ciede_util.py).  The condition of DESIGN.md section 22: MEASURED_ATOL must not exceed ATOL_LIMIT, 1 % of the unit BT.2124
# defines as one just-noticeable difference; a pow() that misses it is defective, the tolerance is not widened.  The library on an
# MI355X gives the emulation's bits (tests/test_gpu_itp.py), so the device's figures ARE these.
ATOL_LIMIT = 0.01
MEASURED_ATOL = 6.7e-4       # (6.67e-4: 259 x 37 p016 at 16 bits, PQ, one_code)
MEASURED_RTOL = 5.9e-4       # (5.89e-4: 259 x 37 p016 at 10 bits, PQ, one_code)
MEASURED_MEAN_REL = 2.0e-3   # (1.99e-3: 2 x 2 p016 at 16 bits, PQ, one_code: a mean dE of 0.003, the error is the absolute one)
MEASURED_POW_REL = 6.0e-8    # the largest relative error of the f32 pow() over the five exponents: half an ulp
ATOL, RTOL, MEAN_REL_TOL = 4 * MEASURED_ATOL, 4 * MEASURED_RTOL, 4 * MEASURED_MEAN_REL
# the printed digits of BT.2100 / BT.2408: half a unit of the last one
PIN_SIGNAL_TOL, PIN_LIGHT_TOL = 5e-5, 0.5


def pins():
    with open(os.path.join(_HERE, "golden", "itp_pins.json")) as f:
        return json.load(f)


def _yuv_of_rgb(rgb, bits):
    """R'G'B' in [0, 1] -> limited-range BT.2020 NCL sample values"""
    s = 1 << (bits - 8)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = 0.2627 * r + 0.6780 * g + 0.0593 * b
    u, v = (b - y) / 1.8814, (r - y) / 1.4746
    return (np.rint(16 * s + 219 * s * y).astype(np.int64), np.rint(128 * s + 224 * s * u).astype(np.int64), np.rint(128 * s + 224 * s * v).astype(np.int64))


def pair(w, h, bits, kind, seed=0):
    """((Y, Cb, Cr), (Y, Cb, Cr)) sample values (int64, depth `bits`):
      noise         independent uniform samples over the whole code range on both sides: sub-black and super-white codes, colours far
                    outside the gamut (the clamp)
      primaries     every chroma cell one of the eight corners of the BT.2020 R'G'B' cube; the other side another corner in half of them
      near_neutral  chroma within two 8-bit codes of neutral, luma anywhere in range; the other side off by up to one 8-bit code
      near_black    luma and the other side's luma in codes 16 s .. 20 s (64 .. 80 at 10 bits), chroma near neutral
      near_peak     luma from reference white to the largest code, moderate chroma
      quadrant      four flat colours; the distorted side moves one quadrant's chroma and another's luma
      one_code      a natural-range picture against itself with ONE plane (seed % 3) moved by one code everywhere"""
    rng = np.random.default_rng([0x17B, seed, w, h, bits, KINDS.index(kind)])
    M, s = (1 << bits) - 1, 1 << (bits - 8)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    ys, cs = (h, w), (ch, cw)
    if kind == "noise":
        ref = tuple(rng.integers(0, M + 1, sh) for sh in (ys, cs, cs))
        dis = tuple(rng.integers(0, M + 1, sh) for sh in (ys, cs, cs))
    elif kind == "primaries":
        corners = np.array([[(i >> 2) & 1, (i >> 1) & 1, i & 1] for i in range(8)], np.float64)
        ia = rng.integers(0, 8, cs)
        ib = np.where(rng.integers(0, 2, cs) == 0, ia, rng.integers(0, 8, cs))
        up = lambda c: np.repeat(np.repeat(c, 2, 0), 2, 1)[:h, :w]
        a, b = _yuv_of_rgb(corners[ia], bits), _yuv_of_rgb(corners[ib], bits)
        ref = (up(a[0]), a[1], a[2])
        dis = (np.clip(up(b[0]) + rng.integers(-s, s + 1, ys), 0, M), b[1], b[2])
    elif kind == "near_neutral":
        ref = (rng.integers(16 * s, 236 * s, ys), 128 * s + rng.integers(-2 * s, 2 * s + 1, cs), 128 * s + rng.integers(-2 * s, 2 * s + 1, cs))
        dis = tuple(np.clip(p + rng.integers(-s, s + 1, p.shape), 0, M) for p in ref)
    elif kind == "near_black":
        ref = (rng.integers(16 * s, 20 * s + 1, ys), 128 * s + rng.integers(-s, s + 1, cs), 128 * s + rng.integers(-s, s + 1, cs))
        dis = (rng.integers(16 * s, 20 * s + 1, ys), ref[1] + rng.integers(-s, s + 1, cs), ref[2] + rng.integers(-s, s + 1, cs))
    elif kind == "near_peak":
        ref = (rng.integers(230 * s, M + 1, ys), 128 * s + rng.integers(-16 * s, 16 * s + 1, cs), 128 * s + rng.integers(-16 * s, 16 * s + 1, cs))
        dis = (rng.integers(230 * s, M + 1, ys), ref[1] + rng.integers(-2 * s, 2 * s + 1, cs), ref[2] + rng.integers(-2 * s, 2 * s + 1, cs))
    elif kind == "quadrant":
        y, x = np.indices(ys)
        q = 2 * (y >= h // 2) + (x >= w // 2)
        cy, cx = np.indices(cs)
        qc = 2 * (2 * cy >= h // 2) + (2 * cx >= w // 2)
        col = np.array([(60, 100, 160), (120, 150, 110), (180, 90, 90), (200, 170, 140)]) * s
        ref = (col[q, 0], col[qc, 1], col[qc, 2])
        dis = (ref[0] + np.where(q == 1, 9 * s, 0), ref[1] + np.where(qc == 2, 7 * s, 0), ref[2] - np.where(qc == 2, 5 * s, 0))
    elif kind == "one_code":
        ref = (rng.integers(16 * s, 236 * s, ys), 128 * s + rng.integers(-40 * s, 40 * s + 1, cs), 128 * s + rng.integers(-40 * s, 40 * s + 1, cs))
        dis = tuple(p + (1 if k == seed % 3 else 0) for k, p in enumerate(ref))
    else:
        raise ValueError(kind)
    return tuple(np.asarray(p, np.int64) for p in ref), tuple(np.asarray(p, np.int64) for p in dis)


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


_emul = None


def emul_lib():
    global _emul
    if _emul is None:
        L = C.CDLL(build_emul())
        assert L.ie_desc_size() == C.sizeof(_Desc)
        for f in (L.ie_log2, L.ie_exp2, L.ie_pq_eotf, L.ie_pq_inv):
            f.argtypes, f.restype = [C.c_void_p, C.c_void_p, C.c_uint], None
        L.ie_pow.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
        L.ie_hlg_display.argtypes, L.ie_hlg_display.restype = [C.c_void_p, C.c_void_p], None
        L.ie_run.argtypes = [C.c_uint, C.c_uint, C.c_int, C.c_uint, C.c_int, C.c_uint, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                             C.c_void_p]
        _emul = L
    return _emul


def tile():
    """(TW, TH): luma positions per tile edge"""
    L = emul_lib()
    return int(L.ie_tile_w()), int(L.ie_tile_h())


def shapes():
    """the sizes the issue names: the smallest, odd ones, the tile's width and height at -1, 0 and +1, and one picture of more than
    one tile each way, odd both ways"""
    tw, th = tile()
    return ((2, 2), (3, 3), (17, 9), (tw - 1, th + 1), (tw, th), (tw + 1, th - 1), (259, 37))


def geom(w, h, layout, bits):
    """workgroups per slot, or None where the library refuses"""
    out = (C.c_ulonglong * 1)()
    if emul_lib().ie_geom(w, h, LAYOUT.get(layout, layout), bits, out):
        return None
    return int(out[0])


def _vec(fn, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    fn(x.ctypes.data, out.ctypes.data, x.size)
    return out


def kernel_log2(x):
    return _vec(emul_lib().ie_log2, x)


def kernel_exp2(x):
    return _vec(emul_lib().ie_exp2, x)


def kernel_pow(x, which):
    """the device's f32 pow(x, POW_EXPONENTS[which])"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    assert emul_lib().ie_pow(x.ctypes.data, int(which), out.ctypes.data, x.size) == 0
    return out


def kernel_pq_eotf(x):
    return _vec(emul_lib().ie_pq_eotf, x)


def kernel_pq_inv(x):
    return _vec(emul_lib().ie_pq_inv, x)


def kernel_hlg_display(rgb):
    x, out = np.array(rgb, np.float32), np.zeros(3, np.float32)
    emul_lib().ie_hlg_display(x.ctypes.data, out.ctypes.data)
    return out


def kernel_ictcp(y, u, v, bits=10, transfer="pq"):
    out = np.zeros(3, np.float32)
    assert emul_lib().ie_ictcp(int(y), int(u), int(v), int(bits), TRANSFER[transfer], out.ctypes.data_as(C.c_void_p)) == 0
    return out


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


def frames_of(layout, pairs, w, h, bits, pad=0, dirty=True, aligned=False):
    """[(ref, dis) sample planes] -> [(ref plane arrays, dis plane arrays)] of `layout`"""
    out = []
    for f, pr in enumerate(pairs):
        sides = []
        for side, planes in enumerate(pr):
            arr = layout_planes(layout, planes, w, h, bits, pad=pad, dirty=xpsnr_util.dirt_seed(f, side) if dirty else None)
            if aligned:
                arr = [aligned_copy(p) for p in arr]
            sides.append(arr)
        out.append(tuple(sides))
    return out


def emulate(w, h, layout, bits, batches, frames, transfer="pq", cap=None, vec=None, maps=True):
    """the emulated kernels over pairs: frames = [(ref plane arrays, dis plane arrays)] (frames_of); compute c takes the next
    batches[c] pairs as its slots 0 .. batches[c]-1 of ONE library object with `cap` slots (default: the largest batch), whose buffers
    are reused from compute to compute.  vec=False: the sample-by-sample path everywhere.  -> [(de_sum, de_max, map float32 [h, w] or
    None)] per pair, or None for a geometry the library refuses"""
    L = emul_lib()
    if geom(w, h, layout, bits) is None:
        return None
    n = len(frames)
    assert sum(batches) == n
    desc = (_Desc * (2 * n))()
    keep = []
    for f, pr in enumerate(frames):
        for side, planes in enumerate(pr):
            planes = [p if p.strides[1] == p.itemsize else np.ascontiguousarray(p) for p in planes]
            if len(planes) == 3 and planes[1].strides[0] != planes[2].strides[0]:
                planes[1:] = [np.ascontiguousarray(p) for p in planes[1:]]
            keep.extend(planes)
            d = desc[2 * f + side]
            d.p0, d.p1 = planes[0].ctypes.data, planes[1].ctypes.data
            d.p2 = planes[2].ctypes.data if len(planes) > 2 else None
            d.pitch, d.pitch2 = planes[0].strides[0], planes[1].strides[0]
    res = np.zeros((n, 2), np.float64)
    mp = np.zeros((n, h, w), np.float32) if maps else None
    bt = (C.c_int * len(batches))(*batches)
    rc = L.ie_run(w, h, LAYOUT[layout], bits, TRANSFER[transfer], cap or max(batches), len(batches), C.addressof(bt), C.addressof(desc),
                  -1 if vec is None else int(bool(vec)), res.ctypes.data, mp.ctypes.data if maps else None)
    assert rc == 0, rc
    return [(float(res[i, 0]), float(res[i, 1]), mp[i].copy() if maps else None) for i in range(n)]


def errors(got_map, want):
    """the per-position figures of one picture against its restatement (itp_ref.Want).  No position is skipped.
    -> (largest |got - want| over want < 1, largest |got - want| / want over want >= 1)"""
    got = got_map.astype(np.float64)
    err = np.abs(got - want.map)
    small = want.map < 1.0
    a = float(err[small].max()) if small.any() else 0.0
    r = float((err[~small] / want.map[~small]).max()) if (~small).any() else 0.0
    return a, r


def agrees(got_map, want, atol, rtol):
    """None, or the first position outside |got - want| <= atol + rtol * want"""
    got = got_map.astype(np.float64)
    ok = np.abs(got - want.map) <= atol + rtol * want.map
    if ok.all():
        return None
    y, x = np.argwhere(~ok)[0]
    return f"({x}, {y}): got {got[y, x]!r}, want {want.map[y, x]!r}; {int((~ok).sum())} positions differ"


def mean_rel(got_sum, want):
    if want.de_sum == 0:
        return 0.0 if got_sum == 0 else float("inf")
    return abs(got_sum - want.de_sum) / want.de_sum
