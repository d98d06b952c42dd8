"""TEST INFRASTRUCTURE ONLY: pictures and tolerances of the CIEDE2000 tests and the emulated kernels (tests/ciede_emul/libciede_emul.so:
the SOURCE of turbo-metrics_amd/csrc/tm_ciede_kernels.h run lane by lane on the CPU).  The plane arrays of the four layouts come from
tests/xpsnr_util.layout_planes, dirty bits included."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

from tests import ciede_ref as R
from tests import xpsnr_util

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_EMUL_DIR = os.path.join(_HERE, "ciede_emul")
_EMUL_LIB = os.path.join(_EMUL_DIR, "libciede_emul.so")
_EMUL_SRCS = [os.path.join(_EMUL_DIR, "ciede_emul.cpp"), os.path.join(_HERE, "emul", "hip_emul.h")] + [
    os.path.join(_ROOT, "turbo-metrics_amd", "csrc", f) for f in ("tm_ciede_kernels.h", "tm_sample_load.h", "tm_p10.h", "tm_platform.h", "tm_geom.h")]
LAYOUT = {"nv12": 0, "p016": 1, "i420": 2, "i420p10": 3}
MATRIX = {"bt709": 0, "bt601": 1, "libvmaf": 2}
layout_planes = xpsnr_util.layout_planes
# every layout at the depths it carries
CASES = (("nv12", 8), ("p016", 10), ("p016", 12), ("p016", 16), ("i420", 8), ("i420", 10), ("i420", 12), ("i420", 16), ("i420p10", 10))
KINDS = ("noise", "primaries", "near_neutral", "near_black", "near_peak", "quadrant", "hue_sweep")

# ---- tolerances: measured, not chosen ---------------------------------------------------------------------------------------------
# A position agrees when |got - want| <= ATOL + RTOL * want against the float64 restatement.  The two figures are measured by
# tests/test_ciede_cpu.py::test_emulation_against_restatement over every shape, CASE and KIND (it prints them): MEASURED_ATOL is the
# largest |got - want| over the positions with want < 1, MEASURED_RTOL the largest |got - want| / want over those with want >= 1, so
# that every measured position lies inside MEASURED_ATOL + MEASURED_RTOL * want.  MEASURED_MEAN_REL is the largest relative error of
# de_mean.  The tolerances are 4 times those (this project's margin, tests/hvs_util.py).  *_CPU: the emulated kernel, the host's libm
# standing in for the device's powf / cbrtf / atan2f / expf / sinf / cosf; *_GPU: the library on an MI355X against the same
# restatement (tests/test_gpu_ciede.py::test_library_against_restatement prints them).  Where the GPU's figure is the larger one, the
# GPU tolerance is 4 times the GPU's.
MEASURED_ATOL_CPU = 1.4e-4       # (a neutral colour against another: a', b' are rounding noise of 500 (f(X) - f(Y)))
MEASURED_RTOL_CPU = 5.4e-4       # (a neutral colour against a saturated one: the hue of the neutral side is noise in f32 AND in f64, and R_T dC' dH' carries it)
MEASURED_MEAN_REL_CPU = 4.0e-5
MEASURED_ATOL_GPU = 1.4e-4       # (1.369e-4: i420 / p016 at 16 bits)
MEASURED_RTOL_GPU = 3.5e-4       # (3.413e-4: likewise)
MEASURED_MEAN_REL_GPU = 3.4e-5   # (3.396e-5: 12 bits); none exceeds the CPU's figure: the GPU tolerance is the CPU's
ATOL, RTOL, MEAN_REL_TOL = 4 * MEASURED_ATOL_CPU, 4 * MEASURED_RTOL_CPU, 4 * MEASURED_MEAN_REL_CPU
_g = lambda gpu, cpu: 4 * max(cpu, gpu if gpu is not None else 0.0)
ATOL_GPU, RTOL_GPU, MEAN_REL_TOL_GPU = _g(MEASURED_ATOL_GPU, MEASURED_ATOL_CPU), _g(MEASURED_RTOL_GPU, MEASURED_RTOL_CPU), _g(MEASURED_MEAN_REL_GPU, MEASURED_MEAN_REL_CPU)
# the Sharma table: four printed decimals (5e-5) plus the 1e-6 slack observed in float64
SHARMA_TOL = 5.1e-5
# the largest share of positions under the branch flip rule in any picture but the hue sweep (random hues: 2 / 360 = 0.6 %)
NEAR_SHARE = 0.02


def sharma():
    """the 34 published pairs: rows of L1 a1 b1 L2 a2 b2 dE00"""
    with open(os.path.join(_HERE, "golden", "ciede_sharma.json")) as f:
        return np.array(json.load(f)["rows"], np.float64)


def _yuv_of_rgb(rgb, bits):
    """R'G'B' in [0, 1] -> limited-range BT.709 sample values"""
    s = 1 << (bits - 8)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = 0.2126 * r + 0.7152 * g + 0.0722 * b
    u, v = (b - y) / 1.8556, (r - y) / 1.5748
    return (np.rint(16 * s + 219 * s * y).astype(np.int64), np.rint(128 * s + 224 * s * u).astype(np.int64), np.rint(128 * s + 224 * s * v).astype(np.int64))


def pair(w, h, bits, kind, seed=0):
    """((Y, Cb, Cr), (Y, Cb, Cr)) sample values (int64, depth `bits`):
      noise         independent uniform samples over the whole code range on both sides (far outside the gamut too: nothing clamps)
      primaries     every chroma cell one of the eight corners of the R'G'B' cube; the other side another corner in half of the cells
      near_neutral  chroma within two 8-bit codes of neutral, luma anywhere in range; the other side off by up to one 8-bit code
      near_black    luma from code 0 to just above black, chroma near neutral: the linear branches of the sRGB curve and of f(t)
      near_peak     luma from reference white to the largest code, moderate chroma
      quadrant      four flat colours; the distorted side moves one quadrant's chroma and another's luma
      hue_sweep     a saturated hue that turns along x against its opposite turned by -60 .. +60 degrees along y: |h'1 - h'2| passes 180"""
    rng = np.random.default_rng([0xC1ED, seed, w, h, bits, KINDS.index(kind)])
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
        ref = (rng.integers(0, 21 * s, ys), 128 * s + rng.integers(-4 * s, 4 * s + 1, cs), 128 * s + rng.integers(-4 * s, 4 * s + 1, cs))
        dis = (rng.integers(0, 21 * s, ys), ref[1] + rng.integers(-s, s + 1, cs), ref[2] + rng.integers(-s, s + 1, cs))
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
    elif kind == "hue_sweep":
        cy, cx = np.indices(cs)
        th = 2 * np.pi * (cx + 0.37 * cy + seed) / max(cw, 8)
        dl = np.pi + np.radians(60.0) * (2 * (cy + 0.5) / ch - 1) + np.radians(3.0) * rng.standard_normal(cs)
        A = 70 * s
        ref = (np.full(ys, 126 * s) + rng.integers(-8 * s, 8 * s + 1, ys), np.rint(128 * s + A * np.cos(th)).astype(np.int64), np.rint(128 * s + A * np.sin(th)).astype(np.int64))
        dis = (np.full(ys, 126 * s) + rng.integers(-8 * s, 8 * s + 1, ys), np.rint(128 * s + A * np.cos(th + dl)).astype(np.int64),
               np.rint(128 * s + A * np.sin(th + dl)).astype(np.int64))
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
        assert L.ce_desc_size() == C.sizeof(_Desc)
        L.ce_de00.restype = C.c_float
        L.ce_de00.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float]
        L.ce_run.argtypes = [C.c_uint, C.c_uint, C.c_int, C.c_uint, C.c_int, C.c_double, C.c_double, C.c_double, C.c_uint, C.c_int, C.c_void_p,
                             C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _emul = L
    return _emul


def tile():
    """(TW, TH): luma positions per tile edge"""
    L = emul_lib()
    return int(L.ce_tile_w()), int(L.ce_tile_h())


def shapes():
    """the sizes the issue names, from the kernel's tile: the smallest, odd ones, the tile's width and height at -1, 0 and +1, and
    one picture of several workgroups in both directions"""
    tw, th = tile()
    return ((2, 2), (3, 3), (17, 9), (tw - 1, th + 1), (tw, th), (tw + 1, th - 1), (2 * tw + 3, th + 5))


def geom(w, h, layout, bits):
    """workgroups per slot, or None where the library refuses"""
    out = (C.c_ulonglong * 1)()
    if emul_lib().ce_geom(w, h, LAYOUT.get(layout, layout), bits, out):
        return None
    return int(out[0])


def kernel_de00(lab1, lab2, k=(1.0, 1.0, 1.0)):
    """the device function on two Lab triples (f32)"""
    a, b = np.array(lab1, np.float32), np.array(lab2, np.float32)
    return float(emul_lib().ce_de00(a.ctypes.data, b.ctypes.data, k[0], k[1], k[2]))


def kernel_lab(y, u, v, matrix="bt709", bits=8):
    out = np.zeros(3, np.float32)
    assert emul_lib().ce_lab(int(y), int(u), int(v), MATRIX[matrix], int(bits), out.ctypes.data_as(C.c_void_p)) == 0
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


def emulate(w, h, layout, bits, batches, frames, matrix="bt709", k=(1.0, 1.0, 1.0), cap=None, vec=None, maps=True):
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
    rc = L.ce_run(w, h, LAYOUT[layout], bits, MATRIX[matrix], k[0], k[1], k[2], cap or max(batches), len(batches), C.addressof(bt), C.addressof(desc),
                  -1 if vec is None else int(bool(vec)), res.ctypes.data, mp.ctypes.data if maps else None)
    assert rc == 0, rc
    return [(float(res[i, 0]), float(res[i, 1]), mp[i].copy() if maps else None) for i in range(n)]


def errors(got_map, want):
    """the per-position figures of one picture against its restatement (ciede_ref.Want), the branch flip rule applied: where the
    restatement is within NEAR_DEG of opposite hues, the nearer of its two branch values is the one compared with.  No position is
    skipped.  -> (largest |got - want| over want < 1, largest |got - want| / want over want >= 1)"""
    got = got_map.astype(np.float64)
    e0, e1 = np.abs(got - want.map), np.abs(got - want.alt)
    use_alt = want.near & (e1 < e0)
    err = np.where(use_alt, e1, e0)
    ref = np.where(use_alt, want.alt, want.map)
    small = ref < 1.0
    a = float(err[small].max()) if small.any() else 0.0
    r = float((err[~small] / ref[~small]).max()) if (~small).any() else 0.0
    return a, r


def agrees(got_map, want, atol, rtol):
    """None, or the first position outside |got - want| <= atol + rtol * want (under the branch flip rule)"""
    got = got_map.astype(np.float64)
    ok = np.abs(got - want.map) <= atol + rtol * want.map
    ok |= want.near & (np.abs(got - want.alt) <= atol + rtol * want.alt)
    if ok.all():
        return None
    y, x = np.argwhere(~ok)[0]
    return f"({x}, {y}): got {got[y, x]!r}, want {want.map[y, x]!r} (other branch {want.alt[y, x]!r}, near {bool(want.near[y, x])}); {int((~ok).sum())} positions differ"


def mean_rel_map(got_sum, got_map, want):
    """relative error of de_sum against the restatement's sum with every position under the branch flip rule taken at the branch the
    kernel's own map value is nearer to"""
    got = got_map.astype(np.float64)
    use_alt = want.near & (np.abs(got - want.alt) < np.abs(got - want.map))
    s = float(np.where(use_alt, want.alt, want.map).sum())
    if s == 0:
        return 0.0 if got_sum == 0 else float("inf")
    return abs(got_sum - s) / s
