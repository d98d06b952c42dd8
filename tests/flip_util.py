"""TEST INFRASTRUCTURE ONLY: pictures for the FLIP tests, the emulated kernels (tests/flip_emul/libflip_emul.so: the SOURCE of
turbo-metrics_amd/csrc/tm_flip_kernels.h run lane by lane on the CPU) and the tolerances both tiers hold the kernels to."""
import ctypes as C
import functools
import os
import subprocess
from types import SimpleNamespace

import numpy as np

from tests import flip_ref

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_EMUL_DIR = os.path.join(_HERE, "flip_emul")
_EMUL_LIB = os.path.join(_EMUL_DIR, "libflip_emul.so")
_EMUL_SRCS = [os.path.join(_EMUL_DIR, "flip_emul.cpp"), os.path.join(_HERE, "emul", "hip_emul.h")] + [
    os.path.join(_ROOT, "turbo-metrics_amd", "csrc", f) for f in ("tm_flip_kernels.h", "tm_device_math.h", "tm_math_tables.inc", "tm_platform.h")]
DEFAULT_PPD = flip_ref.DEFAULT_PPD
KINDS = ("noise", "step", "pixel", "dark", "smooth")

# The conditions of the definition's text: the square root of step 5 turns f32 noise of 1e-7 into about 3e-4 of dEf, and step 6 passes at
# most |c ln c| <= 0.37 of that on.  The figures MEASURED on the CPU (emulation against the float64 restatement, every shape and kind of
# tests/test_flip_cpu.py) times the margin of 4 for the device's exp2f / log2f / sqrtf are DESIGN.md section 14's; the tests assert both.
COND_PIXEL, COND_MEAN = 2e-3, 1e-4
# measured (test_emulation_against_the_restatement prints them): 1.097e-4 per pixel over the three maps, 6.65e-7 on the mean -> x 4
TOL_PIXEL, TOL_MEAN = 4.4e-4, 2.7e-6
assert TOL_PIXEL <= COND_PIXEL and TOL_MEAN <= COND_MEAN


def pair(w, h, kind, seed=0):
    """(ref, dis): uint8 [h][w][3]
      noise   independent uniform bytes on both sides
      step    a vertical step edge, sharp in ref, shifted by a column and dimmed in dis
      pixel   a smooth picture, dis differs in ONE pixel
      dark    values 0 .. 6, dis off by at most one code: e is near 0, the sRGB line segment, the Lab line segment
      smooth  a colour gradient, dis with a little noise on it: small differences everywhere"""
    rng = np.random.default_rng([0xF11B, seed, w, h])
    yy, xx = np.indices((h, w))
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "step":
        a = np.where(xx[..., None] < w // 2, np.array([30, 40, 50]), np.array([220, 200, 180])).astype(np.uint8)
        b = np.where(xx[..., None] < w // 2 + 1, np.array([30, 40, 50]), np.array([200, 200, 190])).astype(np.uint8)
        return a, b
    if kind == "smooth" or kind == "pixel":
        a = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(w + h - 2, 1)], -1).astype(np.uint8)
        if kind == "pixel":
            b = a.copy()
            b[h // 2, w // 2] = 255 - b[h // 2, w // 2]
            return a, b
        return a, np.clip(a.astype(np.int64) + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)
    if kind == "dark":
        a = rng.integers(0, 6, (h, w, 3), dtype=np.uint8)
        return a, (a + rng.integers(0, 2, (h, w, 3), dtype=np.uint8)).astype(np.uint8)
    raise ValueError(kind)


def padded(img, pitch, fill=0xA5):
    """the same picture with rows `pitch` bytes apart, garbage between them: (the [h][w][3] view, the buffer that owns it)"""
    h, w, _ = img.shape
    assert pitch >= 3 * w
    buf = np.full(h * pitch, fill, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (h, w, 3), (pitch, 3, 1))
    view[...] = img
    return view, buf


def build_emul():
    if os.path.exists(_EMUL_LIB) and all(os.path.getmtime(s) <= os.path.getmtime(_EMUL_LIB) for s in _EMUL_SRCS):
        return _EMUL_LIB
    # the flags tests/emul/emul.py builds the engine's emulated kernels with
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-pthread",
                           "-Wno-unknown-pragmas", "-I", os.path.join(_HERE, "emul"), "-o", _EMUL_LIB, _EMUL_SRCS[0]])
    return _EMUL_LIB


class _Desc(C.Structure):
    _fields_ = [("p", C.c_void_p * 2), ("pitch", C.c_ulonglong * 2)]


class _Res(C.Structure):
    _fields_ = [("mean", C.c_double), ("min", C.c_double), ("max", C.c_double)]


@functools.lru_cache(None)
def _lib():
    L = C.CDLL(build_emul())
    L.fe_geom.argtypes = [C.c_uint, C.c_uint, C.c_int, C.c_double, C.POINTER(C.c_double), C.c_void_p]
    L.fe_radius.argtypes = [C.c_double, C.POINTER(C.c_uint)]
    L.fe_run.argtypes = [C.c_uint, C.c_uint, C.c_int, C.c_double, C.c_uint, C.c_int, C.POINTER(C.c_int), C.POINTER(_Desc), C.POINTER(_Res),
                         C.c_void_p]
    assert L.fe_desc_size() == C.sizeof(_Desc) and L.fe_res_size() == C.sizeof(_Res)
    return L


def tile():
    """(T_W, T_H, halo) of the kernel"""
    out = (C.c_uint * 3)()
    _lib().fe_tile(out)
    return tuple(int(x) for x in out)


def emul_radius(ppd):
    out = (C.c_uint * 2)()
    _lib().fe_radius(float(ppd), out)
    return int(out[0]), int(out[1])


def geom(w, h, ppd=DEFAULT_PPD, layout=0):
    """the library's host side: namespace(cmax, ws[4][21], wf[3][21]), or None for what it refuses"""
    cm = C.c_double()
    taps = np.zeros((7, 21), np.float32)
    if _lib().fe_geom(w, h, layout, float(ppd), C.byref(cm), taps.ctypes.data_as(C.c_void_p)) != 0:
        return None
    return SimpleNamespace(cmax=cm.value, ws=taps[:4], wf=taps[4:])


def emulate(w, h, pairs, batches=None, ppd=DEFAULT_PPD, cap=None):
    """the emulated kernels over (ref, dis) pairs of uint8 [h][w][3] arrays (any row stride): compute c takes the next batches[c] pairs
    as its slots of ONE library object with `cap` slots whose buffers are reused.  -> per pair a namespace(flip, color, feature, mean,
    min, max), or None for a geometry the library refuses"""
    L = _lib()
    n = len(pairs)
    batches = batches or [n]
    assert sum(batches) == n
    desc = (_Desc * n)()
    for f, (a, b) in enumerate(pairs):
        for s, p in enumerate((a, b)):
            assert p.dtype == np.uint8 and p.shape == (h, w, 3) and p.strides[1:] == (3, 1)
            desc[f].p[s], desc[f].pitch[s] = p.ctypes.data, p.strides[0] if h > 1 else max(p.strides[0], 3 * w)
    res = (_Res * n)()
    maps = np.zeros((n, 3, h, w), np.float32)
    bt = (C.c_int * len(batches))(*batches)
    rc = L.fe_run(w, h, 0, float(ppd), cap or max(batches), len(batches), bt, desc, res, maps.ctypes.data_as(C.c_void_p))
    if rc == -1:
        return None
    assert rc == 0, rc
    return [SimpleNamespace(flip=maps[f, 0], color=maps[f, 1], feature=maps[f, 2], mean=res[f].mean, min=res[f].min, max=res[f].max)
            for f in range(n)]


def close(got, want, tol_pixel=TOL_PIXEL, tol_mean=TOL_MEAN):
    """a computed pair (emulated or from the library) against the float64 restatement; returns the largest differences (maps, mean)"""
    worst = 0.0
    for name in ("flip", "color", "feature"):
        g, w_ = getattr(got, name), getattr(want, name)
        assert g.dtype == np.float32 and g.shape == w_.shape, name
        d = float(np.abs(g.astype(np.float64) - w_).max())
        assert d <= tol_pixel, (name, d)
        worst = max(worst, d)
    dm = abs(got.mean - want.mean)
    assert dm <= tol_mean, ("mean", got.mean, want.mean)
    assert abs(got.min - want.min) <= tol_pixel and abs(got.max - want.max) <= tol_pixel
    return worst, dm
