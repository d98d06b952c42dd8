"""TEST INFRASTRUCTURE ONLY: pictures and tolerances of the PSNR-HVS tests and the emulated kernels (tests/hvs_emul/libhvs_emul.so:
the SOURCE of turbo-metrics_amd/csrc/tm_hvs_kernels.h run lane by lane on the CPU).  The plane arrays of the four luma layouts come
from tests/motion_util.luma_plane, dirty bits included."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import motion_util

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_EMUL_DIR = os.path.join(_HERE, "hvs_emul")
_EMUL_LIB = os.path.join(_EMUL_DIR, "libhvs_emul.so")
_EMUL_SRCS = [os.path.join(_EMUL_DIR, "hvs_emul.cpp"), os.path.join(_HERE, "emul", "hip_emul.h")] + [
    os.path.join(_ROOT, "turbo-metrics_amd", "csrc", f) for f in ("tm_hvs_kernels.h", "tm_sample_load.h", "tm_p10.h", "tm_platform.h", "tm_geom.h")]
LAYOUT = {"y8": 0, "y16_msb": 1, "y16_low": 2, "y10_packed": 3}
# the four layouts at D = 8, 10, 12, 16 (what each carries)
CASES = (("y8", 8), ("y16_msb", 10), ("y16_msb", 12), ("y16_msb", 16), ("y16_low", 10), ("y16_low", 12), ("y16_low", 16), ("y10_packed", 10))
KINDS = ("noise", "flat_noise", "ramp_one", "quadrant", "checker", "extreme", "near_peak")

# The emulated kernel (every f32 operation the kernel's own) against the float64 restatement: the largest relative error of S2 / S1
# that tests/test_hvs_cpu.py::test_emulation_against_restatement measures over every shape, CASE and KIND is 2.8e-7 / 4.0e-7 (it
# prints both); the tolerance is the larger times 4 (FLIP's margin, for pictures outside the measured set): 1.6e-6.  The condition the issue sets, not a
# measurement: no more than 1e-4 relative (0.0004 dB).
MEASURED_REL = 4.0e-7
REL_TOL = 4 * MEASURED_REL
assert REL_TOL <= 1e-4

luma_plane = motion_util.luma_plane  # sample values -> the plane array of a layout, optionally padded and with dirty bits


def pair(w, h, bits, kind, seed=0):
    """(ref, dis) sample values (int64) of depth `bits`:
      noise       independent uniform samples on both sides
      flat_noise  a flat reference against noise (variance 0 on one side: the pop = 0 branch)
      ramp_one    a ramp, and the same ramp with one pixel per block row off by one code
      quadrant    flat blocks with noise in one quadrant; the distorted side adds a small error everywhere
      checker     a full-amplitude checkerboard against its inverse in the lower half and itself above
      extreme     every sample 0 or 2^D - 1 at random, independently on both sides
      near_peak   a slow ramp just below 2^D - 1, and a copy that differs by one code in a quarter of the samples"""
    rng = np.random.default_rng([0x485, seed, w, h, bits, KINDS.index(kind)])
    M = (1 << bits) - 1
    y, x = np.indices((h, w))
    if kind == "noise":
        ref, dis = rng.integers(0, M + 1, (h, w)), rng.integers(0, M + 1, (h, w))
    elif kind == "flat_noise":
        ref, dis = np.full((h, w), M // 3), rng.integers(0, M + 1, (h, w))
    elif kind == "ramp_one":
        ref = ((x * 5 + y * 3 + seed) * max(1, M // 255)) % (M + 1)
        dis = ref.copy()
        for by in range(0, h, 8):
            px, py = int(rng.integers(0, w)), min(h - 1, by + int(rng.integers(0, 8)))
            dis[py, px] += 1 if dis[py, px] < M else -1
    elif kind == "quadrant":
        ref = np.full((h, w), M // 2)
        q = ((x % 8) < 4) & ((y % 8) >= 4)
        ref = np.where(q, rng.integers(0, M + 1, (h, w)), ref)
        dis = np.clip(ref + rng.integers(-max(1, M // 128), max(1, M // 128) + 1, (h, w)), 0, M)
    elif kind == "checker":
        ref = ((x + y) % 2) * M
        dis = ((x + y + (y >= h // 2)) % 2) * M
    elif kind == "extreme":
        ref, dis = rng.integers(0, 2, (h, w)) * M, rng.integers(0, 2, (h, w)) * M
    elif kind == "near_peak":
        ref = M - ((x + 2 * y) // 4) % 8
        dis = ref - (rng.integers(0, 4, (h, w)) == 0)
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


def emul_lib():
    L = C.CDLL(build_emul())
    assert L.he_desc_size() == C.sizeof(_Desc)
    return L


def tile():
    """(TW, TH): samples per tile edge"""
    L = emul_lib()
    return int(L.he_tile_w()), int(L.he_tile_h())


def shapes():
    """the sizes the issue names, from the kernel's tile"""
    tw, th = tile()
    return ((8, 8), (15, 9), (16, 8), (tw - 8, th + 8), (tw, th), (tw + 8, th - 8), (tw + 1, th + 7))


def kernel_tables():
    """(CSF, MASK) float32 [8, 8] as the kernel source holds them"""
    a, b = np.zeros(64, np.float32), np.zeros(64, np.float32)
    emul_lib().he_tables(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))
    return a.reshape(8, 8), b.reshape(8, 8)


def kernel_dct8(x):
    v = np.array(x, np.float32)
    emul_lib().he_dct8(v.ctypes.data_as(C.c_void_p))
    return v


def geom(w, h, layout, bits):
    """(blocks, cells) per slot, or None where the library refuses"""
    out = (C.c_ulonglong * 2)()
    if emul_lib().he_geom(w, h, LAYOUT.get(layout, layout), bits, out):
        return None
    return int(out[0]), int(out[1])


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


def emulate(w, h, layout, bits, batches, frames, cap=None, vec=None):
    """the emulated kernels over pairs: frames = [(ref plane array, dis plane array)] (luma_plane); compute c takes the next batches[c]
    pairs as its slots 0 .. batches[c]-1 of ONE library object with `cap` slots (default: the largest batch), whose buffers are reused
    from compute to compute.  vec=False: the sample-by-sample path everywhere.  -> [(s_hvs, s_hvsm, blocks)] per pair, or None for a
    geometry the library refuses"""
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
    res = np.zeros((n, 2), np.float64)
    bt = (C.c_int * len(batches))(*batches)
    rc = L.he_run(w, h, LAYOUT[layout], bits, cap or max(batches), len(batches), bt, desc, -1 if vec is None else int(bool(vec)),
                  res.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return [(float(res[i, 0]), float(res[i, 1]), gm[0]) for i in range(n)]


def planes_of(layout, pairs, bits, pad=0, dirty=True, aligned=False):
    """[(ref, dis) sample values] -> [(ref plane array, dis plane array)] of `layout`"""
    out = []
    for f, pr in enumerate(pairs):
        sides = []
        for side, Y in enumerate(pr):
            p = luma_plane(layout, Y, bits, pad=pad, dirty=(1000 + 2 * f + side) if dirty else None)
            sides.append(aligned_copy(p) if aligned else p)
        out.append(tuple(sides))
    return out


# What the float64 restatement itself leaves where the exact value is 0: C X C^T on integers below 2^16 is wrong by up to about
# 64 * 2^-53 * 2^16 = 5e-10 per coefficient, whose weighted square stays below 1e-17 per term and 1e-12 per picture of the sizes tested.
# The smallest S2 of two pictures that differ at all is (0.0975^2 * 0.21)^2 = 4e-6 (one sample off by one code).
REF_FLOOR = 1e-12


def rel_err(got, want):
    """relative error of a sum against the restatement's; 0 where the two differ by no more than the restatement's own floor"""
    if abs(got - want) <= REF_FLOOR:
        return 0.0
    if want == 0:
        return float("inf")
    return abs(got - want) / want
