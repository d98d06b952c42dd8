"""TEST INFRASTRUCTURE ONLY: pictures for the YUV PSNR / SSIM tests and the emulated kernels (tests/yuv_emul/libyuv_emul.so: the
SOURCE of turbo-metrics_amd/csrc/tm_yuv_kernels.h run lane by lane on the CPU).  The plane arrays of the four layouts come from
tests/xpsnr_util.layout_planes, dirty bits included."""
import ctypes as C
import os
import subprocess
from typing import NamedTuple

import numpy as np

from tm_pkg import tm
from tests import xpsnr_util
from tests import yuv_ref as R

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_EMUL_DIR = os.path.join(_HERE, "yuv_emul")
_EMUL_LIB = os.path.join(_EMUL_DIR, "libyuv_emul.so")
_EMUL_SRCS = [os.path.join(_EMUL_DIR, "yuv_emul.cpp"), os.path.join(_HERE, "emul", "hip_emul.h")] + [
    os.path.join(_ROOT, "turbo-metrics_amd", "csrc", f) for f in ("tm_yuv_kernels.h", "tm_sample_load.h", "tm_p10.h", "tm_platform.h", "tm_geom.h")]
LAYOUT = tm.yuv.LAYOUTS
layout_planes = xpsnr_util.layout_planes
# every layout at the depths the issue names, where the layout carries them
CASES = (("nv12", 8), ("p016", 10), ("p016", 12), ("p016", 16), ("i420", 8), ("i420", 10), ("i420", 12), ("i420", 16), ("i420p10", 10))
KINDS = ("noise", "smooth", "extreme", "flat")


def pair(w, h, bits, kind, seed=0):
    """((Y, Cb, Cr), (Y, Cb, Cr)) sample values (int64, depth `bits`):
      noise    independent uniform samples over the whole range on both sides
      smooth   a gradient plus a little noise; the distorted side adds a small error to it
      extreme  every sample 0 or 2^D - 1 at random, independently on both sides
      flat     one value per plane and side (the values depend on the seed)"""
    rng = np.random.default_rng([0x9A7, seed, w, h, bits, KINDS.index(kind)])
    M = (1 << bits) - 1
    shapes = ((h, w), ((h + 1) // 2, (w + 1) // 2), ((h + 1) // 2, (w + 1) // 2))

    def one(sh, side, ref=None):
        if kind == "noise":
            return rng.integers(0, M + 1, sh, dtype=np.int64)
        if kind == "extreme":
            return rng.integers(0, 2, sh, dtype=np.int64) * M
        if kind == "flat":
            return np.full(sh, int(rng.integers(0, M + 1)), np.int64)
        if side == 0:
            y, x = np.indices(sh)
            return ((x * 7 + y * 3 + seed * 11) * max(1, M // 255) + rng.integers(0, max(1, M // 32), sh)) % (M + 1)
        return np.clip(ref + rng.integers(-max(1, M // 64), max(1, M // 64) + 1, sh), 0, M)
    ref = tuple(one(sh, 0).astype(np.int64) for sh in shapes)
    dis = tuple(one(sh, 1, r).astype(np.int64) for sh, r in zip(shapes, ref))
    return ref, dis


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


class _Res(C.Structure):
    _fields_ = [("sse", C.c_uint64 * 3), ("ssim_sum", C.c_double * 3)]


def tile():
    """windows per tile edge"""
    return int(C.CDLL(build_emul()).ye_tile())


def constants(bits):
    c = (C.c_longlong * 2)()
    C.CDLL(build_emul()).ye_constants(bits, c)
    return int(c[0]), int(c[1])


def geom(w, h, layout, bits):
    """(floats of a slot's maps, the three planes' offsets, workgroups per slot, cells per slot), or None where the library refuses"""
    out = (C.c_ulonglong * 6)()
    if C.CDLL(build_emul()).ye_geom(w, h, LAYOUT.get(layout, layout), bits, out):
        return None
    return int(out[0]), (int(out[1]), int(out[2]), int(out[3])), int(out[4]), int(out[5])


class Got(NamedTuple):
    sse: tuple       # per plane
    maps: list       # per plane float32 [mh, mw]
    ssim_sum: tuple  # per plane


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


def split_maps(w, h, flat):
    """one slot's maps -> the three planes' [mh, mw] arrays"""
    out, o = [], 0
    for p in range(3):
        pw, ph = (w, h) if p == 0 else ((w + 1) // 2, (h + 1) // 2)
        mw, mh = (pw >> 2) - 1, (ph >> 2) - 1
        out.append(flat[o:o + mw * mh].reshape(mh, mw).copy())
        o += mw * mh
    assert o == flat.size
    return out


def emulate(w, h, layout, bits, batches, frames, cap=None, vec=None):
    """the emulated kernels over pairs: frames = [(ref plane arrays, dis plane arrays)] (layout_planes); compute c takes the next
    batches[c] pairs as its slots 0 .. batches[c]-1 of ONE library object with `cap` slots (default: the largest batch), whose buffers
    are reused from compute to compute.  vec=False: the sample-by-sample path everywhere.  -> [Got] per pair, or None for a geometry the
    library refuses"""
    L = C.CDLL(build_emul())
    assert L.ye_desc_size() == C.sizeof(_Desc) and L.ye_res_size() == C.sizeof(_Res)
    gm = geom(w, h, layout, bits)
    if gm is None:
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
    res = (_Res * n)()
    maps = np.zeros((n, gm[0]), np.float32)
    bt = (C.c_int * len(batches))(*batches)
    rc = L.ye_run(w, h, LAYOUT[layout], bits, cap or max(batches), len(batches), bt, desc, -1 if vec is None else int(bool(vec)), res,
                  maps.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return [Got(tuple(int(v) for v in res[i].sse), split_maps(w, h, maps[i]), tuple(float(v) for v in res[i].ssim_sum)) for i in range(n)]


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


def agrees(got, want):
    """the required agreement of one pair with the restatement: sse equal, every map value bit-identical, ssim_sum within the derived
    bound (yuv_ref.sum_bound) of the exactly rounded sum.  -> None, or what differs"""
    for p in range(3):
        if got.sse[p] != want[p].sse:
            return f"plane {p}: sse {got.sse[p]} != {want[p].sse}"
        if got.maps[p].shape != want[p].map.shape or not np.array_equal(got.maps[p].view(np.uint32), want[p].map.view(np.uint32)):
            return f"plane {p}: map differs"
        if not abs(got.ssim_sum[p] - want[p].ssim_sum) <= R.sum_bound(want[p]):
            return f"plane {p}: ssim_sum {got.ssim_sum[p]!r} vs {want[p].ssim_sum!r}, bound {R.sum_bound(want[p])!r}"
    return None
