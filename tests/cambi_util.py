"""TEST INFRASTRUCTURE ONLY: pictures for the CAMBI tests and the emulated kernels (tests/cambi_emul/libcambi_emul.so: the SOURCE of
turbo-metrics_amd/csrc/tm_cambi_kernels.h run lane by lane on the CPU).  The plane arrays of the four layouts come from
tests/motion_util.luma_plane, dirty bits included."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np

from tests import motion_util

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_EMUL_DIR = os.path.join(_HERE, "cambi_emul")
_EMUL_LIB = os.path.join(_EMUL_DIR, "libcambi_emul.so")
_EMUL_SRCS = [os.path.join(_EMUL_DIR, "cambi_emul.cpp"), os.path.join(_HERE, "emul", "hip_emul.h")] + [
    os.path.join(_ROOT, "turbo-metrics_amd", "csrc", f) for f in ("tm_cambi_kernels.h", "tm_sample_load.h", "tm_p10.h", "tm_platform.h", "tm_geom.h")]
LAYOUT = {"y8": 0, "y16_msb": 1, "y16_low": 2, "y10_packed": 3}
CASES = motion_util.CASES
luma_plane = motion_util.luma_plane
KINDS = ("noise", "flat", "stairs_lo", "stairs_hi", "mixed")
SIZES = ((32, 32), (33, 47), (64, 64), (129, 67), (200, 96))
WINDOWS = (3, 7, 15, 63)


def picture(w, h, bits, kind, seed=0):
    """one luma plane of sample values (int64, depth `bits`); the 10-bit codes named are those after step 1:
      noise      independent uniform samples over the whole range (the mask is almost empty)
      flat       one value everywhere
      stairs_lo  one-code steps 5 columns wide around code 178 (tvi[1]): steps on either side of the first threshold
      stairs_hi  the same around code 559 (tvi[4]): the right part of the picture is above every threshold
      mixed      stairs_lo with noise in the right half: masked and unmasked pixels in one window"""
    rng = np.random.default_rng([0xCA3B1, seed, w, h, bits])
    M = (1 << bits) - 1
    x = np.indices((h, w))[1]
    unit = (1 << (bits - 10)) if bits > 10 else 1  # one 10-bit code in samples (below 10 bits a sample is 1 or 4 codes)

    def stairs(centre10):
        c = centre10 * unit if bits >= 10 else centre10 >> (10 - bits)
        return np.clip(c + (x // 5 - w // 10 + seed % 3) * unit, 0, M)
    if kind == "noise":
        p = rng.integers(0, M + 1, (h, w), dtype=np.int64)
    elif kind == "flat":
        p = np.full((h, w), int(rng.integers(0, M + 1)), np.int64)
    elif kind == "stairs_lo":
        p = stairs(178)
    elif kind == "stairs_hi":
        p = stairs(559)
    elif kind == "mixed":
        p = stairs(178)
        p[:, w // 2:] = rng.integers(0, M + 1, (h, w - w // 2), dtype=np.int64)
    else:
        raise ValueError(kind)
    return p.astype(np.int64)


def build_emul():
    if os.path.exists(_EMUL_LIB) and all(os.path.getmtime(s) <= os.path.getmtime(_EMUL_LIB) for s in _EMUL_SRCS):
        return _EMUL_LIB
    # the flags tests/emul/emul.py builds the engine's emulated kernels with
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-pthread",
                           "-Wno-unknown-pragmas", "-I", os.path.join(_HERE, "emul"), "-o", _EMUL_LIB, _EMUL_SRCS[0]])
    return _EMUL_LIB


class _Desc(C.Structure):
    _fields_ = [("p", C.c_void_p), ("pitch", C.c_ulonglong), ("vec", C.c_int), ("pad_", C.c_int)]


class _Res(C.Structure):
    _fields_ = [("t", C.c_uint32 * 5), ("n_gt", C.c_uint32 * 5), ("k", C.c_uint32 * 5), ("pad_", C.c_uint32), ("sum_gt", C.c_double * 5)]


def _lib():
    L = C.CDLL(build_emul())
    L.ce_geom.argtypes = [C.c_uint, C.c_uint, C.c_int, C.c_uint, C.c_uint, C.c_double, C.c_double, C.POINTER(C.c_ulonglong)]
    L.ce_run.argtypes = [C.c_uint, C.c_uint, C.c_int, C.c_uint, C.c_uint, C.c_double, C.c_double, C.c_uint, C.c_int, C.POINTER(C.c_int),
                         C.POINTER(_Desc), C.c_int, C.POINTER(_Res), C.c_void_p, C.c_void_p]
    return L


def geom(w, h, layout, bits, window=0, topk=0.6, thr=0.019):
    """the library's geometry, or None for what it refuses"""
    out = (C.c_ulonglong * 19)()
    if _lib().ce_geom(w, h, LAYOUT.get(layout, layout), bits, window, topk, thr, out) != 0:
        return None
    v = [int(x) for x in out]
    return SimpleNamespace(w=v[0:5], h=v[5:10], off=v[10:15], tot=v[15], window=v[16], oc=v[17], band_rows=v[18])


def emulate(w, h, layout, bits, batches, planes, window=0, topk=0.6, thr=0.019, cap=None, vec=None):
    """the emulated kernels over plane arrays (luma_plane): compute c takes the next batches[c] planes as its slots 0 .. batches[c]-1
    of ONE library object with `cap` slots (default: the largest batch), whose buffers are reused from compute to compute.
    vec=False: the sample-by-sample path everywhere.  -> per plane a namespace with mask[s], plane[s], cmap[s], t, n_gt, k, sum_gt
    (lists over the scales), or None for a geometry the library refuses"""
    L = _lib()
    assert L.ce_desc_size() == C.sizeof(_Desc) and L.ce_res_size() == C.sizeof(_Res)
    g = geom(w, h, layout, bits, window, topk, thr)
    if g is None:
        return None
    n = len(planes)
    assert sum(batches) == n
    desc = (_Desc * n)()
    keep = []
    for f, p in enumerate(planes):
        if p.strides[1] != p.itemsize:
            p = np.ascontiguousarray(p)
        keep.append(p)
        desc[f].p, desc[f].pitch = p.ctypes.data, p.strides[0]
    res = (_Res * n)()
    q = np.zeros((n, g.tot), np.uint16)
    cv = np.zeros((n, g.tot), np.float32)
    bt = (C.c_int * len(batches))(*batches)
    rc = L.ce_run(w, h, LAYOUT.get(layout, layout), bits, window, topk, thr, cap or max(batches), len(batches), bt, desc,
                  -1 if vec is None else int(bool(vec)), res, q.ctypes.data_as(C.c_void_p), cv.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    out = []
    for f in range(n):
        r = SimpleNamespace(window=g.window, mask=[], plane=[], cmap=[], t=list(res[f].t), n_gt=list(res[f].n_gt), k=list(res[f].k),
                            sum_gt=list(res[f].sum_gt))
        for s in range(5):
            a, m = g.off[s], g.w[s] * g.h[s]
            qs = q[f, a:a + m].reshape(g.h[s], g.w[s])
            r.mask.append((qs >> 15) != 0)
            r.plane.append((qs & 0x7FFF).astype(np.int64))
            r.cmap.append(cv[f, a:a + m].reshape(g.h[s], g.w[s]).copy())
        out.append(r)
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


def same(got, want, scales=range(5)):
    """a computed picture (emulated or from the library) against the restatement: planes, masks and c-values exactly, t, n_gt and k
    exactly, sum_gt within w_s h_s 2^-53 relative of math.fsum -- the bound of a naive f64 sum of that many non-negative terms"""
    for s in scales:
        if getattr(got, "mask", None):
            assert (got.mask[s] == want.mask[s]).all(), ("mask", s)
            assert (got.plane[s] == want.plane[s]).all(), ("plane", s)
        assert got.cmap[s].dtype == np.float32 and got.cmap[s].shape == want.cmap[s].shape
        bad = np.flatnonzero(got.cmap[s].view(np.uint32) != want.cmap[s].view(np.uint32))
        assert bad.size == 0, ("cmap", s, bad[:8], got.cmap[s].ravel()[bad[:8]], want.cmap[s].ravel()[bad[:8]])
        assert (got.t[s], got.n_gt[s], got.k[s]) == (want.t[s], want.n_gt[s], want.k[s]), ("pool", s)
        n = want.cmap[s].size
        assert abs(got.sum_gt[s] - want.sum_gt[s]) <= n * 2.0 ** -53 * want.sum_gt[s], ("sum_gt", s, got.sum_gt[s], want.sum_gt[s])
    return True
