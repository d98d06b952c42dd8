"""ctypes binding of include/turbo_metrics_yuv.h (libturbometrics_yuv.so, built in-tree): plane-wise PSNR and x264 / ffmpeg SSIM of
4:2:0 pictures on the MI355X.  A prototype table of its own (ffi.SYMBOLS is the engine's); loaded on first use.
Raises if the library is missing: there is no CPU path.

    y = Yuv(1920, 1080, "nv12", 8, batch=8)
    y.set_pair(0, (y, uv), (y2, uv2)); ...; y.compute(n); y.frames(n)  -> [YuvFrame(sse=(y, u, v), ssim=(..), ssim_sum=(..))]
    y.ssim_map(slot, plane)  -> the (bh - 1) x (bw - 1) float32 window values
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import ffi, synth
from .engine import _ptr_and_mem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libturbometrics_yuv.so")

LAYOUTS = {"nv12": 0, "p016": 1, "i420": 2, "i420p10": 3}


class YuvFrameC(C.Structure):
    _fields_ = [("sse", C.c_uint64 * 3), ("ssim", C.c_double * 3), ("ssim_sum", C.c_double * 3)]


_vp, _u32, _i, _sz = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t
SYMBOLS = {
    "tm_yuv_create": (_i, [C.POINTER(_vp), _u32, _u32, _i, _u32, _u32]),
    "tm_yuv_destroy": (None, [_vp]),
    "tm_yuv_mem_usage": (_sz, [_vp]),
    "tm_yuv_set_frame": (_i, [_vp, _u32, _i, _vp, _vp, _vp, _sz, _sz, _i]),
    "tm_yuv_compute_async": (_i, [_vp, _u32]),
    "tm_yuv_sync": (_i, [_vp]),
    "tm_yuv_get": (_i, [_vp, _u32, _u32, C.POINTER(YuvFrameC)]),
    "tm_yuv_get_ssim_map": (_i, [_vp, _u32, _i, _vp, _sz]),
    "tm_yuv_psnr": (C.c_double, [C.c_uint64, C.c_uint64, _u32, C.c_double]),
    "tm_yuv_ssim_db": (C.c_double, [C.c_double]),
    "tm_yuv_ssim_all": (C.c_double, [C.POINTER(C.c_double), _u32, _u32]),
    "tm_yuv_map_size": (_i, [_u32, _u32, _i, C.POINTER(_u32), C.POINTER(_u32)]),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`.  There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class YuvError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed: code {code}")
        self.code = code


def _chk(rc, what):
    if rc != ffi.TM_OK:
        raise YuvError(rc, what)


class YuvFrame(NamedTuple):
    sse: tuple       # (Y, Cb, Cr) sums of squared differences
    ssim: tuple      # (Y, Cb, Cr) mean window value
    ssim_sum: tuple  # (Y, Cb, Cr) f64 sums of the window values


class Yuv:
    """Plane-wise SSE and SSIM of `batch` pairs per compute.  layout: "nv12" | "p016" | "i420" | "i420p10" (include/turbo_metrics_yuv.h).
    A picture is the tuple of its planes: (Y, CbCr) for nv12 / p016, (Y, Cb, Cr) otherwise; numpy arrays (copied) or torch tensors
    (device tensors are read in place, pinned host tensors by DMA: both must stay alive until compute returns).
    compute(n) is compute_async(n) then sync(): the two halves let several objects, each on its own stream, be in flight at once."""

    def __init__(self, w, h, layout="nv12", bits=8, batch=1):
        self._L = lib()
        self.w, self.h, self.bits, self.batch = int(w), int(h), int(bits), int(batch)
        self.layout = layout
        h_ = C.c_void_p()
        _chk(self._L.tm_yuv_create(C.byref(h_), self.w, self.h, LAYOUTS[layout], self.bits, self.batch), "tm_yuv_create")
        self._h = h_
        self._keep = {}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tm_yuv_destroy(self._h)
        self._h = None
        self._keep = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def mem_usage(self):
        return int(self._L.tm_yuv_mem_usage(self._h))

    def _plane_shapes(self):
        """(rows, elements per row) of each plane of this layout, and the element size in bytes"""
        cw, ch = (self.w + 1) // 2, (self.h + 1) // 2
        if self.layout in ("nv12", "p016"):
            return [(self.h, self.w), (ch, 2 * cw)], 1 if self.layout == "nv12" else 2
        if self.layout == "i420":
            return [(self.h, self.w), (ch, cw), (ch, cw)], 1 if self.bits == 8 else 2
        return [(self.h, synth.p10_row_words(self.w)), (ch, synth.p10_row_words(cw)), (ch, synth.p10_row_words(cw))], 4

    def set_frame(self, slot, side, planes):
        """Checks every plane against the layout before the library sees a pointer: the plane count, the element size (unsigned
        integers; signed 16- and 32-bit ones as views of unsigned data), 2-D shapes of at least the picture's rows x row width, a
        column stride of 1, and one row pitch for Cb and Cr (host numpy planes are copied to one instead).  ValueError otherwise."""
        planes = list(planes)
        shapes, esz = self._plane_shapes()
        if len(planes) != len(shapes):
            raise ValueError(f"{self.layout} takes {len(shapes)} planes, got {len(planes)}")
        for i, (p, (rows, cols)) in enumerate(zip(planes, shapes)):
            if hasattr(p, "data_ptr"):
                size, signed, ok = p.element_size(), p.dtype.is_signed, not (p.dtype.is_floating_point or p.dtype.is_complex
                                                                                   or str(p.dtype) == "torch.bool")
                shape, stride = tuple(p.shape), tuple(p.stride())
            else:
                if not isinstance(p, np.ndarray):
                    raise ValueError(f"plane {i}: a numpy array or a torch tensor, got {type(p).__name__}")
                size, signed, ok = p.itemsize, p.dtype.kind == "i", p.dtype.kind in "ui"
                shape, stride = p.shape, tuple(s // p.itemsize for s in p.strides)
            if not ok or size != esz or (signed and size not in (2, 4)):
                raise ValueError(f"plane {i}: {self.layout} at {self.bits} bits takes {8 * esz}-bit unsigned elements, got {p.dtype}")
            if len(shape) != 2 or shape[0] < rows or shape[1] < cols:
                raise ValueError(f"plane {i}: at least {rows} x {cols} elements, got shape {shape}")
            if stride[1] != 1 or stride[0] < cols:
                raise ValueError(f"plane {i}: rows of contiguous elements are needed, got strides {stride}")
        if len(planes) == 3 and not any(hasattr(p, "data_ptr") for p in planes[1:]) and planes[1].strides[0] != planes[2].strides[0]:
            # one pitch for Cb and Cr (tm_yuv_set_frame takes pitch_uv once): host copies of the rows the picture uses
            planes[1:] = [np.ascontiguousarray(p[:rows, :cols]) for p, (rows, cols) in zip(planes[1:], shapes[1:])]
        planes = [_ptr_and_mem(p) for p in planes]
        mems = {m for _, m, _ in planes}
        if len(mems) != 1:
            raise ValueError("the planes must live in the same kind of memory")
        pitch = lambda k: int(k.stride(0) * k.element_size()) if hasattr(k, "data_ptr") else int(k.strides[0])
        if len(planes) == 3 and pitch(planes[1][2]) != pitch(planes[2][2]):
            raise ValueError("Cb and Cr must have the same row pitch (tm_yuv_set_frame takes pitch_uv once)")
        self._keep[(slot, side)] = [k for _, _, k in planes]
        y, u = planes[0], planes[1]
        v = planes[2] if len(planes) > 2 else (None, None, None)
        _chk(self._L.tm_yuv_set_frame(self._h, slot, side, y[0], u[0], v[0], pitch(y[2]), pitch(u[2]), mems.pop()), "tm_yuv_set_frame")

    def set_pair(self, slot, ref, dis):
        self.set_frame(slot, ffi.TM_SIDE_REF, ref)
        self.set_frame(slot, ffi.TM_SIDE_DIS, dis)

    def compute(self, n):
        """slots [0, n); waits for the result"""
        _chk(self._L.tm_yuv_compute_async(self._h, int(n)), "tm_yuv_compute_async")
        _chk(self._L.tm_yuv_sync(self._h), "tm_yuv_sync")

    def compute_async(self, n):
        """tm_yuv_compute_async: queues slots [0, n) on this object's stream and returns; the planes stay alive until sync()"""
        _chk(self._L.tm_yuv_compute_async(self._h, int(n)), "tm_yuv_compute_async")

    def sync(self):
        """tm_yuv_sync: waits for what compute_async queued"""
        _chk(self._L.tm_yuv_sync(self._h), "tm_yuv_sync")

    def frames(self, n, first=0):
        out = (YuvFrameC * n)()
        _chk(self._L.tm_yuv_get(self._h, int(first), int(n), out), "tm_yuv_get")
        return [YuvFrame(tuple(int(v) for v in f.sse), tuple(float(v) for v in f.ssim), tuple(float(v) for v in f.ssim_sum)) for f in out]

    def samples(self):
        """(n_y, n_u, n_v): the planes' sample counts"""
        nc = ((self.w + 1) // 2) * ((self.h + 1) // 2)
        return (self.w * self.h, nc, nc)

    def ssim_map(self, slot, plane=0):
        """the window values of plane 0 | 1 | 2 of a slot of the last compute: float32 [mh, mw]"""
        if plane not in (0, 1, 2):
            raise ValueError(f"plane 0, 1 or 2, got {plane!r}")
        mw, mh = map_size(self.w, self.h, plane)
        out = np.empty((mh, mw), np.float32)
        _chk(self._L.tm_yuv_get_ssim_map(self._h, int(slot), int(plane), out.ctypes.data_as(C.c_void_p), mw * 4), "tm_yuv_get_ssim_map")
        return out


def psnr(sse, n_samples, bits, cap=0.0):
    """tm_yuv_psnr: 10 log10(max^2 n / sse), inf at sse = 0; cap > 0: the smaller of that and cap"""
    return float(lib().tm_yuv_psnr(int(sse), int(n_samples), int(bits), float(cap)))


def psnr_cap(bits):
    """libvmaf's cap: 6 D + 12"""
    return 6.0 * bits + 12.0


def ssim_db(s):
    return float(lib().tm_yuv_ssim_db(float(s)))


def ssim_all(ssim, w, h):
    return float(lib().tm_yuv_ssim_all((C.c_double * 3)(*[float(v) for v in ssim]), int(w), int(h)))


def map_size(w, h, plane=0):
    """(mw, mh) of a plane's SSIM map"""
    mw, mh = _u32(), _u32()
    _chk(lib().tm_yuv_map_size(int(w), int(h), int(plane), C.byref(mw), C.byref(mh)), "tm_yuv_map_size")
    return int(mw.value), int(mh.value)
