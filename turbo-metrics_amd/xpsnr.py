"""ctypes binding of include/turbo_metrics_xpsnr.h (libturbometrics_xpsnr.so, built in-tree): XPSNR over sequences of 4:2:0 pictures on
the MI355X.  A prototype table of its own (ffi.SYMBOLS is the engine's); loaded on first use.  Raises if the library is missing: there
is no CPU path.

    x = Xpsnr(1920, 1080, "nv12", 8, fps=(30, 1), batch=8)
    x.set_pair(0, (y, uv), (y2, uv2)); ...; x.compute(n); x.frames(n)  -> [XpsnrFrame(wsse=(y, cb, cr), xpsnr=(y, cb, cr))]
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import ffi, synth
from .engine import _ptr_and_mem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libturbometrics_xpsnr.so")

LAYOUTS = {"nv12": 0, "p016": 1, "i420": 2, "i420p10": 3}


class XpsnrFrameC(C.Structure):
    _fields_ = [("wsse", C.c_uint64 * 3), ("xpsnr", C.c_double * 3)]


_vp, _u32, _i, _sz = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t
SYMBOLS = {
    "tm_xpsnr_create": (_i, [C.POINTER(_vp), _u32, _u32, _i, _u32, _u32, _u32, _u32]),
    "tm_xpsnr_destroy": (None, [_vp]),
    "tm_xpsnr_mem_usage": (_sz, [_vp]),
    "tm_xpsnr_set_frame": (_i, [_vp, _u32, _i, _vp, _vp, _vp, _sz, _sz, _i]),
    "tm_xpsnr_compute_async": (_i, [_vp, _u32]),
    "tm_xpsnr_sync": (_i, [_vp]),
    "tm_xpsnr_get": (_i, [_vp, _u32, _u32, C.POINTER(XpsnrFrameC)]),
    "tm_xpsnr_reset": (_i, [_vp]),
    "tm_xpsnr_block_size": (_u32, [_u32, _u32]),
    "tm_xpsnr_from_wsse": (C.c_double, [C.c_uint64, _u32, _u32, _u32]),
    "tm_xpsnr_sequence": (C.c_double, [C.c_double, C.c_double, C.c_uint64, _u32, _u32, _u32]),
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


class XpsnrError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed: code {code}")
        self.code = code


def _chk(rc, what):
    if rc != ffi.TM_OK:
        raise XpsnrError(rc, what)


class XpsnrFrame(NamedTuple):
    wsse: tuple   # (Y, Cb, Cr) rounded weighted SSE
    xpsnr: tuple  # (Y, Cb, Cr) dB, inf when the weighted SSE is 0


class Xpsnr:
    """XPSNR of one sequence, `batch` pictures per compute.  layout: "nv12" | "p016" | "i420" | "i420p10" (include/turbo_metrics_xpsnr.h).
    A picture is the tuple of its planes: (Y, CbCr) for nv12 / p016, (Y, Cb, Cr) otherwise; numpy arrays (copied) or torch tensors
    (device tensors are read in place, pinned host tensors by DMA: both must stay alive until compute returns).
    compute(n) is compute_async(n) then sync(): the two halves let several objects, each on its own stream, be in flight at once."""

    def __init__(self, w, h, layout="nv12", bits=8, fps=(25, 1), batch=1):
        self._L = lib()
        self.w, self.h, self.bits, self.batch = int(w), int(h), int(bits), int(batch)
        self.layout = layout
        h_ = C.c_void_p()
        _chk(self._L.tm_xpsnr_create(C.byref(h_), self.w, self.h, LAYOUTS[layout], self.bits, int(fps[0]), int(fps[1]), self.batch),
             "tm_xpsnr_create")
        self._h = h_
        self._keep = {}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tm_xpsnr_destroy(self._h)
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
        return int(self._L.tm_xpsnr_mem_usage(self._h))

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
            # one pitch for Cb and Cr (tm_xpsnr_set_frame takes pitch_uv once): host copies of the rows the picture uses
            planes[1:] = [np.ascontiguousarray(p[:rows, :cols]) for p, (rows, cols) in zip(planes[1:], shapes[1:])]
        planes = [_ptr_and_mem(p) for p in planes]
        mems = {m for _, m, _ in planes}
        if len(mems) != 1:
            raise ValueError("the planes must live in the same kind of memory")
        pitch = lambda k: int(k.stride(0) * k.element_size()) if hasattr(k, "data_ptr") else int(k.strides[0])
        if len(planes) == 3 and pitch(planes[1][2]) != pitch(planes[2][2]):
            raise ValueError("Cb and Cr must have the same row pitch (tm_xpsnr_set_frame takes pitch_uv once)")
        self._keep[(slot, side)] = [k for _, _, k in planes]
        y, u = planes[0], planes[1]
        v = planes[2] if len(planes) > 2 else (None, None, None)
        _chk(self._L.tm_xpsnr_set_frame(self._h, slot, side, y[0], u[0], v[0], pitch(y[2]), pitch(u[2]), mems.pop()), "tm_xpsnr_set_frame")

    def set_pair(self, slot, ref, dis):
        self.set_frame(slot, ffi.TM_SIDE_REF, ref)
        self.set_frame(slot, ffi.TM_SIDE_DIS, dis)

    def compute(self, n):
        """slots [0, n) continue the sequence; waits for the result"""
        _chk(self._L.tm_xpsnr_compute_async(self._h, int(n)), "tm_xpsnr_compute_async")
        _chk(self._L.tm_xpsnr_sync(self._h), "tm_xpsnr_sync")

    def compute_async(self, n):
        """tm_xpsnr_compute_async: queues slots [0, n) on this object's stream and returns; the planes stay alive until sync()"""
        _chk(self._L.tm_xpsnr_compute_async(self._h, int(n)), "tm_xpsnr_compute_async")

    def sync(self):
        """tm_xpsnr_sync: waits for what compute_async queued"""
        _chk(self._L.tm_xpsnr_sync(self._h), "tm_xpsnr_sync")

    def frames(self, n, first=0):
        out = (XpsnrFrameC * n)()
        _chk(self._L.tm_xpsnr_get(self._h, int(first), int(n), out), "tm_xpsnr_get")
        return [XpsnrFrame(tuple(int(v) for v in f.wsse), tuple(float(v) for v in f.xpsnr)) for f in out]

    def reset(self):
        _chk(self._L.tm_xpsnr_reset(self._h), "tm_xpsnr_reset")


def block_size(w, h):
    return int(lib().tm_xpsnr_block_size(int(w), int(h)))


def from_wsse(wsse, pw, ph, bits):
    return float(lib().tm_xpsnr_from_wsse(int(wsse), int(pw), int(ph), int(bits)))


def sequence(sum_sqrt_wsse, sum_xpsnr, n_frames, pw, ph, bits):
    return float(lib().tm_xpsnr_sequence(float(sum_sqrt_wsse), float(sum_xpsnr), int(n_frames), int(pw), int(ph), int(bits)))
