"""ctypes binding of include/turbo_metrics_siti.h (libturbometrics_siti.so, built in-tree): ITU-T P.910 spatial / temporal information
over the luma planes of one sequence on the MI355X.  A prototype table of its own (ffi.SYMBOLS is the engine's); loaded on first use.
Raises if the library is missing: there is no CPU path.

    m = Siti(1920, 1080, "y8", 8, batch=8)
    m.set_frame(0, y); ...; m.compute(n); m.frames(n)  -> [SitiFrame(s1, s2, t1, t2, ti_valid, si, ti)]
    si(s1, s2, n_si, gain), ti(t1, t2, n, bits, gain): the library's host functions; sequence SI / TI are the maxima over the frames
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import ffi, synth
from .engine import _ptr_and_mem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libturbometrics_siti.so")

LAYOUTS = {"y8": 0, "y16_msb": 1, "y16_low": 2, "y10_packed": 3}


class SitiFrameC(C.Structure):
    _fields_ = [("s1", C.c_uint64), ("s2", C.c_uint64), ("t1", C.c_int64), ("t2", C.c_uint64), ("ti_valid", C.c_int), ("si", C.c_double), ("ti", C.c_double)]


_vp, _u32, _i, _sz = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t
SYMBOLS = {
    "tm_siti_create": (_i, [C.POINTER(_vp), _u32, _u32, _i, _u32, _u32]),
    "tm_siti_destroy": (None, [_vp]),
    "tm_siti_mem_usage": (_sz, [_vp]),
    "tm_siti_set_frame": (_i, [_vp, _u32, _vp, _sz, _i]),
    "tm_siti_compute_async": (_i, [_vp, _u32]),
    "tm_siti_sync": (_i, [_vp]),
    "tm_siti_get": (_i, [_vp, _u32, _u32, C.POINTER(SitiFrameC)]),
    "tm_siti_reset": (_i, [_vp]),
    "tm_siti_si": (C.c_double, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_double]),
    "tm_siti_ti": (C.c_double, [C.c_int64, C.c_uint64, C.c_uint64, _u32, C.c_double]),
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


class SitiError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed: code {code}")
        self.code = code


def _chk(rc, what):
    if rc != ffi.TM_OK:
        raise SitiError(rc, what)


class SitiFrame(NamedTuple):
    s1: int        # sum q over the (w - 2)(h - 2) interior positions, q the Sobel magnitude rounded to an integer on the 16-bit scale
    s2: int        # sum q^2
    t1: int        # sum d over the w h positions, d = this picture - the previous one; 0 for the first picture of a sequence
    t2: int        # sum d^2
    ti_valid: int  # 0 for the first picture of a sequence
    si: float      # the library's si / ti of the sums at gain 1
    ti: float


class Siti:
    """P.910 SI / TI of one sequence, `batch` pictures per compute.  layout: "y8" | "y16_msb" | "y16_low" | "y10_packed"
    (include/turbo_metrics_siti.h).  A picture is its luma plane: a numpy array (copied) or a torch tensor (device tensors are read
    in place, pinned host tensors by DMA: both must stay alive until compute returns).
    compute(n) is compute_async(n) then sync(): the two halves let several objects, each on its own stream, be in flight at once."""

    def __init__(self, w, h, layout="y8", bits=8, batch=1):
        self._L = lib()
        self.w, self.h, self.bits, self.batch = int(w), int(h), int(bits), int(batch)
        self.layout = layout
        h_ = C.c_void_p()
        _chk(self._L.tm_siti_create(C.byref(h_), self.w, self.h, LAYOUTS[layout], self.bits, self.batch), "tm_siti_create")
        self._h = h_
        self._keep = {}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tm_siti_destroy(self._h)
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
        return int(self._L.tm_siti_mem_usage(self._h))

    def plane_shape(self):
        """(rows, elements per row) of the luma plane of this layout, and the element size in bytes"""
        if self.layout == "y10_packed":
            return (self.h, synth.p10_row_words(self.w)), 4
        return (self.h, self.w), 1 if self.layout == "y8" else 2

    def set_frame(self, slot, y):
        """Checks the plane against the layout before the library sees a pointer: the element size (unsigned integers; signed 16- and
        32-bit ones as views of unsigned data), a 2-D shape of at least the picture's rows x row width, a column stride of 1.
        ValueError otherwise."""
        (rows, cols), esz = self.plane_shape()
        if hasattr(y, "data_ptr"):
            size, signed = y.element_size(), y.dtype.is_signed
            ok = not (y.dtype.is_floating_point or y.dtype.is_complex or str(y.dtype) == "torch.bool")
            shape, stride = tuple(y.shape), tuple(y.stride())
        else:
            if not isinstance(y, np.ndarray):
                raise ValueError(f"a numpy array or a torch tensor is needed, got {type(y).__name__}")
            size, signed, ok = y.itemsize, y.dtype.kind == "i", y.dtype.kind in "ui"
            shape, stride = y.shape, tuple(s // y.itemsize for s in y.strides)
        if not ok or size != esz or (signed and size not in (2, 4)):
            raise ValueError(f"{self.layout} at {self.bits} bits takes {8 * esz}-bit unsigned elements, got {y.dtype}")
        if len(shape) != 2 or shape[0] < rows or shape[1] < cols:
            raise ValueError(f"at least {rows} x {cols} elements are needed, got shape {shape}")
        if stride[1] != 1 or stride[0] < cols:
            raise ValueError(f"rows of contiguous elements are needed, got strides {stride}")
        if not 0 <= int(slot) < self.batch:
            raise ValueError(f"slot {slot} of a batch of {self.batch}")
        ptr, mem, keep = _ptr_and_mem(y)
        pitch = int(keep.stride(0) * keep.element_size()) if hasattr(keep, "data_ptr") else int(keep.strides[0])
        self._keep[int(slot)] = keep
        _chk(self._L.tm_siti_set_frame(self._h, int(slot), ptr, pitch, mem), "tm_siti_set_frame")

    def compute(self, n):
        """slots [0, n) continue the sequence; waits for the result"""
        _chk(self._L.tm_siti_compute_async(self._h, int(n)), "tm_siti_compute_async")
        _chk(self._L.tm_siti_sync(self._h), "tm_siti_sync")

    def compute_async(self, n):
        """tm_siti_compute_async: queues slots [0, n) on this object's stream and returns; the planes stay alive until sync()"""
        _chk(self._L.tm_siti_compute_async(self._h, int(n)), "tm_siti_compute_async")

    def sync(self):
        """tm_siti_sync: waits for what compute_async queued"""
        _chk(self._L.tm_siti_sync(self._h), "tm_siti_sync")

    def frames(self, n, first=0):
        out = (SitiFrameC * n)()
        _chk(self._L.tm_siti_get(self._h, int(first), int(n), out), "tm_siti_get")
        return [SitiFrame(int(f.s1), int(f.s2), int(f.t1), int(f.t2), int(f.ti_valid), float(f.si), float(f.ti)) for f in out]

    def reset(self):
        _chk(self._L.tm_siti_reset(self._h), "tm_siti_reset")


def si(s1, s2, n_si, gain=1.0):
    """tm_siti_si: gain sqrt(n_si s2 - s1^2) / n_si / 256"""
    return float(lib().tm_siti_si(int(s1), int(s2), int(n_si), float(gain)))


def ti(t1, t2, n, bits, gain=1.0):
    """tm_siti_ti: gain sqrt(n t2 - t1^2) / n / 2^(bits - 8)"""
    return float(lib().tm_siti_ti(int(t1), int(t2), int(n), int(bits), float(gain)))


LIMITED_RANGE_GAIN = 255.0 / 219.0  # the linear limited-to-full-range stretch, without clipping
