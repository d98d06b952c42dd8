"""ctypes binding of include/turbo_metrics_hvs.h (libturbometrics_hvs.so, built in-tree): PSNR-HVS and PSNR-HVS-M over the luma planes
of reference / distorted pairs on the MI355X.  A prototype table of its own (ffi.SYMBOLS is the engine's);
loaded on first use.  Raises if the library is missing: there is no CPU path.

    v = Hvs(1920, 1080, "y8", 8, batch=8)
    v.set_pair(0, y_ref, y_dis); ...; v.compute(n); v.frames(n)  -> [HvsFrame(s_hvs, s_hvsm, blocks, psnr_hvs, psnr_hvs_m)]
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import ffi, synth
from .engine import _ptr_and_mem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libturbometrics_hvs.so")

LAYOUTS = {"y8": 0, "y16_msb": 1, "y16_low": 2, "y10_packed": 3}


class HvsFrameC(C.Structure):
    _fields_ = [("s_hvs", C.c_double), ("s_hvsm", C.c_double), ("blocks", C.c_uint64)]


_vp, _u32, _i, _sz = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t
SYMBOLS = {
    "tm_hvs_create": (_i, [C.POINTER(_vp), _u32, _u32, _i, _u32, _u32]),
    "tm_hvs_destroy": (None, [_vp]),
    "tm_hvs_mem_usage": (_sz, [_vp]),
    "tm_hvs_set_pair": (_i, [_vp, _u32, _vp, _vp, _sz, _sz, _i]),
    "tm_hvs_compute_async": (_i, [_vp, _u32]),
    "tm_hvs_sync": (_i, [_vp]),
    "tm_hvs_get": (_i, [_vp, _u32, _u32, C.POINTER(HvsFrameC)]),
    "tm_hvs_psnr": (C.c_double, [C.c_double, C.c_uint64, _u32]),
    "tm_hvs_csf": (C.POINTER(C.c_float), []),
    "tm_hvs_mask": (C.POINTER(C.c_float), []),
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


class HvsError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed: code {code}")
        self.code = code


def _chk(rc, what):
    if rc != ffi.TM_OK:
        raise HvsError(rc, what)


class HvsFrame(NamedTuple):
    s_hvs: float       # S2: the sum of the squared CSF-weighted coefficients of the difference
    s_hvsm: float      # S1: the same after contrast masking
    blocks: int        # 8x8 blocks of the picture
    psnr_hvs: float    # tm_hvs_psnr(s_hvs, blocks, bits)
    psnr_hvs_m: float  # tm_hvs_psnr(s_hvsm, blocks, bits)


def psnr(s, blocks, bits):
    """tm_hvs_psnr: 10 log10(peak^2 * 64 * blocks / s); inf for s = 0.  Of a sequence: the summed s and the summed blocks."""
    return float(lib().tm_hvs_psnr(float(s), int(blocks), int(bits)))


def tables():
    """(CSF, MASK): the library's two 8x8 tables as float32 arrays, [vertical frequency][horizontal frequency]"""
    L = lib()
    return (np.ctypeslib.as_array(L.tm_hvs_csf(), (64,)).reshape(8, 8).copy(), np.ctypeslib.as_array(L.tm_hvs_mask(), (64,)).reshape(8, 8).copy())


class Hvs:
    """PSNR-HVS / PSNR-HVS-M of `batch` reference / distorted pairs per compute.  layout: "y8" | "y16_msb" | "y16_low" | "y10_packed"
    (include/turbo_metrics_hvs.h).  A picture is its luma plane: a numpy array (copied) or a torch tensor (device tensors are read in
    place, pinned host tensors by DMA: both must stay alive until compute returns).  The two planes of a pair live in the same kind
    of memory.
    compute(n) is compute_async(n) then sync(): the two halves let several objects, each on its own stream, be in flight at once."""

    def __init__(self, w, h, layout="y8", bits=8, batch=1):
        self._L = lib()
        self.w, self.h, self.bits, self.batch = int(w), int(h), int(bits), int(batch)
        self.layout = layout
        h_ = C.c_void_p()
        _chk(self._L.tm_hvs_create(C.byref(h_), self.w, self.h, LAYOUTS[layout], self.bits, self.batch), "tm_hvs_create")
        self._h = h_
        self._keep = {}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tm_hvs_destroy(self._h)
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
        return int(self._L.tm_hvs_mem_usage(self._h))

    def plane_shape(self):
        """(rows, elements per row) of the luma plane of this layout, and the element size in bytes"""
        if self.layout == "y10_packed":
            return (self.h, synth.p10_row_words(self.w)), 4
        return (self.h, self.w), 1 if self.layout == "y8" else 2

    def _check(self, y):
        """Checks a plane against the layout before the library sees a pointer: the element size (unsigned integers; signed 16- and
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

    def set_pair(self, slot, y_ref, y_dis):
        self._check(y_ref)
        self._check(y_dis)
        if not 0 <= int(slot) < self.batch:
            raise ValueError(f"slot {slot} of a batch of {self.batch}")
        (pr, mr, kr), (pd, md, kd) = _ptr_and_mem(y_ref), _ptr_and_mem(y_dis)
        if mr != md:
            raise ValueError("the two planes of a pair must live in the same kind of memory")
        pitch = lambda k: int(k.stride(0) * k.element_size()) if hasattr(k, "data_ptr") else int(k.strides[0])
        self._keep[int(slot)] = (kr, kd)
        _chk(self._L.tm_hvs_set_pair(self._h, int(slot), pr, pd, pitch(kr), pitch(kd), mr), "tm_hvs_set_pair")

    def compute(self, n):
        """slots [0, n); waits for the result"""
        _chk(self._L.tm_hvs_compute_async(self._h, int(n)), "tm_hvs_compute_async")
        _chk(self._L.tm_hvs_sync(self._h), "tm_hvs_sync")

    def compute_async(self, n):
        """tm_hvs_compute_async: queues slots [0, n) on this object's stream and returns; the planes stay alive until sync()"""
        _chk(self._L.tm_hvs_compute_async(self._h, int(n)), "tm_hvs_compute_async")

    def sync(self):
        """tm_hvs_sync: waits for what compute_async queued"""
        _chk(self._L.tm_hvs_sync(self._h), "tm_hvs_sync")

    def frames(self, n, first=0):
        out = (HvsFrameC * n)()
        _chk(self._L.tm_hvs_get(self._h, int(first), int(n), out), "tm_hvs_get")
        return [HvsFrame(float(f.s_hvs), float(f.s_hvsm), int(f.blocks), psnr(f.s_hvs, f.blocks, self.bits), psnr(f.s_hvsm, f.blocks, self.bits))
                for f in out]
