"""ctypes binding of include/turbo_metrics_gmsd.h (libturbometrics_gmsd.so, built in-tree): GMSD, the gradient magnitude similarity
deviation, over the luma planes of reference / distorted pairs on the MI355X.  A prototype table of its own
(ffi.SYMBOLS is the engine's); loaded on first use.  Raises if the library is missing: there is no CPU path.

    g = Gmsd(1920, 1080, "y8", 8, batch=8, maps=False)
    g.set_pair(0, y_ref, y_dis); ...; g.compute(n); g.frames(n)  -> [GmsdFrame(e1, e2, e_max, n, gmsd, gmsm)];  g.map(slot) with maps=True
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import ffi, synth
from .engine import _ptr_and_mem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libturbometrics_gmsd.so")

LAYOUTS = {"y8": 0, "y16_msb": 1, "y16_low": 2, "y10_packed": 3}
TM_GMSD_MAPS = 1


class GmsdFrameC(C.Structure):
    _fields_ = [("e1", C.c_double), ("e2", C.c_double), ("e_max", C.c_float), ("n", C.c_uint64)]


_vp, _u32, _i, _sz = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t
SYMBOLS = {
    "tm_gmsd_create": (_i, [C.POINTER(_vp), _u32, _u32, _i, _u32, _u32, _u32]),
    "tm_gmsd_destroy": (None, [_vp]),
    "tm_gmsd_mem_usage": (_sz, [_vp]),
    "tm_gmsd_set_pair": (_i, [_vp, _u32, _vp, _vp, _sz, _sz, _i]),
    "tm_gmsd_compute_async": (_i, [_vp, _u32]),
    "tm_gmsd_sync": (_i, [_vp]),
    "tm_gmsd_get": (_i, [_vp, _u32, _u32, C.POINTER(GmsdFrameC)]),
    "tm_gmsd_map": (_i, [_vp, _u32, _vp, _sz]),
    "tm_gmsd_score": (C.c_double, [C.c_double, C.c_double, C.c_uint64, _i]),
    "tm_gmsd_mean": (C.c_double, [C.c_double, C.c_uint64]),
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


class GmsdError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed: code {code}")
        self.code = code


def _chk(rc, what):
    if rc != ffi.TM_OK:
        raise GmsdError(rc, what)


class GmsdFrame(NamedTuple):
    e1: float      # the sum of e = 1 - GMS over the decimated positions
    e2: float      # the sum of e^2
    e_max: float   # the largest e
    n: int         # decimated positions: ceil(w / 2) ceil(h / 2)
    gmsd: float    # tm_gmsd_score(e1, e2, n, population)
    gmsm: float    # tm_gmsd_mean(e1, n): the mean GMS


def score(e1, e2, n, population=False):
    """tm_gmsd_score: sqrt(max(0, (e2 - e1^2 / n) / (n - 1))), the sample standard deviation of GMS; population: / n.  NaN for n < 2.  Of a
    sequence: the summed e1, e2 and n of its pairs."""
    return float(lib().tm_gmsd_score(float(e1), float(e2), int(n), int(bool(population))))


def mean(e1, n):
    """tm_gmsd_mean: 1 - e1 / n, the mean GMS.  NaN for n < 2."""
    return float(lib().tm_gmsd_mean(float(e1), int(n)))


class Gmsd:
    """GMSD of `batch` reference / distorted pairs per compute; maps=True keeps every slot's GMS map for map().  layout: "y8" | "y16_msb" | "y16_low" | "y10_packed"
    (include/turbo_metrics_gmsd.h).  A picture is its luma plane: a numpy array (copied) or a torch tensor (device tensors are read in
    place, pinned host tensors by DMA: both must stay alive until compute returns).  The two planes of a pair live in the same kind
    of memory.
    compute(n) is compute_async(n) then sync(): the two halves let several objects, each on its own stream, be in flight at once."""

    def __init__(self, w, h, layout="y8", bits=8, batch=1, maps=False, population=False):
        self._L = lib()
        self.w, self.h, self.bits, self.batch = int(w), int(h), int(bits), int(batch)
        self.layout, self.maps, self.population = layout, bool(maps), bool(population)
        h_ = C.c_void_p()
        _chk(self._L.tm_gmsd_create(C.byref(h_), self.w, self.h, LAYOUTS[layout], self.bits, self.batch, TM_GMSD_MAPS if maps else 0), "tm_gmsd_create")
        self._h = h_
        self._keep = {}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tm_gmsd_destroy(self._h)
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
        return int(self._L.tm_gmsd_mem_usage(self._h))

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
        _chk(self._L.tm_gmsd_set_pair(self._h, int(slot), pr, pd, pitch(kr), pitch(kd), mr), "tm_gmsd_set_pair")

    def compute(self, n):
        """slots [0, n); waits for the result"""
        _chk(self._L.tm_gmsd_compute_async(self._h, int(n)), "tm_gmsd_compute_async")
        _chk(self._L.tm_gmsd_sync(self._h), "tm_gmsd_sync")

    def compute_async(self, n):
        """tm_gmsd_compute_async: queues slots [0, n) on this object's stream and returns; the planes stay alive until sync()"""
        _chk(self._L.tm_gmsd_compute_async(self._h, int(n)), "tm_gmsd_compute_async")

    def sync(self):
        """tm_gmsd_sync: waits for what compute_async queued"""
        _chk(self._L.tm_gmsd_sync(self._h), "tm_gmsd_sync")

    def frames(self, n, first=0):
        out = (GmsdFrameC * n)()
        _chk(self._L.tm_gmsd_get(self._h, int(first), int(n), out), "tm_gmsd_get")
        return [GmsdFrame(float(f.e1), float(f.e2), float(f.e_max), int(f.n), score(f.e1, f.e2, f.n, self.population), mean(f.e1, f.n)) for f in out]

    def map(self, slot, out=None):
        """tm_gmsd_map: the GMS map of slot `slot` of the last compute, ceil(h / 2) x ceil(w / 2) float32 (into `out`, a float32 array of at
        least that shape with contiguous rows, if given).  GmsdError(TM_ERR_STATE) without maps=True."""
        h2, w2 = (self.h + 1) // 2, (self.w + 1) // 2
        if out is None:
            out = np.empty((h2, w2), np.float32)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.ndim == 2 and out.shape[0] >= h2 and out.shape[1] >= w2 and
                  out.strides[1] == 4 and out.strides[0] >= 4 * w2):
            raise ValueError(f"a float32 array of at least {h2} x {w2} with contiguous rows is needed")
        _chk(self._L.tm_gmsd_map(self._h, int(slot), out.ctypes.data, out.strides[0] if h2 > 1 else 4 * w2), "tm_gmsd_map")
        return out[:h2, :w2]
