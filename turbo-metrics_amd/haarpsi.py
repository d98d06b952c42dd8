"""ctypes binding of include/turbo_metrics_haarpsi.h (libturbometrics_haarpsi.so, built in-tree): HaarPSI, the Haar wavelet-based
perceptual similarity index (grayscale form), over the luma planes of reference / distorted pairs on the MI355X.
A prototype table of its own (ffi.SYMBOLS is the engine's); loaded on first use.  Raises if the library is missing: there is no CPU path.

    p = HaarPsi(1920, 1080, "y8", 8, batch=8, maps=False)
    p.set_pair(0, y_ref, y_dis); ...; p.compute(n); p.frames(n)  -> [HaarPsiFrame(haarpsi, q, ws)];  p.map(slot) with maps=True
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import ffi, synth
from .engine import _ptr_and_mem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libturbometrics_haarpsi.so")

LAYOUTS = {"y8": 0, "y16_msb": 1, "y16_low": 2, "y10_packed": 3}
TM_HAARPSI_MAPS = 1


class HaarPsiFrameC(C.Structure):
    _fields_ = [("q", C.c_double), ("ws", C.c_uint64)]


_vp, _u32, _i, _sz = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t
SYMBOLS = {
    "tm_haarpsi_create": (_i, [C.POINTER(_vp), _u32, _u32, _i, _u32, _u32, _u32]),
    "tm_haarpsi_destroy": (None, [_vp]),
    "tm_haarpsi_mem_usage": (_sz, [_vp]),
    "tm_haarpsi_set_pair": (_i, [_vp, _u32, _vp, _vp, _sz, _sz, _i]),
    "tm_haarpsi_compute_async": (_i, [_vp, _u32]),
    "tm_haarpsi_sync": (_i, [_vp]),
    "tm_haarpsi_get": (_i, [_vp, _u32, _u32, C.POINTER(HaarPsiFrameC)]),
    "tm_haarpsi_map": (_i, [_vp, _u32, _vp, _sz]),
    "tm_haarpsi_score": (C.c_double, [C.c_double, C.c_uint64]),
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


class HaarPsiError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed: code {code}")
        self.code = code


def _chk(rc, what):
    if rc != ffi.TM_OK:
        raise HaarPsiError(rc, what)


class HaarPsiFrame(NamedTuple):
    haarpsi: float  # tm_haarpsi_score(q, ws): 1 = identical; NaN where both pictures are flat
    q: float        # the sum of q_o W_o over the decimated positions and both orientations
    ws: int         # the sum of W_o, exact


def score(q, ws):
    """tm_haarpsi_score: x = q / ws, (log((1 - x) / x) / 4.2f)^2.  NaN for ws = 0.  Of a sequence: the summed q and ws of its pairs."""
    return float(lib().tm_haarpsi_score(float(q), int(ws)))


class HaarPsi:
    """HaarPSI of `batch` reference / distorted pairs per compute; maps=True keeps every slot's local similarity map for map().  layout:
    "y8" | "y16_msb" | "y16_low" | "y10_packed" (include/turbo_metrics_haarpsi.h).  A picture is its luma plane: a numpy array (copied) or
    a torch tensor (device tensors are read in place, pinned host tensors by DMA: both must stay alive until compute returns).  The two
    planes of a pair live in the same kind of memory.
    compute(n) is compute_async(n) then sync(): the two halves let several objects, each on its own stream, be in flight at once."""

    def __init__(self, w, h, layout="y8", bits=8, batch=1, maps=False):
        self._L = lib()
        self.w, self.h, self.bits, self.batch = int(w), int(h), int(bits), int(batch)
        self.layout, self.maps = layout, bool(maps)
        h_ = C.c_void_p()
        _chk(self._L.tm_haarpsi_create(C.byref(h_), self.w, self.h, LAYOUTS[layout], self.bits, self.batch, TM_HAARPSI_MAPS if maps else 0), "tm_haarpsi_create")
        self._h = h_
        self._keep = {}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tm_haarpsi_destroy(self._h)
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
        return int(self._L.tm_haarpsi_mem_usage(self._h))

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
        _chk(self._L.tm_haarpsi_set_pair(self._h, int(slot), pr, pd, pitch(kr), pitch(kd), mr), "tm_haarpsi_set_pair")

    def compute(self, n):
        """slots [0, n); waits for the result"""
        _chk(self._L.tm_haarpsi_compute_async(self._h, int(n)), "tm_haarpsi_compute_async")
        _chk(self._L.tm_haarpsi_sync(self._h), "tm_haarpsi_sync")

    def compute_async(self, n):
        """tm_haarpsi_compute_async: queues slots [0, n) on this object's stream and returns; the planes stay alive until sync()"""
        _chk(self._L.tm_haarpsi_compute_async(self._h, int(n)), "tm_haarpsi_compute_async")

    def sync(self):
        """tm_haarpsi_sync: waits for what compute_async queued"""
        _chk(self._L.tm_haarpsi_sync(self._h), "tm_haarpsi_sync")

    def frames(self, n, first=0):
        out = (HaarPsiFrameC * n)()
        _chk(self._L.tm_haarpsi_get(self._h, int(first), int(n), out), "tm_haarpsi_get")
        return [HaarPsiFrame(score(f.q, f.ws), float(f.q), int(f.ws)) for f in out]

    def map(self, slot, out=None):
        """tm_haarpsi_map: the local similarity map (s_v + s_h) / 2 of slot `slot` of the last compute, ceil(h / 2) x ceil(w / 2) float32
        (into `out`, a float32 array of at least that shape with contiguous rows, if given).  HaarPsiError(TM_ERR_STATE) without
        maps=True."""
        h2, w2 = (self.h + 1) // 2, (self.w + 1) // 2
        if out is None:
            out = np.empty((h2, w2), np.float32)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.ndim == 2 and out.shape[0] >= h2 and out.shape[1] >= w2 and
                  out.strides[1] == 4 and out.strides[0] >= 4 * w2):
            raise ValueError(f"a float32 array of at least {h2} x {w2} with contiguous rows is needed")
        _chk(self._L.tm_haarpsi_map(self._h, int(slot), out.ctypes.data, out.strides[0] if h2 > 1 else 4 * w2), "tm_haarpsi_map")
        return out[:h2, :w2]
