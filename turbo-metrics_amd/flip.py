"""ctypes binding of include/turbo_metrics_flip.h (libturbometrics_flip.so, built in-tree): LDR-FLIP, the perceptual difference map of
pairs of sRGB pictures, on the MI355X.  A prototype table of its own (ffi.SYMBOLS is the engine's); loaded on
first use.  Raises if the library is missing: there is no CPU path.

    f = Flip(1920, 1080, "rgb8", batch=8)
    f.set_pair(0, ref, dis); ...; f.compute(n); f.frames(n)  -> [FlipFrame(mean, min, max)];  f.map(0), f.map(0, "color")
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import ffi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libturbometrics_flip.so")

LAYOUTS = {"rgb8": 0}
KINDS = {"flip": 0, "color": 1, "feature": 2}
DEFAULT_PPD = 67.02064327658226
MAX_RADIUS = 10


class FlipFrameC(C.Structure):
    _fields_ = [("mean", C.c_double), ("min", C.c_double), ("max", C.c_double)]


_vp, _u32, _i, _sz, _d = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t, C.c_double
SYMBOLS = {
    "tm_flip_create": (_i, [C.POINTER(_vp), _u32, _u32, _i, _d, _u32]),
    "tm_flip_destroy": (None, [_vp]),
    "tm_flip_mem_usage": (_sz, [_vp]),
    "tm_flip_set_pair": (_i, [_vp, _u32, _vp, _sz, _vp, _sz, _i]),
    "tm_flip_compute_async": (_i, [_vp, _u32]),
    "tm_flip_sync": (_i, [_vp]),
    "tm_flip_get": (_i, [_vp, _u32, _u32, C.POINTER(FlipFrameC)]),
    "tm_flip_get_map": (_i, [_vp, _u32, _i, _vp, _sz]),
    "tm_flip_radius": (_i, [_d, C.POINTER(_u32), C.POINTER(_u32)]),
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


class FlipError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed: code {code}")
        self.code = code


def _chk(rc, what):
    if rc != ffi.TM_OK:
        raise FlipError(rc, what)


class FlipFrame(NamedTuple):
    mean: float  # the FLIP score of the pair
    min: float
    max: float


def radius(ppd=None):
    """(spatial, feature) filter radii at `ppd` pixels per degree (tm_flip_radius): (10, 9) at the default"""
    a, b = _u32(), _u32()
    _chk(lib().tm_flip_radius(float(ppd or 0.0), C.byref(a), C.byref(b)), "tm_flip_radius")
    return int(a.value), int(b.value)


def _surface(x, w, h):
    """(pointer, pitch in bytes, memory kind, what keeps it alive) of a packed RGB8 picture [h][w][3] or [h][3 w]: a numpy array or a
    torch tensor (device tensors are read in place).  ValueError for anything else"""
    if hasattr(x, "data_ptr"):
        if str(x.dtype) != "torch.uint8":
            raise ValueError(f"rgb8 takes 8-bit unsigned elements, got {x.dtype}")
        shape, stride = tuple(x.shape), tuple(x.stride())
        ptr, keep = int(x.data_ptr()), x
        mem = ffi.TM_MEM_DEVICE if getattr(x, "is_cuda", False) else ffi.TM_MEM_HOST
    else:
        if not isinstance(x, np.ndarray):
            raise ValueError(f"a numpy array or a torch tensor is needed, got {type(x).__name__}")
        if x.dtype != np.uint8:
            raise ValueError(f"rgb8 takes 8-bit unsigned elements, got {x.dtype}")
        shape, stride = x.shape, x.strides
        ptr, keep, mem = x.ctypes.data, x, ffi.TM_MEM_HOST
    if len(shape) == 3:
        if shape[0] < h or shape[1] < w or shape[2] != 3 or stride[2] != 1 or stride[1] != 3:
            raise ValueError(f"at least {h} x {w} x 3 packed bytes are needed, got shape {shape} strides {stride}")
    elif len(shape) == 2:
        if shape[0] < h or shape[1] < 3 * w or stride[1] != 1:
            raise ValueError(f"at least {h} x {3 * w} bytes are needed, got shape {shape} strides {stride}")
    else:
        raise ValueError(f"a picture is [h][w][3] or [h][3 w], got shape {shape}")
    pitch = int(stride[0])
    if pitch < 3 * w:
        if shape[0] > 1:
            raise ValueError(f"rows of at least {3 * w} bytes are needed, got a row stride of {pitch}")
        pitch = 3 * w
    return ptr, pitch, mem, keep


class Flip:
    """LDR-FLIP of `batch` pairs per compute.  layout: "rgb8" (packed sRGB bytes, any row pitch); ppd: pixels per degree, None for the
    default 67.02 (FlipError(TM_ERR_UNSUPPORTED) above 74.04, where the spatial radius passes MAX_RADIUS).  Stateless: nothing is kept
    between computes.  compute(n) is compute_async(n) then sync()."""

    def __init__(self, w, h, layout="rgb8", ppd=None, batch=8):
        self._h = None
        self._L = lib()
        self.w, self.h, self.batch = int(w), int(h), int(batch)
        self.ppd = float(ppd) if ppd else DEFAULT_PPD
        h_ = C.c_void_p()
        _chk(self._L.tm_flip_create(C.byref(h_), self.w, self.h, LAYOUTS[layout], self.ppd, self.batch), "tm_flip_create")
        self._h = h_
        self._keep = {}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tm_flip_destroy(self._h)
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
        return int(self._L.tm_flip_mem_usage(self._h))

    def set_pair(self, slot, ref, dis):
        if not 0 <= int(slot) < self.batch:
            raise ValueError(f"slot {slot} of a batch of {self.batch}")
        rp, rpitch, rmem, rkeep = _surface(ref, self.w, self.h)
        dp, dpitch, dmem, dkeep = _surface(dis, self.w, self.h)
        if rmem != dmem:
            raise ValueError("both pictures of a pair are in host memory or both in device memory")
        self._keep[int(slot)] = (rkeep, dkeep)
        _chk(self._L.tm_flip_set_pair(self._h, int(slot), rp, rpitch, dp, dpitch, rmem), "tm_flip_set_pair")

    def compute(self, n):
        """FLIP of slots [0, n); waits for the result"""
        self.compute_async(n)
        self.sync()

    def compute_async(self, n):
        _chk(self._L.tm_flip_compute_async(self._h, int(n)), "tm_flip_compute_async")

    def sync(self):
        _chk(self._L.tm_flip_sync(self._h), "tm_flip_sync")

    def frames(self, n, first=0):
        out = (FlipFrameC * n)()
        _chk(self._L.tm_flip_get(self._h, int(first), int(n), out), "tm_flip_get")
        return [FlipFrame(float(f.mean), float(f.min), float(f.max)) for f in out]

    def map(self, slot, kind="flip"):
        """one map of a computed slot, float32 [h][w]: "flip", "color" (dEc) or "feature" (dEf)"""
        if kind not in KINDS:
            raise ValueError(f"kind {kind!r}: one of {sorted(KINDS)}")
        out = np.empty((self.h, self.w), np.float32)
        _chk(self._L.tm_flip_get_map(self._h, int(slot), KINDS[kind], out.ctypes.data_as(_vp), out.strides[0]), "tm_flip_get_map")
        return out
