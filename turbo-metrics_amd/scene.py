"""ctypes binding of include/turbo_metrics_scene.h (libturbometrics_scene.so, built in-tree): the 256-bin luma histogram of every
picture on the MI355X, and the host functions that turn consecutive histograms into scene cuts.  A prototype table of its own
(ffi.SYMBOLS is the engine's); loaded on first use.  Raises if the library is missing: there is no CPU path.

    s = Scene(1920, 1080, "y8", 8, batch=8)
    s.set_frame(0, y); ...; s.compute(n); s.frames(n)  -> [SceneFrame(hist)];  cuts([f.hist for f in all_frames], 1920, 1080)
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import ffi, synth
from .engine import _ptr_and_mem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libturbometrics_scene.so")

LAYOUTS = {"y8": 0, "y16_msb": 1, "y16_low": 2, "y10_packed": 3}
DEFAULT_BINS = 64
DEFAULT_THRESHOLD = 0.5


class SceneFrameC(C.Structure):
    _fields_ = [("hist", C.c_uint32 * 256)]


_vp, _u32, _i, _sz, _u64 = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t, C.c_uint64
_hist = C.POINTER(C.c_uint32)
SYMBOLS = {
    "tm_scene_create": (_i, [C.POINTER(_vp), _u32, _u32, _i, _u32, _u32]),
    "tm_scene_destroy": (None, [_vp]),
    "tm_scene_mem_usage": (_sz, [_vp]),
    "tm_scene_set_frame": (_i, [_vp, _u32, _vp, _sz, _i]),
    "tm_scene_compute_async": (_i, [_vp, _u32]),
    "tm_scene_sync": (_i, [_vp]),
    "tm_scene_get": (_i, [_vp, _u32, _u32, C.POINTER(SceneFrameC)]),
    "tm_scene_distance": (_i, [_hist, _hist, _i, C.POINTER(_u64)]),
    "tm_scene_score": (C.c_double, [_u64, _u32, _u32]),
    "tm_scene_is_cut": (_i, [C.c_double, C.c_double]),
    "tm_scene_stats": (_i, [_hist, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.c_double)]),
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


class SceneError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed: code {code}")
        self.code = code


def _chk(rc, what):
    if rc != ffi.TM_OK:
        raise SceneError(rc, what)


class SceneFrame(NamedTuple):
    hist: np.ndarray  # uint32[256]: hist[b] = samples with sample >> (D - 8) == b


class Scene:
    """The luma histograms of `batch` pictures per compute.  layout: "y8" | "y16_msb" | "y16_low" | "y10_packed"
    (include/turbo_metrics_scene.h).  A picture is its luma plane: a numpy array (copied) or a torch tensor (device tensors are read
    in place, pinned host tensors by DMA: both must stay alive until compute returns).  Stateless: nothing is kept between computes.
    compute(n) is compute_async(n) then sync(): the two halves let several objects, each on its own stream, be in flight at once."""

    def __init__(self, w, h, layout="y8", bits=8, batch=1):
        self._L = lib()
        self.w, self.h, self.bits, self.batch = int(w), int(h), int(bits), int(batch)
        self.layout = layout
        h_ = C.c_void_p()
        _chk(self._L.tm_scene_create(C.byref(h_), self.w, self.h, LAYOUTS[layout], self.bits, self.batch), "tm_scene_create")
        self._h = h_
        self._keep = {}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tm_scene_destroy(self._h)
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
        return int(self._L.tm_scene_mem_usage(self._h))

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
        if stride[1] != 1 or (stride[0] < cols and shape[0] > 1):
            raise ValueError(f"rows of contiguous elements are needed, got strides {stride}")
        if not 0 <= int(slot) < self.batch:
            raise ValueError(f"slot {slot} of a batch of {self.batch}")
        ptr, mem, keep = _ptr_and_mem(y)
        pitch = int(keep.stride(0) * keep.element_size()) if hasattr(keep, "data_ptr") else int(keep.strides[0])
        self._keep[int(slot)] = keep
        _chk(self._L.tm_scene_set_frame(self._h, int(slot), ptr, max(pitch, cols * esz), mem), "tm_scene_set_frame")

    def compute(self, n):
        """the histograms of slots [0, n); waits for the result"""
        _chk(self._L.tm_scene_compute_async(self._h, int(n)), "tm_scene_compute_async")
        _chk(self._L.tm_scene_sync(self._h), "tm_scene_sync")

    def compute_async(self, n):
        """tm_scene_compute_async: queues slots [0, n) on this object's stream and returns; the planes stay alive until sync()"""
        _chk(self._L.tm_scene_compute_async(self._h, int(n)), "tm_scene_compute_async")

    def sync(self):
        """tm_scene_sync: waits for what compute_async queued"""
        _chk(self._L.tm_scene_sync(self._h), "tm_scene_sync")

    def frames(self, n, first=0):
        out = (SceneFrameC * n)()
        _chk(self._L.tm_scene_get(self._h, int(first), int(n), out), "tm_scene_get")
        return [SceneFrame(np.ctypeslib.as_array(f.hist).astype(np.uint32)) for f in out]


def _h(hist):
    a = np.ascontiguousarray(hist, dtype=np.uint32)
    if a.shape != (256,):
        raise ValueError(f"a histogram of 256 bins is needed, got shape {a.shape}")
    return a, a.ctypes.data_as(_hist)


def distance(a, b, bins=DEFAULT_BINS):
    """sum over the merged bins of |A_k - B_k| (tm_scene_distance); ValueError for a `bins` that is not 8, 16, 32, 64, 128 or 256"""
    (ka, pa), (kb, pb) = _h(a), _h(b)
    out = _u64()
    if lib().tm_scene_distance(pa, pb, int(bins), C.byref(out)) != ffi.TM_OK:
        raise ValueError(f"bins is one of 8, 16, 32, 64, 128, 256, got {bins}")
    return int(out.value)


def score(dist, w, h):
    return float(lib().tm_scene_score(int(dist), int(w), int(h)))


def is_cut(s, threshold=DEFAULT_THRESHOLD):
    return bool(lib().tm_scene_is_cut(float(s), float(threshold)))


def stats(hist):
    """(lowest bin in use, highest bin in use, mean bin) of one histogram (tm_scene_stats)"""
    k, p = _h(hist)
    lo, hi, mean = _u32(), _u32(), C.c_double()
    if lib().tm_scene_stats(p, C.byref(lo), C.byref(hi), C.byref(mean)) != ffi.TM_OK:
        raise ValueError("the histogram is empty")
    return int(lo.value), int(hi.value), float(mean.value)


def cuts(hists, w, h, bins=DEFAULT_BINS, threshold=DEFAULT_THRESHOLD):
    """one sequence's histograms, in order -> (scores, cut_flags): a picture's score is that of the distance to the picture before
    it; the first picture has score 0 and is never a cut"""
    scores, flags = [], []
    for i, cur in enumerate(hists):
        s = 0.0 if i == 0 else score(distance(hists[i - 1], cur, bins), w, h)
        scores.append(s)
        flags.append(i > 0 and is_cut(s, threshold))
    return scores, flags
