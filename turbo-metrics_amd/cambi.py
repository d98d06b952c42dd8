"""ctypes binding of include/turbo_metrics_cambi.h (libturbometrics_cambi.so, built in-tree): CAMBI, VMAF's banding index, of every
picture of one stream on the MI355X.  A prototype table of its own (ffi.SYMBOLS is the engine's); loaded on
first use.  Raises if the library is missing: there is no CPU path.

    c = Cambi(1920, 1080, "y8", 8, batch=8)
    c.set_frame(0, y); ...; c.compute(n); c.frames(n)  -> [CambiFrame(cambi, scales, t, n_gt, k, sum_gt)];  c.heatmap(0, 2)
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import ffi, synth
from .engine import _ptr_and_mem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libturbometrics_cambi.so")

LAYOUTS = {"y8": 0, "y16_msb": 1, "y16_low": 2, "y10_packed": 3}
SCALES = 5
DEFAULT_TOPK = 0.6
DEFAULT_TVI_THRESHOLD = 0.019


class CambiFrameC(C.Structure):
    _fields_ = [("t", C.c_uint32 * SCALES), ("n_gt", C.c_uint32 * SCALES), ("k", C.c_uint32 * SCALES), ("reserved", C.c_uint32),
                ("sum_gt", C.c_double * SCALES)]


_vp, _u32, _i, _sz, _d = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t, C.c_double
SYMBOLS = {
    "tm_cambi_create": (_i, [C.POINTER(_vp), _u32, _u32, _i, _u32, _u32, _d, _d, _u32]),
    "tm_cambi_destroy": (None, [_vp]),
    "tm_cambi_mem_usage": (_sz, [_vp]),
    "tm_cambi_set_frame": (_i, [_vp, _u32, _vp, _sz, _i]),
    "tm_cambi_compute_async": (_i, [_vp, _u32]),
    "tm_cambi_sync": (_i, [_vp]),
    "tm_cambi_get": (_i, [_vp, _u32, _u32, C.POINTER(CambiFrameC)]),
    "tm_cambi_get_map": (_i, [_vp, _u32, _u32, _vp, _sz]),
    "tm_cambi_scores": (_i, [C.POINTER(CambiFrameC), _u32, C.POINTER(_d)]),
    "tm_cambi_tvi": (_i, [_d, C.POINTER(_u32)]),
    "tm_cambi_mask_index": (_u32, [_u32, _u32]),
    "tm_cambi_window": (_u32, [_u32, _u32]),
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


class CambiError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed: code {code}")
        self.code = code


def _chk(rc, what):
    if rc != ffi.TM_OK:
        raise CambiError(rc, what)


class CambiFrame(NamedTuple):
    cambi: float        # min(sum_s weight_s scales[s] / area, 1000)
    scales: tuple       # the five scale scores
    t: tuple            # per scale: the k-th largest c-value, f32 bits
    n_gt: tuple         # per scale: c-values strictly above t
    k: tuple
    sum_gt: tuple       # per scale: their f64 sum


def tvi(tvi_threshold=DEFAULT_TVI_THRESHOLD):
    """the four visibility thresholds (tm_cambi_tvi): (178, 305, 432, 559) for 0.019"""
    out = (_u32 * 4)()
    _chk(lib().tm_cambi_tvi(float(tvi_threshold), out), "tm_cambi_tvi")
    return tuple(int(x) for x in out)


def mask_index(w, h):
    return int(lib().tm_cambi_mask_index(int(w), int(h)))


def window(w, requested=0):
    return int(lib().tm_cambi_window(int(w), int(requested)))


def scores(t, n_gt, k, sum_gt, win):
    """(five scale scores, cambi) of one picture's raw fields (tm_cambi_scores)"""
    f = CambiFrameC()
    for s in range(SCALES):
        f.t[s], f.n_gt[s], f.k[s], f.sum_gt[s] = int(t[s]), int(n_gt[s]), int(k[s]), float(sum_gt[s])
    out = (_d * 6)()
    if lib().tm_cambi_scores(C.byref(f), int(win), out) != ffi.TM_OK:
        raise ValueError("k is at least 1 and above n_gt at every scale, and the window is 3 .. 127")
    return tuple(float(x) for x in out[:5]), float(out[5])


class Cambi:
    """CAMBI of `batch` pictures per compute.  layout: "y8" | "y16_msb" | "y16_low" | "y10_packed" (include/turbo_metrics_cambi.h);
    window: 0 derives it from the width.  A picture is its luma plane: a numpy array (copied) or a torch tensor (device tensors are
    read in place, pinned host tensors by DMA: both must stay alive until compute returns).  Stateless: nothing is kept between
    computes.
    compute(n) is compute_async(n) then sync(): the two halves let several objects, each on its own stream, be in flight at once."""

    def __init__(self, w, h, layout="y8", bits=8, window=0, topk=DEFAULT_TOPK, tvi_threshold=DEFAULT_TVI_THRESHOLD, batch=1):
        self._L = lib()
        self.w, self.h, self.bits, self.batch = int(w), int(h), int(bits), int(batch)
        self.layout = layout
        h_ = C.c_void_p()
        _chk(self._L.tm_cambi_create(C.byref(h_), self.w, self.h, LAYOUTS[layout], self.bits, int(window), float(topk), float(tvi_threshold),
                                     self.batch), "tm_cambi_create")
        self._h = h_
        self._keep = {}
        self.window = int(self._L.tm_cambi_window(self.w, int(window)))
        self.scale_shapes = []
        sw, sh = self.w, self.h
        for s in range(SCALES):
            self.scale_shapes.append((sh, sw))
            sw, sh = (sw + 1) >> 1, (sh + 1) >> 1

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tm_cambi_destroy(self._h)
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
        return int(self._L.tm_cambi_mem_usage(self._h))

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
        _chk(self._L.tm_cambi_set_frame(self._h, int(slot), ptr, max(pitch, cols * esz), mem), "tm_cambi_set_frame")

    def compute(self, n):
        """CAMBI of slots [0, n); waits for the result"""
        _chk(self._L.tm_cambi_compute_async(self._h, int(n)), "tm_cambi_compute_async")
        _chk(self._L.tm_cambi_sync(self._h), "tm_cambi_sync")

    def compute_async(self, n):
        """tm_cambi_compute_async: queues slots [0, n) on this object's stream and returns; the planes stay alive until sync()"""
        _chk(self._L.tm_cambi_compute_async(self._h, int(n)), "tm_cambi_compute_async")

    def sync(self):
        """tm_cambi_sync: waits for what compute_async queued"""
        _chk(self._L.tm_cambi_sync(self._h), "tm_cambi_sync")

    def frames(self, n, first=0):
        out = (CambiFrameC * n)()
        _chk(self._L.tm_cambi_get(self._h, int(first), int(n), out), "tm_cambi_get")
        res = []
        for f in out:
            sc = (_d * 6)()
            _chk(self._L.tm_cambi_scores(C.byref(f), self.window, sc), "tm_cambi_scores")
            res.append(CambiFrame(float(sc[5]), tuple(float(x) for x in sc[:5]), tuple(f.t), tuple(f.n_gt), tuple(f.k), tuple(f.sum_gt)))
        return res

    def heatmap(self, slot, scale):
        """the c-values of one scale of a computed slot: float32 [h_scale][w_scale]"""
        if not 0 <= int(scale) < SCALES:
            raise ValueError(f"scale {scale} of {SCALES}")
        out = np.empty(self.scale_shapes[int(scale)], np.float32)
        _chk(self._L.tm_cambi_get_map(self._h, int(slot), int(scale), out.ctypes.data_as(_vp), out.strides[0]), "tm_cambi_get_map")
        return out
