"""ctypes binding of include/turbo_metrics_mdsi.h (libturbometrics_mdsi.so, built in-tree): MDSI, the mean deviation similarity index
of 4:2:0 pictures on the MI355X.  A prototype table of its own (ffi.SYMBOLS is the engine's); loaded on first
use.  Raises if the library is missing: there is no CPU path.

    t = Mdsi(1920, 1080, "nv12", 8, matrix="bt709", factor=0, batch=8, maps=False)
    t.set_pair(0, (y, uv), (y2, uv2)); ...; t.compute(n); t.frames(n)  -> [MdsiFrame(.mdsi, .mad, .negatives, ...)]
    t.map(slot)  -> the ceil(h / f) x ceil(w / f) float32 GCS values (maps=True)
    mdsi.score(dev, n), mdsi.factor(w, h), mdsi.lhm(y, u, v, matrix, bits): the host functions of the definition
MDSI does not pool across pictures: a sequence's value is the mean of its pairs' values.
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import ffi, synth
from .engine import _ptr_and_mem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libturbometrics_mdsi.so")

LAYOUTS = {"nv12": 0, "p016": 1, "i420": 2, "i420p10": 3}
MATRICES = {"bt709": 0, "bt601": 1, "by_height": 2}
TM_MDSI_MAPS = 1


class MdsiFrameC(C.Structure):
    _fields_ = [("sum_re", C.c_double), ("sum_im", C.c_double), ("dev", C.c_double), ("n", C.c_uint64), ("negatives", C.c_uint64),
                ("factor", C.c_uint32), ("pad_", C.c_uint32)]


_vp, _u32, _i, _sz, _d = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t, C.c_double
SYMBOLS = {
    "tm_mdsi_create": (_i, [C.POINTER(_vp), _u32, _u32, _i, _u32, _i, _u32, _u32, _u32]),
    "tm_mdsi_destroy": (None, [_vp]),
    "tm_mdsi_mem_usage": (_sz, [_vp]),
    "tm_mdsi_get_factor": (_u32, [_vp]),
    "tm_mdsi_set_frame": (_i, [_vp, _u32, _i, _vp, _vp, _vp, _sz, _sz, _i]),
    "tm_mdsi_compute_async": (_i, [_vp, _u32]),
    "tm_mdsi_sync": (_i, [_vp]),
    "tm_mdsi_get": (_i, [_vp, _u32, _u32, C.POINTER(MdsiFrameC)]),
    "tm_mdsi_map": (_i, [_vp, _u32, _vp, _sz]),
    "tm_mdsi_score": (_d, [_d, C.c_uint64]),
    "tm_mdsi_factor": (_u32, [_u32, _u32]),
    "tm_mdsi_lhm": (_i, [_u32, _u32, _u32, _i, _u32, C.POINTER(_d)]),
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


class MdsiError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed: code {code}")
        self.code = code


def _chk(rc, what):
    if rc != ffi.TM_OK:
        raise MdsiError(rc, what)


class MdsiFrame(NamedTuple):
    mdsi: float       # (dev / n)^(1/4): 0 for identical pictures, larger is worse
    mad: float        # dev / n
    negatives: int    # positions with GCS < 0 (the complex branch of the fourth root)
    sum_re: float     # the f64 sums of Re z and Im z over the n positions
    sum_im: float
    dev: float        # the f64 sum of |z - mu|
    n: int
    factor: int


class Mdsi:
    """MDSI of `batch` pairs per compute.  layout: "nv12" | "p016" | "i420" | "i420p10" (include/turbo_metrics_mdsi.h); matrix:
    "bt709" | "bt601" | "by_height"; factor: 1 .. 128, or 0 for max(1, round(min(w, h) / 256)).  A picture is the tuple of its planes:
    (Y, CbCr) for nv12 / p016, (Y, Cb, Cr) otherwise; numpy arrays (copied) or torch tensors (device tensors are read in place, pinned
    host tensors by DMA: both must stay alive until compute returns).  compute(n) is compute_async(n) then sync()."""

    def __init__(self, w, h, layout="nv12", bits=8, matrix="bt709", factor=0, batch=1, maps=False):
        self._L = lib()
        self.w, self.h, self.bits, self.batch = int(w), int(h), int(bits), int(batch)
        self.layout, self.matrix, self.maps = layout, matrix, bool(maps)
        if layout not in LAYOUTS:
            raise ValueError(f"layout is one of {', '.join(map(repr, LAYOUTS))}, got {layout!r}")
        if matrix not in MATRICES:
            raise ValueError(f"matrix is 'bt709', 'bt601' or 'by_height', got {matrix!r}")
        h_ = C.c_void_p()
        _chk(self._L.tm_mdsi_create(C.byref(h_), self.w, self.h, LAYOUTS[layout], self.bits, MATRICES[matrix], int(factor),
                                    TM_MDSI_MAPS if self.maps else 0, self.batch), "tm_mdsi_create")
        self._h = h_
        self._keep = {}
        self.factor = int(self._L.tm_mdsi_get_factor(self._h))  # the library's own: forced, or from the picture size
        self.wd, self.hd = -(-self.w // self.factor), -(-self.h // self.factor)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tm_mdsi_destroy(self._h)
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
        return int(self._L.tm_mdsi_mem_usage(self._h))

    def _plane_shapes(self):
        """(rows, elements per row) of each plane of this layout, and the element size in bytes"""
        cw, ch = (self.w + 1) // 2, (self.h + 1) // 2
        if self.layout in ("nv12", "p016"):
            return [(self.h, self.w), (ch, 2 * cw)], 1 if self.layout == "nv12" else 2
        if self.layout == "i420":
            return [(self.h, self.w), (ch, cw), (ch, cw)], 1 if self.bits == 8 else 2
        return [(self.h, synth.p10_row_words(self.w)), (ch, synth.p10_row_words(cw)), (ch, synth.p10_row_words(cw))], 4

    def set_frame(self, slot, side, planes):
        """Checks every plane against the layout before the library sees a pointer (the checks of tm.Yuv): the plane count, the
        element size (unsigned integers; signed 16- and 32-bit ones as views of unsigned data), 2-D shapes of at least the picture's
        rows x row width, a column stride of 1, and one row pitch for Cb and Cr (host numpy planes are copied to one instead).
        ValueError otherwise."""
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
            # one pitch for Cb and Cr (tm_mdsi_set_frame takes pitch_uv once): host copies of the rows the picture uses
            planes[1:] = [np.ascontiguousarray(p[:rows, :cols]) for p, (rows, cols) in zip(planes[1:], shapes[1:])]
        planes = [_ptr_and_mem(p) for p in planes]
        mems = {m for _, m, _ in planes}
        if len(mems) != 1:
            raise ValueError("the planes must live in the same kind of memory")
        pitch = lambda k: int(k.stride(0) * k.element_size()) if hasattr(k, "data_ptr") else int(k.strides[0])
        if len(planes) == 3 and pitch(planes[1][2]) != pitch(planes[2][2]):
            raise ValueError("Cb and Cr must have the same row pitch (tm_mdsi_set_frame takes pitch_uv once)")
        self._keep[(slot, side)] = [k for _, _, k in planes]
        y, u = planes[0], planes[1]
        v = planes[2] if len(planes) > 2 else (None, None, None)
        _chk(self._L.tm_mdsi_set_frame(self._h, slot, side, y[0], u[0], v[0], pitch(y[2]), pitch(u[2]), mems.pop()), "tm_mdsi_set_frame")

    def set_pair(self, slot, ref, dis):
        self.set_frame(slot, ffi.TM_SIDE_REF, ref)
        self.set_frame(slot, ffi.TM_SIDE_DIS, dis)

    def compute(self, n):
        """slots [0, n); waits for the result"""
        _chk(self._L.tm_mdsi_compute_async(self._h, int(n)), "tm_mdsi_compute_async")
        _chk(self._L.tm_mdsi_sync(self._h), "tm_mdsi_sync")

    def compute_async(self, n):
        """tm_mdsi_compute_async: queues slots [0, n) on this object's stream and returns; the planes stay alive until sync()"""
        _chk(self._L.tm_mdsi_compute_async(self._h, int(n)), "tm_mdsi_compute_async")

    def sync(self):
        """tm_mdsi_sync: waits for what compute_async queued"""
        _chk(self._L.tm_mdsi_sync(self._h), "tm_mdsi_sync")

    def frames(self, n, first=0):
        out = (MdsiFrameC * n)()
        _chk(self._L.tm_mdsi_get(self._h, int(first), int(n), out), "tm_mdsi_get")
        return [MdsiFrame(score(f.dev, f.n), float(f.dev) / int(f.n), int(f.negatives), float(f.sum_re), float(f.sum_im), float(f.dev), int(f.n),
                          int(f.factor)) for f in out]

    def map(self, slot):
        """the GCS of every decimated position of a slot of the last compute: float32 [hd, wd] (maps=True; MdsiError TM_ERR_STATE
        otherwise)"""
        out = np.empty((self.hd, self.wd), np.float32)
        _chk(self._L.tm_mdsi_map(self._h, int(slot), out.ctypes.data_as(C.c_void_p), self.wd * 4), "tm_mdsi_map")
        return out


def score(dev, n):
    """tm_mdsi_score: (dev / n)^(1/4), in double"""
    return float(lib().tm_mdsi_score(float(dev), int(n)))


def factor_of(w, h):
    """tm_mdsi_factor: max(1, round(min(w, h) / 256)), halves away from zero"""
    return int(lib().tm_mdsi_factor(int(w), int(h)))


factor = factor_of


def lhm(y, u, v, matrix="bt709", bits=8):
    """tm_mdsi_lhm: one limited-range Y'CbCr triple of depth `bits` -> (L, H, M) on the 0 .. 255 scale, in double"""
    out = (C.c_double * 3)()
    _chk(lib().tm_mdsi_lhm(int(y), int(u), int(v), MATRICES[matrix], int(bits), out), "tm_mdsi_lhm")
    return tuple(float(t) for t in out)
