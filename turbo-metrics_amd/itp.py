"""ctypes binding of include/turbo_metrics_itp.h (libturbometrics_itp.so, built in-tree): the BT.2124 colour difference dE ITP of
4:2:0 HDR pictures on the MI355X.  A prototype table of its own (ffi.SYMBOLS is the engine's); loaded on first
use.  Raises if the library is missing: there is no CPU path.

    t = Itp(3840, 2160, "p016", 10, transfer="pq", batch=8, maps=False)
    t.set_pair(0, (y, uv), (y2, uv2)); ...; t.compute(n); t.frames(n)  -> [ItpFrame(de_sum, de_mean, de_max, pixels)]
    t.map(slot)  -> the h x w float32 dE ITP values (maps=True)
    itp.ictcp(y, u, v, bits, transfer), itp.de(ictcp1, ictcp2), itp.pq_eotf(signal), itp.pq_inv_eotf(light),
    itp.hlg_display(rgb): the host functions of the definition
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import ffi, synth
from .engine import _ptr_and_mem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libturbometrics_itp.so")

LAYOUTS = {"nv12": 0, "p016": 1, "i420": 2, "i420p10": 3}
TRANSFERS = {"pq": 0, "hlg": 1}


class ItpFrameC(C.Structure):
    _fields_ = [("de_sum", C.c_double), ("de_mean", C.c_double), ("de_max", C.c_double), ("pixels", C.c_uint64)]


_vp, _u32, _i, _sz, _d = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t, C.c_double
SYMBOLS = {
    "tm_itp_create": (_i, [C.POINTER(_vp), _u32, _u32, _i, _u32, _i, _i, _i, _u32]),
    "tm_itp_destroy": (None, [_vp]),
    "tm_itp_mem_usage": (_sz, [_vp]),
    "tm_itp_set_frame": (_i, [_vp, _u32, _i, _vp, _vp, _vp, _sz, _sz, _i]),
    "tm_itp_compute_async": (_i, [_vp, _u32]),
    "tm_itp_sync": (_i, [_vp]),
    "tm_itp_get": (_i, [_vp, _u32, _u32, C.POINTER(ItpFrameC)]),
    "tm_itp_get_map": (_i, [_vp, _u32, _vp, _sz]),
    "tm_itp_ictcp": (_i, [_u32, _u32, _u32, _u32, _i, C.POINTER(_d)]),
    "tm_itp_de": (_d, [C.POINTER(_d), C.POINTER(_d)]),
    "tm_itp_pq_eotf": (_d, [_d]),
    "tm_itp_pq_inv_eotf": (_d, [_d]),
    "tm_itp_hlg_display": (_i, [C.POINTER(_d), C.POINTER(_d)]),
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


class ItpError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed: code {code}")
        self.code = code


def _chk(rc, what):
    if rc != ffi.TM_OK:
        raise ItpError(rc, what)


class ItpFrame(NamedTuple):
    de_sum: float   # the f64 sum of dE ITP over all luma positions
    de_mean: float  # de_sum / pixels
    de_max: float
    pixels: int


class Itp:
    """dE ITP of `batch` pairs per compute.  layout: "nv12" | "p016" | "i420" | "i420p10" (include/turbo_metrics_itp.h); transfer:
    "pq" | "hlg" (on a 1000 cd/m2 display); the matrix is BT.2020 non-constant luminance.  A picture is the tuple of its planes:
    (Y, CbCr) for nv12 / p016, (Y, Cb, Cr) otherwise; numpy arrays (copied) or torch tensors (device tensors are read in place, pinned
    host tensors by DMA: both must stay alive until compute returns).  compute(n) is compute_async(n) then sync()."""

    def __init__(self, w, h, layout="p016", bits=10, transfer="pq", batch=1, maps=False):
        self._L = lib()
        self.w, self.h, self.bits, self.batch = int(w), int(h), int(bits), int(batch)
        self.layout, self.transfer, self.maps = layout, transfer, bool(maps)
        if transfer not in TRANSFERS:
            raise ValueError(f"transfer is 'pq' or 'hlg', got {transfer!r}")
        h_ = C.c_void_p()
        _chk(self._L.tm_itp_create(C.byref(h_), self.w, self.h, LAYOUTS[layout], self.bits, TRANSFERS[transfer], 0, int(self.maps), self.batch),
             "tm_itp_create")
        self._h = h_
        self._keep = {}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tm_itp_destroy(self._h)
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
        return int(self._L.tm_itp_mem_usage(self._h))

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
            # one pitch for Cb and Cr (tm_itp_set_frame takes pitch_uv once): host copies of the rows the picture uses
            planes[1:] = [np.ascontiguousarray(p[:rows, :cols]) for p, (rows, cols) in zip(planes[1:], shapes[1:])]
        planes = [_ptr_and_mem(p) for p in planes]
        mems = {m for _, m, _ in planes}
        if len(mems) != 1:
            raise ValueError("the planes must live in the same kind of memory")
        pitch = lambda k: int(k.stride(0) * k.element_size()) if hasattr(k, "data_ptr") else int(k.strides[0])
        if len(planes) == 3 and pitch(planes[1][2]) != pitch(planes[2][2]):
            raise ValueError("Cb and Cr must have the same row pitch (tm_itp_set_frame takes pitch_uv once)")
        self._keep[(slot, side)] = [k for _, _, k in planes]
        y, u = planes[0], planes[1]
        v = planes[2] if len(planes) > 2 else (None, None, None)
        _chk(self._L.tm_itp_set_frame(self._h, slot, side, y[0], u[0], v[0], pitch(y[2]), pitch(u[2]), mems.pop()), "tm_itp_set_frame")

    def set_pair(self, slot, ref, dis):
        self.set_frame(slot, ffi.TM_SIDE_REF, ref)
        self.set_frame(slot, ffi.TM_SIDE_DIS, dis)

    def compute(self, n):
        """slots [0, n); waits for the result"""
        _chk(self._L.tm_itp_compute_async(self._h, int(n)), "tm_itp_compute_async")
        _chk(self._L.tm_itp_sync(self._h), "tm_itp_sync")

    def compute_async(self, n):
        """tm_itp_compute_async: queues slots [0, n) on this object's stream and returns; the planes stay alive until sync()"""
        _chk(self._L.tm_itp_compute_async(self._h, int(n)), "tm_itp_compute_async")

    def sync(self):
        """tm_itp_sync: waits for what compute_async queued"""
        _chk(self._L.tm_itp_sync(self._h), "tm_itp_sync")

    def frames(self, n, first=0):
        out = (ItpFrameC * n)()
        _chk(self._L.tm_itp_get(self._h, int(first), int(n), out), "tm_itp_get")
        return [ItpFrame(float(f.de_sum), float(f.de_mean), float(f.de_max), int(f.pixels)) for f in out]

    def map(self, slot):
        """the dE ITP of every luma position of a slot of the last compute: float32 [h, w] (maps=True; ItpError TM_ERR_STATE otherwise)"""
        out = np.empty((self.h, self.w), np.float32)
        _chk(self._L.tm_itp_get_map(self._h, int(slot), out.ctypes.data_as(C.c_void_p), self.w * 4), "tm_itp_get_map")
        return out


def ictcp(y, u, v, bits=10, transfer="pq"):
    """tm_itp_ictcp: one limited-range BT.2020 Y'CbCr triple of depth `bits` -> (I, Ct, Cp), in double"""
    out = (C.c_double * 3)()
    _chk(lib().tm_itp_ictcp(int(y), int(u), int(v), int(bits), TRANSFERS[transfer], out), "tm_itp_ictcp")
    return tuple(float(t) for t in out)


def de(ictcp1, ictcp2):
    """tm_itp_de: 720 sqrt(dI^2 + (dCt / 2)^2 + dCp^2) of two (I, Ct, Cp) triples, in double"""
    a, b = (C.c_double * 3)(*[float(v) for v in ictcp1]), (C.c_double * 3)(*[float(v) for v in ictcp2])
    return float(lib().tm_itp_de(a, b))


def pq_eotf(signal):
    """tm_itp_pq_eotf: PQ signal in [0, 1] -> cd/m2"""
    return float(lib().tm_itp_pq_eotf(float(signal)))


def pq_inv_eotf(light):
    """tm_itp_pq_inv_eotf: cd/m2 in [0, 10000] -> PQ signal"""
    return float(lib().tm_itp_pq_inv_eotf(float(light)))


def hlg_display(rgb):
    """tm_itp_hlg_display: HLG R'G'B' signals -> (R, G, B) in cd/m2 on the 1000 cd/m2 display"""
    a, out = (C.c_double * 3)(*[float(v) for v in rgb]), (C.c_double * 3)()
    _chk(lib().tm_itp_hlg_display(a, out), "tm_itp_hlg_display")
    return tuple(float(t) for t in out)
