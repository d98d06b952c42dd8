"""TEST INFRASTRUCTURE ONLY: the definition of plane-wise YUV PSNR and SSIM restated in numpy, written from
the text: int64 block and window sums, one float32 expression per window, float64 (math.fsum: exactly rounded) plane sums.  The
`mistake=` argument seeds one of the mistakes the tests must catch."""
import math
from typing import NamedTuple

import numpy as np

LAYOUT_BITS = {"nv12": (8,), "p016": tuple(range(9, 17)), "i420": tuple(range(8, 17)), "i420p10": (10,)}
MAX_DIM = 32768
MISTAKES = ("stride8", "c2_no63", "covar_single", "no_remainder_columns", "chroma_floor")


def supported(w, h, layout, bits):
    return 16 <= w <= MAX_DIM and 16 <= h <= MAX_DIM and layout in LAYOUT_BITS and bits in LAYOUT_BITS[layout]


def constants(bits, mistake=None):
    mx = float((1 << bits) - 1)
    c1 = int(.01 * .01 * mx * mx * 64 + .5)
    c2 = int(.03 * .03 * mx * mx * 64 * (1 if mistake == "c2_no63" else 63) + .5)
    return c1, c2


def chroma_size(w, h, mistake=None):
    return (w // 2, h // 2) if mistake == "chroma_floor" else ((w + 1) // 2, (h + 1) // 2)


def sse(a, b, mistake=None):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if mistake == "no_remainder_columns":
        a, b = a[:, :a.shape[1] // 4 * 4], b[:, :b.shape[1] // 4 * 4]
    d = a - b
    return int((d * d).sum())


def block_sums(a, b):
    """s1, s2, ss, s12 of every 4x4 block: int64 [bh, bw]"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    bh, bw = a.shape[0] >> 2, a.shape[1] >> 2
    blk = lambda p: p[:4 * bh, :4 * bw].reshape(bh, 4, bw, 4).sum((1, 3))
    return blk(a), blk(b), blk(a * a + b * b), blk(a * b)


def ssim_map(a, b, bits, mistake=None):
    """the window values: float32 [bh - 1, bw - 1]"""
    c1, c2 = constants(bits, mistake)
    win = lambda s: s[:-1, :-1] + s[:-1, 1:] + s[1:, :-1] + s[1:, 1:]
    s1, s2, ss, s12 = (win(s) for s in block_sums(a, b))
    if mistake == "stride8":
        s1, s2, ss, s12 = (s[::2, ::2] for s in (s1, s2, ss, s12))
    vars_ = ss * 64 - s1 * s1 - s2 * s2
    covar = s12 * 64 - s1 * s2
    f = lambda x: x.astype(np.float32)
    n = f(2 * s1 * s2 + c1) * f((1 if mistake == "covar_single" else 2) * covar + c2)
    d = f(s1 * s1 + s2 * s2 + c1) * f(vars_ + c2)
    v = n / d
    assert v.dtype == np.float32
    return v


class Plane(NamedTuple):
    sse: int
    map: np.ndarray   # float32 [bh - 1, bw - 1]
    ssim_sum: float   # the exactly rounded sum of the map
    abs_sum: float    # sum |v|: the scale of the summation bound
    ssim: float


def plane(a, b, bits, mistake=None):
    m = ssim_map(a, b, bits, mistake)
    vals = [float(v) for v in m.ravel()]
    s = math.fsum(vals)
    return Plane(sse(a, b, mistake), m, s, math.fsum(abs(v) for v in vals), s / m.size)


def frame(ref, dis, bits, mistake=None):
    """ref, dis: (Y, Cb, Cr) sample arrays -> [Plane] * 3"""
    return [plane(a, b, bits, mistake) for a, b in zip(ref, dis)]


def psnr(sse_, n, bits, cap=0.0):
    if not 8 <= bits <= 16:
        return math.nan
    if sse_ == 0:
        return cap if cap > 0 else math.inf
    mx = float((1 << bits) - 1)
    v = 10.0 * math.log10(((mx * mx) * float(n)) / float(sse_))
    return min(v, cap) if cap > 0 else v


def psnr_avg(sses, ns, bits, cap=0.0):
    return psnr(sum(sses), sum(ns), bits, cap)


def ssim_all(ssims, ns):
    return (ns[0] * ssims[0] + ns[1] * ssims[1] + ns[2] * ssims[2]) / (ns[0] + ns[1] + ns[2])


def ssim_db(s):
    return math.inf if s >= 1.0 else -10.0 * math.log10(1.0 - s)


def sum_bound(p):
    """what a float64 sum of the map's n values in any order may differ from the exactly rounded sum by: each of the n - 1 additions
    rounds a partial sum of magnitude at most sum |v| by at most 2^-53 of it, and the reference's own rounding is one more"""
    return p.map.size * 2.0 ** -53 * p.abs_sum
