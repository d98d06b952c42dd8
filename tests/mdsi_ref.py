"""TEST INFRASTRUCTURE ONLY: MDSI as DESIGN.md section 23 states it, in float64 numpy and in the PAPER's form -- R'G'B' per pixel from
Y'CbCr with replicated chroma, L, H, M per pixel, its own zero-padded conv2 'same' with ones(f) / f^2, decimation, Prewitt / 3, the
gradient of the actual fused plane, the similarity quotients as the paper writes them, numpy's complex ** 0.25 and mad -- written from
that text and not from the kernel, which maps exact integer box sums and evaluates 1 - e forms.  `mistake` seeds one deliberate error
(tests/test_mdsi_cpu.py shows that each moves a number)."""
import math
from typing import NamedTuple

import numpy as np

C1, C2, C3, ALPHA = 140.0, 55.0, 550.0, 0.6
MATRICES = {"bt709": (1.5748, 0.187324, 0.468124, 1.8556), "bt601": (1.402, 0.344136, 0.714136, 1.772)}
PREWITT = np.array([[1, 0, -1], [1, 0, -1], [1, 0, -1]], np.float64) / 3
MISTAKES = ("window0", "replicate", "half_even", "div_n_in", "chroma_once", "gs_swapped", "mu_real", "fused_mean_mag", "offsets_ff",
            "byte_behind")


def factor(w, h, mistake=None):
    """max(1, round(min(w, h) / 256)), MATLAB's round: halves away from zero"""
    q = min(w, h) / 256
    r = round(q) if mistake == "half_even" else math.floor(q + 0.5)  # Python's round() is half-even
    return max(1, int(r))


def matrix_of(matrix, h):
    return ("bt709" if h >= 720 else "bt601") if matrix == "by_height" else matrix


def conv2_same(a, k, pad="zero", value=0.0):
    """MATLAB's conv2(a, k, 'same'): the true convolution (kernel flipped) of the padded plane, the central part the size of `a`, which
    for an even kernel side n starts at element n / 2 of the full result.  pad: "zero", "edge" (a seeded mistake) or "value" (`value` outside)"""
    H, W = a.shape
    kh, kw = k.shape
    if pad == "edge":
        p = np.pad(a, ((kh, kh), (kw, kw)), mode="edge")
    else:
        p = np.pad(a, ((kh, kh), (kw, kw)), mode="constant", constant_values=value if pad == "value" else 0.0)
    out = np.zeros((H, W))
    for i in range(kh):
        for j in range(kw):  # out[y, x] += k[i, j] * a[y + kh // 2 - i, x + kw // 2 - j]
            y0, x0 = kh + kh // 2 - i, kw + kw // 2 - j
            out += k[i, j] * p[y0:y0 + H, x0:x0 + W]
    return out


def lhm(Y, U, V, bits, matrix):
    """sample values (arrays of one shape) -> L, H, M on the 0 .. 255 scale, R'G'B' not clipped"""
    s = float(1 << (bits - 8))
    c = MATRICES[matrix]
    yn, un, vn = (Y - 16 * s) / (219 * s), (U - 128 * s) / (224 * s), (V - 128 * s) / (224 * s)
    R, G, B = 255 * (yn + c[0] * vn), 255 * (yn - c[1] * un - c[2] * vn), 255 * (yn + c[3] * un)
    return 0.2989 * R + 0.5870 * G + 0.1140 * B, 0.30 * R + 0.04 * G - 0.35 * B, 0.34 * R - 0.60 * G + 0.17 * B


def _planes_direct(Y, U, V, bits, matrix, f):
    """the "chroma_once" mistake, window by window: where a window starts on an odd luma index every chroma sample it touches enters
    once on that axis, whatever number of the window's positions take it"""
    H, W = Y.shape
    hd, wd = -(-H // f), -(-W // f)
    lead = (f + 1) // 2 - 1
    k = [lhm(*(np.float64(v) for v in t), bits, matrix) for t in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))]
    out = np.zeros((3, hd, wd))

    def axis(i, lim):
        a, b = max(i * f - lead, 0), min(i * f - lead + f - 1, lim - 1)
        cs = list(range(a >> 1, (b >> 1) + 1))
        wt = [1 if a & 1 else min(b, 2 * c + 1) - max(a, 2 * c) + 1 for c in cs]
        return a, b, cs, np.array(wt, np.float64)
    for j in range(hd):
        ra, rb, cys, wy = axis(j, H)
        for i in range(wd):
            ca, cb, cxs, wx = axis(i, W)
            sy = Y[ra:rb + 1, ca:cb + 1].sum()
            wgt = np.outer(wy, wx)
            su, sv = (U[np.ix_(cys, cxs)] * wgt).sum(), (V[np.ix_(cys, cxs)] * wgt).sum()
            n = (rb - ra + 1) * (cb - ca + 1)
            for q in range(3):
                out[q, j, i] = ((k[0][q] - k[3][q]) * sy + (k[1][q] - k[3][q]) * su + (k[2][q] - k[3][q]) * sv + k[3][q] * n) / (f * f)
    return out


def planes(yuv, bits, matrix, f, mistake=None):
    """(Y, Cb, Cr) integer sample planes -> the decimated L, H, M, [3, hd, wd]"""
    Y, U, V = (np.asarray(p, np.float64) for p in yuv)
    H, W = Y.shape
    if mistake == "chroma_once":
        return _planes_direct(Y, U, V, bits, matrix, f)
    up = lambda c: np.repeat(np.repeat(c, 2, 0), 2, 1)[:H, :W]
    Uu, Vu = up(U), up(V)
    if mistake == "byte_behind" and W % 2:  # the sample behind an odd row's last one: the next row's first in a tight plane
        nxt = lambda p: np.hstack([p, np.vstack([p[1:, :1], np.zeros((1, 1))])])
        Y, Uu, Vu = nxt(Y), np.hstack([Uu, Uu[:, -1:]]), np.hstack([Vu, Vu[:, -1:]])
    P = np.stack(lhm(Y, Uu, Vu, bits, matrix))
    box = np.ones((f, f))
    out = []
    for q in range(3):
        if mistake == "window0":  # rows i f .. i f + f - 1: no centring
            p = np.pad(P[q], ((0, f), (0, f)))
            ave = sum(p[a:a + P[q].shape[0], b:b + P[q].shape[1]] for a in range(f) for b in range(f)) / (f * f)
        elif mistake == "replicate":
            ave = conv2_same(P[q], box, "edge") / (f * f)
        elif mistake == "div_n_in":
            ave = conv2_same(P[q], box) / conv2_same(np.ones_like(P[q]), box)
        elif mistake == "offsets_ff":  # the constant offsets f^2 times: zero SAMPLES outside, not zero planes
            zero = lhm(np.float64(0), np.float64(0), np.float64(0), bits, matrix)[q]
            ave = conv2_same(P[q], box, "value", zero) / (f * f)
        else:
            ave = conv2_same(P[q], box) / (f * f)
        out.append(ave[:H, :W][0::f, 0::f])
    return np.stack(out)


def gradients(L, mistake=None):
    pad = "edge" if mistake == "replicate" else "zero"
    return conv2_same(L, PREWITT, pad), conv2_same(L, PREWITT.T, pad)


class Ref(NamedTuple):
    mdsi: float
    mad: float
    n: int
    negatives: int
    factor: int
    gcs: np.ndarray   # the map, [hd, wd]
    sum_z: complex


def mdsi(ref, dis, bits, matrix="bt709", factor_=0, mistake=None):
    """ref, dis: (Y, Cb, Cr) integer sample planes of depth `bits` -> Ref"""
    assert mistake is None or mistake in MISTAKES
    H, W = np.asarray(ref[0]).shape
    f = factor_ or factor(W, H, mistake)
    m = matrix_of(matrix, H)
    Pr, Pd = planes(ref, bits, m, f, mistake), planes(dis, bits, m, f, mistake)
    Lr, Ld = Pr[0], Pd[0]
    F = (Lr + Ld) / 2
    gr, gd = np.hypot(*gradients(Lr, mistake)), np.hypot(*gradients(Ld, mistake))
    gf = (gr + gd) / 2 if mistake == "fused_mean_mag" else np.hypot(*gradients(F, mistake))
    GS12 = (2 * gr * gd + C1) / (gr ** 2 + gd ** 2 + C1)
    GS13 = (2 * gr * gf + C2) / (gr ** 2 + gf ** 2 + C2)
    GS23 = (2 * gd * gf + C2) / (gd ** 2 + gf ** 2 + C2)
    GS = GS12 + GS13 - GS23 if mistake == "gs_swapped" else GS12 + GS23 - GS13
    CS = (2 * (Pr[1] * Pd[1] + Pr[2] * Pd[2]) + C3) / (Pr[1] ** 2 + Pd[1] ** 2 + Pr[2] ** 2 + Pd[2] ** 2 + C3)
    GCS = ALPHA * GS + (1 - ALPHA) * CS
    z = GCS.astype(np.complex128) ** 0.25
    mu = z.mean()
    if mistake == "mu_real":
        mu = mu.real
    mad = float(np.abs(z - mu).mean())
    return Ref(mad ** 0.25, mad, GCS.size, int((GCS < 0).sum()), f, GCS, complex(z.sum()))


def score(dev, n):
    """the host function tm_mdsi_score, restated"""
    return math.nan if n == 0 else (dev / n) ** 0.25
