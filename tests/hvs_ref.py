"""TEST INFRASTRUCTURE ONLY: PSNR-HVS and PSNR-HVS-M as DESIGN.md section 16 states them, in float64 numpy, written from that text and
not from the kernel.  `mistake` seeds one deliberate error (tests/test_hvs_cpu.py shows that each moves a number)."""
import math
from typing import NamedTuple

import numpy as np

Q = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
              [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
              [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], np.float64)
CSF = np.round(25.73509 / Q, 6)
MASK = np.round((10.0 / Q) ** 2, 6)
MISTAKES = ("transposed_tables", "masked_dc", "biased_variance", "halves", "min_mask", "remainder")


def dct_matrix():
    """C[k][n] = a_k cos((2 n + 1) k pi / 16), a_0 = sqrt(1 / 8), a_k = 1 / 2"""
    k, n = np.indices((8, 8))
    c = 0.5 * np.cos((2 * n + 1) * k * math.pi / 16)
    c[0, :] = math.sqrt(1 / 8)
    return c


C8 = dct_matrix()


def T(x):
    """orthonormal 8x8 DCT-II of [..., 8, 8] blocks"""
    return C8 @ x @ C8.T


def blocks_of(p, remainder=False):
    """[n, 8, 8] non-overlapping blocks of the plane, the right / bottom remainder left out (or zero-padded in: a seeded mistake)"""
    h, w = p.shape
    if remainder:
        p = np.pad(p, ((0, -h % 8), (0, -w % 8)))
        h, w = p.shape
    bh, bw = h // 8, w // 8
    return p[:8 * bh, :8 * bw].reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(bh * bw, 8, 8).astype(np.float64)


def vari(z, biased=False):
    """N / (N - 1) * sum (z - mean)^2 over the last two axes (biased: without the N / (N - 1))"""
    n = z.shape[-1] * z.shape[-2]
    # sum (z - mean)^2 = (N sum z^2 - (sum z)^2) / N; on integers below 2^16 the numerator is exact in float64
    s = (n * (z * z).sum(axis=(-1, -2)) - z.sum(axis=(-1, -2)) ** 2) / n
    return s if biased else s * n / (n - 1)


def maskeff(z, mask, mistake=None):
    t = T(z)
    e = t * t * mask
    m = e.sum(axis=(-1, -2)) - e[..., 0, 0]
    b = mistake == "biased_variance"
    pop = vari(z, b)
    if mistake == "halves":
        parts = vari(z[..., :, 0:4], b) + vari(z[..., :, 4:8], b)
    else:
        parts = vari(z[..., 0:4, 0:4], b) + vari(z[..., 0:4, 4:8], b) + vari(z[..., 4:8, 4:8], b) + vari(z[..., 4:8, 0:4], b)
    pop = np.where(pop != 0, parts / np.where(pop != 0, pop, 1.0), 0.0)
    return np.sqrt(m * pop) / 32


class Sums(NamedTuple):
    s_hvs: float   # S2
    s_hvsm: float  # S1
    blocks: int


def sums(a, b, mistake=None):
    """a, b: integer sample planes [h, w] -> Sums"""
    assert mistake is None or mistake in MISTAKES
    csf, mask = (CSF.T, MASK.T) if mistake == "transposed_tables" else (CSF, MASK)
    A, B = blocks_of(a, mistake == "remainder"), blocks_of(b, mistake == "remainder")
    ma, mb = maskeff(A, mask, mistake), maskeff(B, mask, mistake)
    M = np.minimum(ma, mb) if mistake == "min_mask" else np.maximum(ma, mb)
    u = np.abs(T(A - B))
    s2 = ((u * csf) ** 2).sum()
    v = np.maximum(u - M[:, None, None] / mask, 0.0)
    if mistake != "masked_dc":
        v[:, 0, 0] = u[:, 0, 0]
    s1 = ((v * csf) ** 2).sum()
    return Sums(float(s2), float(s1), A.shape[0])


def psnr(s, blocks, bits):
    if s == 0:
        return math.inf
    peak = float((1 << bits) - 1)
    return 10.0 * math.log10(peak * peak * 64.0 * blocks / s)
