"""TEST INFRASTRUCTURE ONLY: GMSD as DESIGN.md section 20 states it, in float64 numpy and in the PAPER's form -- the 2x2 mean and the
Prewitt responses divided by 4 and by 3, values scaled to 0 .. 255, GMS = (2 m_r m_d + c) / (m_r^2 + m_d^2 + c) with c = 170 -- written
from that text and not from the kernel, which evaluates e = 1 - GMS in integer units.  `mistake` seeds one deliberate error
(tests/test_gmsd_cpu.py shows that each moves a number)."""
import math
from typing import NamedTuple

import numpy as np

T = 170.0
PREWITT = np.array([[1, 0, -1], [1, 0, -1], [1, 0, -1]], np.float64) / 3
MISTAKES = ("replicate", "phase1", "c_unscaled", "halo_wrong_side", "byte_behind")


def conv2_same(a, k, replicate=False):
    """MATLAB's conv2(a, k, 'same'): the true convolution (kernel flipped) of the zero-padded plane, the central part the size of `a`,
    which for an even kernel side n starts at element n / 2 of the full result.  replicate: edge samples repeated instead of zeros (a
    seeded mistake)"""
    H, W = a.shape
    kh, kw = k.shape
    p = np.pad(a, ((kh, kh), (kw, kw)), mode="edge" if replicate else "constant")
    out = np.zeros((H, W))
    for i in range(kh):
        for j in range(kw):  # out[y, x] += k[i, j] * a[y + kh // 2 - i, x + kw // 2 - j]
            y0, x0 = kh + kh // 2 - i, kw + kw // 2 - j
            out += k[i, j] * p[y0:y0 + H, x0:x0 + W]
    return out


def magnitude(y, mistake=None, tile=(64, 32)):
    """the gradient magnitude of the decimated plane of y (float64 values on the 0 .. 255 scale)"""
    rep = mistake == "replicate"
    if mistake == "byte_behind" and y.shape[1] % 2:  # the sample behind an odd row's last one: the next row's first in a tight plane
        nxt = np.vstack([y[1:, :1], np.zeros((1, 1))])
        ave = conv2_same(np.hstack([y, nxt]), np.full((2, 2), 0.25))[:, :-1]
    else:
        ave = conv2_same(y, np.full((2, 2), 0.25), rep)
    dec = ave[1::2, 1::2] if mistake == "phase1" else ave[0::2, 0::2]
    gx, gy = conv2_same(dec, PREWITT, rep), conv2_same(dec, PREWITT.T, rep)
    if mistake == "halo_wrong_side":  # a tile's right halo column taken from its own left side
        tw = tile[0]
        z = np.pad(dec, 1)
        for x in range(tw - 1, dec.shape[1] - 1, tw):
            wrong = z[:, x + 2 - tw]  # decimated column x + 1 - tw (z's columns are one to the right)
            left = z[:, x]            # ... x - 1
            d = wrong - left
            gx[:, x] = (d[:-2] + d[1:-1] + d[2:]) / 3
    return np.sqrt(gx * gx + gy * gy)


class Ref(NamedTuple):
    gmsd: float
    gmsm: float
    n: int
    gms: np.ndarray  # the map, [h2, w2]


def gmsd(a, b, bits, mistake=None, population=False, tile=(64, 32)):
    """a, b: integer sample planes [h, w] of depth `bits` -> Ref"""
    assert mistake is None or mistake in MISTAKES
    scale = 1.0 if mistake == "c_unscaled" else float(1 << (bits - 8))
    mr = magnitude(np.asarray(a, np.float64) / scale, mistake, tile)
    md = magnitude(np.asarray(b, np.float64) / scale, mistake, tile)
    gms = (2 * mr * md + T) / (mr * mr + md * md + T)
    n = gms.size
    return Ref(float(np.std(gms, ddof=0 if population else 1)), float(np.mean(gms)), n, gms)


def pooled(refs, population=False):
    """(gmsd, gmsm) of a sequence: over all positions of all pairs"""
    allv = np.concatenate([r.gms.reshape(-1) for r in refs])
    return float(np.std(allv, ddof=0 if population else 1)), float(np.mean(allv))


def score(e1, e2, n, population=False):
    """the host function tm_gmsd_score, restated"""
    if n < 2:
        return math.nan
    return math.sqrt(max(0.0, (e2 - e1 * e1 / n) / (n if population else n - 1)))
