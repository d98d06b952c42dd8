"""TEST INFRASTRUCTURE ONLY: HaarPSI (grayscale) as DESIGN.md section 21 states it, in float64 numpy and in the PAPER's form -- the 2x2
mean, Haar filters of +-2^-k over 2^k x 2^k, values scaled to 0 .. 255, the local similarity (2 |r| |d| + C) / (r^2 + d^2 + C) with C = 30
averaged over the scales 1 and 2, sigmoid and logit with alpha = 4.2, weights max(|r_3|, |d_3|) -- written from that text and not from
the kernel, which evaluates 1 - similarity in integer units and 1 - sigmoid.  `mistake` seeds one deliberate error
(tests/test_haarpsi_cpu.py shows that each moves the score)."""
import math
from typing import NamedTuple

import numpy as np

C = 30.0
ALPHA = 4.2
MISTAKES = ("scipy_centring", "replicate", "weights_scale2", "logistic_per_scale", "c_unscaled")


def conv2_same(a, k, replicate=False, scipy_centring=False):
    """MATLAB's conv2(a, k, 'same') for the zero-padded plane: full(i) = sum_j k(j) a(i - j), and 'same' keeps the part of a's size that
    starts at element floor(n / 2) of the full result for a kernel side n.  scipy_centring: starts at floor((n - 1) / 2) instead, what
    scipy's convolve2d(mode='same') does (a seeded mistake: for even n the window reaches the other way); replicate: edge samples
    repeated instead of zeros (another)."""
    H, W = a.shape
    kh, kw = k.shape
    oy, ox = ((kh - 1) // 2, (kw - 1) // 2) if scipy_centring else (kh // 2, kw // 2)
    p = np.pad(a, ((kh, kh), (kw, kw)), mode="edge" if replicate else "constant")
    full = np.zeros((H + kh - 1, W + kw - 1))
    for i in range(kh):
        for j in range(kw):  # full[y, x] += k[i, j] * a[y - i, x - j], a's element (0, 0) at p[kh, kw]
            full += k[i, j] * p[kh - i:kh - i + H + kh - 1, kw - j:kw - j + W + kw - 1]
    return full[oy:oy + H, ox:ox + W]


def haar(scale):
    """the paper's vertical Haar filter of a scale: 2^-scale over 2^scale x 2^scale, the upper half positive"""
    n = 1 << scale
    f = np.full((n, n), 2.0 ** -scale)
    f[n // 2:] *= -1
    return f


def coefficients(y, mistake=None):
    """[orientation][scale - 1] -> the Haar coefficients of the decimated plane of y (float64 values on the 0 .. 255 scale)"""
    kw = dict(replicate=mistake == "replicate", scipy_centring=mistake == "scipy_centring")
    dec = conv2_same(y, np.full((2, 2), 0.25), **kw)[0::2, 0::2]
    return [[conv2_same(dec, f, **kw) for f in (haar(s) if o == 0 else haar(s).T for s in (1, 2, 3))] for o in (0, 1)]


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-ALPHA * x))


def logit(p):
    return math.log(p / (1.0 - p)) / ALPHA


class Ref(NamedTuple):
    haarpsi: float
    num: float       # sum sigmoid(similarity) * weight, paper units
    den: float       # sum weight
    sim: np.ndarray  # the unweighted local similarity (s_v + s_h) / 2, [h2, w2]


def haarpsi(a, b, bits, mistake=None):
    """a, b: integer sample planes [h, w] of depth `bits` -> Ref"""
    assert mistake is None or mistake in MISTAKES
    scale = 1.0 if mistake == "c_unscaled" else float(1 << (bits - 8))
    cr = coefficients(np.asarray(a, np.float64) / scale, mistake)
    cd = coefficients(np.asarray(b, np.float64) / scale, mistake)
    num = den = 0.0
    sims = []
    for o in (0, 1):
        per_scale = []
        for s in (0, 1):
            r, d = np.abs(cr[o][s]), np.abs(cd[o][s])
            per_scale.append((2 * r * d + C) / (r * r + d * d + C))
        sim = (per_scale[0] + per_scale[1]) / 2
        wsel = 1 if mistake == "weights_scale2" else 2
        wt = np.maximum(np.abs(cr[o][wsel]), np.abs(cd[o][wsel]))
        mapped = (sigmoid(per_scale[0]) + sigmoid(per_scale[1])) / 2 if mistake == "logistic_per_scale" else sigmoid(sim)
        num += float((mapped * wt).sum())
        den += float(wt.sum())
        sims.append(sim)
    score = math.nan if den == 0.0 else logit(num / den) ** 2
    return Ref(score, num, den, (sims[0] + sims[1]) / 2)


def pooled(refs):
    """the value of a sequence: the same function of the summed numerators and denominators"""
    num, den = sum(r.num for r in refs), sum(r.den for r in refs)
    return math.nan if den == 0.0 else logit(num / den) ** 2
