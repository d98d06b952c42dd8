"""TEST INFRASTRUCTURE ONLY: the float64 numpy restatement of DESIGN.md section 17 -- CIEDE2000 of limited-range 4:2:0 pictures --
written from the definition, not from the kernel.  `mistake=` seeds one deliberate error (MISTAKES): the tests check that each moves
some small picture beyond the tolerance.  `flip=True` evaluates dE00 as if the comparison |h'1 - h'2| <= 180 had gone the other way
(the hue difference wrapped / unwrapped and the mean hue moved by 180 degrees together): what an f32 evaluation may legitimately give
where the two hues are almost exactly opposite."""
from typing import NamedTuple

import numpy as np

MATRIX = {
    "bt709": (1.5748, 0.187324, 0.468124, 1.8556),
    "bt601": (1.402, 0.344136, 0.714136, 1.772),
    "libvmaf": (1.28033, 0.21482, 0.38059, 2.12798),
}
MISTAKES = ("no_G", "no_hbar_180", "dh_unwrapped", "rt_sign", "t_radians", "no_srgb_branch", "chroma_at_xy", "offsets_unscaled",
            "bt601_for_bt709", "kl_ignored")
NEAR_DEG = 1.0  # the branch flip rule: ||h'1 - h'2| - 180| below this


def lab(Y, U, V, bits=8, matrix="bt709", mistake=None):
    """sample values (arrays of one shape) -> (L, a, b)"""
    s = float(1 << (bits - 8))
    so = 1.0 if mistake == "offsets_unscaled" else s
    c = MATRIX["bt601" if (mistake == "bt601_for_bt709" and matrix == "bt709") else matrix]
    Y, U, V = (np.asarray(t, np.float64) for t in (Y, U, V))
    yn, un, vn = (Y - 16 * so) / (219 * s), (U - 128 * so) / (224 * s), (V - 128 * so) / (224 * s)
    rgb = [yn + c[0] * vn, yn - c[1] * un - c[2] * vn, yn + c[3] * un]

    def lin(t):
        p = np.power(np.maximum((t + 0.055) / 1.055, 0.0), 2.4)
        return p if mistake == "no_srgb_branch" else np.where(t <= 0.04045, t / 12.92, p)
    R, G, B = (lin(t) for t in rgb)
    X = 0.4124564 * R + 0.3575761 * G + 0.1804375 * B
    Yc = 0.2126729 * R + 0.7151522 * G + 0.0721750 * B
    Z = 0.0193339 * R + 0.1191920 * G + 0.9503041 * B

    def f(t):
        return np.where(t > 216 / 24389, np.cbrt(np.maximum(t, 0.0)), ((24389 / 27) * t + 16) / 116)
    fx, fy, fz = f(X / 0.95047), f(Yc), f(Z / 1.08883)
    return 116 * fy - 16, 500 * (fx - fy), 200 * (fy - fz)


def de00(lab1, lab2, k=(1.0, 1.0, 1.0), mistake=None, flip=False, parts=False):
    """dE00 of two Lab triples (arrays); parts=True: (dE, near, wrapped, dLp) with `near` the mask of the branch flip rule and
    `wrapped` where |h'1 - h'2| > 180"""
    L1, a1, b1 = (np.asarray(t, np.float64) for t in lab1)
    L2, a2, b2 = (np.asarray(t, np.float64) for t in lab2)
    kL, kC, kH = k
    if mistake == "kl_ignored":
        kL = 1.0
    C1, C2 = np.hypot(a1, b1), np.hypot(a2, b2)
    cb7 = ((C1 + C2) / 2) ** 7
    G = 0.5 * (1 - np.sqrt(cb7 / (cb7 + 25.0 ** 7)))
    if mistake == "no_G":
        G = np.zeros_like(G)
    a1p, a2p = (1 + G) * a1, (1 + G) * a2
    C1p, C2p = np.hypot(a1p, b1), np.hypot(a2p, b2)

    def hue(b, a):
        h = np.degrees(np.arctan2(b, a))
        h = np.where(h < 0, h + 360, h)
        return np.where((a == 0) & (b == 0), 0.0, h)
    h1, h2 = hue(b1, a1p), hue(b2, a2p)
    dLp, dCp = L2 - L1, C2p - C1p
    prod = C1p * C2p
    nz = prod != 0
    d = h2 - h1
    wrapped = np.abs(h1 - h2) > 180
    wr = wrapped ^ bool(flip)
    dh = np.where(wr, d - 360 * np.sign(d), d)
    if mistake == "dh_unwrapped":
        dh = d
    dh = np.where(nz, dh, 0.0)
    dHp = 2 * np.sqrt(prod) * np.sin(np.radians(dh / 2))
    Lb, Cbp = (L1 + L2) / 2, (C1p + C2p) / 2
    hs = h1 + h2
    hb = np.where(wr, np.where(hs < 360, hs / 2 + 180, hs / 2 - 180), hs / 2)
    if mistake == "no_hbar_180":
        hb = hs / 2
    hb = np.where(nz, hb, hs)
    ang = (lambda t: t) if mistake == "t_radians" else np.radians
    T = 1 - 0.17 * np.cos(ang(hb - 30)) + 0.24 * np.cos(ang(2 * hb)) + 0.32 * np.cos(ang(3 * hb + 6)) - 0.20 * np.cos(ang(4 * hb - 63))
    dth = 30 * np.exp(-(((hb - 275) / 25) ** 2))
    c7 = Cbp ** 7
    RC = 2 * np.sqrt(c7 / (c7 + 25.0 ** 7))
    SL = 1 + 0.015 * (Lb - 50) ** 2 / np.sqrt(20 + (Lb - 50) ** 2)
    SC, SH = 1 + 0.045 * Cbp, 1 + 0.015 * Cbp * T
    RT = -np.sin(np.radians(2 * dth)) * RC
    if mistake == "rt_sign":
        RT = -RT
    x, y, z = dLp / (kL * SL), dCp / (kC * SC), dHp / (kH * SH)
    de = np.sqrt(np.maximum(x * x + y * y + z * z + RT * y * z, 0.0))
    if parts:
        near = nz & (np.abs(np.abs(h1 - h2) - 180) < NEAR_DEG)
        return de, near, wrapped & nz, dLp
    return de


def score(de_sum, n):
    if de_sum == 0:
        return 100.0
    return min(45 - 20 * np.log10(de_sum / n), 100.0)


class Want(NamedTuple):
    map: np.ndarray      # float64 [h, w]
    alt: np.ndarray      # the same under the other hue branch (flip=True)
    near: np.ndarray     # bool [h, w]: where the branch flip rule accepts either
    wrapped: np.ndarray  # bool [h, w]: |h'1 - h'2| > 180 (and C'1 C'2 > 0)
    de_sum: float
    de_mean: float
    de_max: float
    score: float


def up(C, w, h, mistake=None):
    """the chroma plane at every luma position: sample (x >> 1, y >> 1)"""
    C = np.asarray(C)
    if mistake == "chroma_at_xy":
        y, x = np.indices((h, w))
        return C[np.minimum(y, C.shape[0] - 1), np.minimum(x, C.shape[1] - 1)]
    return np.repeat(np.repeat(C, 2, 0), 2, 1)[:h, :w]


def picture(ref, dis, bits=8, matrix="bt709", k=(1.0, 1.0, 1.0), mistake=None):
    """ref, dis: (Y [h, w], Cb, Cr [(h + 1) / 2, (w + 1) / 2]) sample values -> Want"""
    h, w = np.asarray(ref[0]).shape
    labs = [lab(p[0], up(p[1], w, h, mistake), up(p[2], w, h, mistake), bits, matrix, mistake) for p in (ref, dis)]
    m, near, wrapped, _ = de00(labs[0], labs[1], k, mistake, parts=True)
    alt = de00(labs[0], labs[1], k, mistake, flip=True)
    s = float(np.sum(m))
    return Want(m, alt, near, wrapped, s, s / (w * h), float(m.max()), float(score(s, w * h)))
