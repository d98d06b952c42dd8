"""TEST INFRASTRUCTURE ONLY: the float64 numpy restatement of DESIGN.md section 22 -- the BT.2124 colour difference dE ITP of
limited-range 4:2:0 HDR pictures -- written from the definition, not from the kernel.  `mistake=` seeds one deliberate error
(MISTAKES): the tests check that each moves some small picture beyond the tolerance."""
from typing import NamedTuple

import numpy as np

M1, M2 = 2610 / 16384, 2523 / 32
C1, C2, C3 = 3424 / 4096, 2413 / 128, 2392 / 128
HLG_A = 0.17883277
HLG_B = 1 - 4 * HLG_A
HLG_C = 0.5 - HLG_A * np.log(4 * HLG_A)
HLG_LW = 1000.0
BT2020 = (1.4746, 0.16455, 0.57135, 1.8814)
BT709 = (1.5748, 0.187324, 0.468124, 1.8556)
LMS = np.array([[1688, 2146, 262], [683, 2951, 462], [99, 309, 3688]], np.float64)
ICTCP = np.array([[2048, 2048, 0], [6610, -13613, 7003], [17933, -17390, -543]], np.float64)
MISTAKES = ("ct_not_halved", "m1_m2_exchanged", "no_clamp", "chroma_at_xy", "bt709_matrix", "no_720")


def pq_eotf(e):
    """PQ signal in [0, 1] -> cd/m2"""
    p = np.power(np.asarray(e, np.float64), 1 / M2)
    with np.errstate(invalid="ignore"):  # a signal above 1 (the seeded mistake without the clamp) has no display light: NaN
        return 10000.0 * np.power(np.maximum(p - C1, 0.0) / (C2 - C3 * p), 1 / M1)


def pq_inv_eotf(f, mistake=None):
    """cd/m2 -> PQ signal"""
    m1, m2 = (M2, M1) if mistake == "m1_m2_exchanged" else (M1, M2)
    y = np.power(np.asarray(f, np.float64) / 10000.0, m1)
    return np.power((C1 + C2 * y) / (1 + C3 * y), m2)


def hlg_scene(e):
    """HLG signal in [0, 1] -> scene light in [0, 1]"""
    e = np.asarray(e, np.float64)
    return np.where(e <= 0.5, e * e / 3, (np.exp((np.maximum(e, 0.5) - HLG_C) / HLG_A) + HLG_B) / 12)


def hlg_display(rgb):
    """HLG R'G'B' signals -> R, G, B in cd/m2 on the 1000 cd/m2 display (system gamma 1.2)"""
    R, G, B = (hlg_scene(t) for t in rgb)
    ys = 0.2627 * R + 0.6780 * G + 0.0593 * B
    k = np.where(ys > 0, HLG_LW * np.power(np.where(ys > 0, ys, 1.0), 0.2), 0.0)
    return k * R, k * G, k * B


def ictcp(Y, U, V, bits=8, transfer="pq", mistake=None):
    """sample values (arrays of one shape) -> (I, Ct, Cp)"""
    s = float(1 << (bits - 8))
    c = BT709 if mistake == "bt709_matrix" else BT2020
    Y, U, V = (np.asarray(t, np.float64) for t in (Y, U, V))
    yn, un, vn = (Y - 16 * s) / (219 * s), (U - 128 * s) / (224 * s), (V - 128 * s) / (224 * s)
    rgb = [yn + c[0] * vn, yn - c[1] * un - c[2] * vn, yn + c[3] * un]
    if mistake == "no_clamp":  # only what keeps the curves defined: nothing below 0
        rgb = [np.maximum(t, 0.0) for t in rgb]
    else:
        rgb = [np.clip(t, 0.0, 1.0) for t in rgb]
    F = hlg_display(rgb) if transfer == "hlg" else tuple(pq_eotf(t) for t in rgb)
    lms = [(LMS[k, 0] * F[0] + LMS[k, 1] * F[1] + LMS[k, 2] * F[2]) / 4096 for k in range(3)]
    n = [pq_inv_eotf(t, mistake) for t in lms]
    return tuple((ICTCP[k, 0] * n[0] + ICTCP[k, 1] * n[1] + ICTCP[k, 2] * n[2]) / 4096 for k in range(3))


def de(a, b, mistake=None):
    """dE ITP of two (I, Ct, Cp) triples (arrays)"""
    di, dt, dp = (np.asarray(b[k], np.float64) - np.asarray(a[k], np.float64) for k in range(3))
    if mistake != "ct_not_halved":
        dt = dt / 2
    return (1.0 if mistake == "no_720" else 720.0) * np.sqrt(di * di + dt * dt + dp * dp)


class Want(NamedTuple):
    map: np.ndarray  # float64 [h, w]
    de_sum: float
    de_mean: float
    de_max: float


def up(C, w, h, mistake=None):
    """the chroma plane at every luma position: sample (x >> 1, y >> 1)"""
    C = np.asarray(C)
    if mistake == "chroma_at_xy":
        y, x = np.indices((h, w))
        return C[np.minimum(y, C.shape[0] - 1), np.minimum(x, C.shape[1] - 1)]
    return np.repeat(np.repeat(C, 2, 0), 2, 1)[:h, :w]


def picture(ref, dis, bits=8, transfer="pq", mistake=None):
    """ref, dis: (Y [h, w], Cb, Cr [(h + 1) / 2, (w + 1) / 2]) sample values -> Want"""
    h, w = np.asarray(ref[0]).shape
    t = [ictcp(p[0], up(p[1], w, h, mistake), up(p[2], w, h, mistake), bits, transfer, mistake) for p in (ref, dis)]
    m = de(t[0], t[1], mistake)
    s = float(np.sum(m))
    return Want(m, s, s / (w * h), float(m.max()))
