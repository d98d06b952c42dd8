"""TEST INFRASTRUCTURE ONLY: LDR-FLIP restated in float64 numpy from the text of DESIGN.md section 14 (Andersson et al., HPG 2020), not
from the kernel: whole-picture arrays, np.pad for the edge replication, np.cbrt / np.power for the transcendentals.

    flip(ref, dis, ppd)  ->  namespace(flip, color, feature, mean, min, max)      ref, dis: uint8 [h][w][3], sRGB

`mistake`: one of MISTAKES, a deliberately wrong reading of the text; tests/test_flip_cpu.py shows that each one is far outside the
tolerance the kernels are held to."""
import math
from types import SimpleNamespace

import numpy as np

DEFAULT_PPD = 0.7 * 3840 / 0.7 * math.pi / 180
MISTAKES = ("zero_pad", "no_clamp", "no_hunt", "redistribute_first", "one_cz_gaussian", "radius_9", "normalise_total", "no_sqrt2",
            "min_feature", "exponent_def")

M = np.array([[10135552 / 24577794, 8788810 / 24577794, 4435075 / 24577794],
              [2613072 / 12288897, 8788810 / 12288897, 887015 / 12288897],
              [1425312 / 73733382, 8788810 / 73733382, 70074185 / 73733382]])
ILL = np.array([0.950428545, 1.0, 1.088900371])
PC, PT = 0.4, 0.95


def radius(ppd=DEFAULT_PPD):
    return math.ceil(3 * math.sqrt(0.04 / (2 * math.pi ** 2)) * ppd), math.ceil(3 * 0.5 * 0.082 * ppd)


def srgb_to_linear(v8):
    c = np.asarray(v8, np.float64) / 255
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def to_nxyz(lin):
    """linear RGB [..., 3] -> XYZ over the illuminant"""
    return (lin @ M.T) / ILL


def ycxcz(nxyz):
    x, y, z = nxyz[..., 0], nxyz[..., 1], nxyz[..., 2]
    return np.stack([116 * y - 16, 500 * (x - y), 200 * (y - z)], -1)


def lab_f(t):
    d = 6 / 29
    return np.where(t > d ** 3, np.cbrt(np.maximum(t, 0)), t / (3 * d * d) + 4 / 29)


def hunt_lab(nxyz, hunt=True):
    f = lab_f(nxyz)
    L = 116 * f[..., 1] - 16
    a, b = 500 * (f[..., 0] - f[..., 1]), 200 * (f[..., 1] - f[..., 2])
    return np.stack([L, 0.01 * L * a, 0.01 * L * b], -1) if hunt else np.stack([L, a, b], -1)


def hyab(p, q):
    return np.abs(p[..., 0] - q[..., 0]) + np.sqrt((p[..., 1] - q[..., 1]) ** 2 + (p[..., 2] - q[..., 2]) ** 2)


def cmax(hunt=True):
    g = hunt_lab(to_nxyz(np.array([0.0, 1.0, 0.0])), hunt)
    b = hunt_lab(to_nxyz(np.array([0.0, 0.0, 1.0])), hunt)
    return float(hyab(g, b)) ** 0.7


def filt1(img, wt, axis, mode="edge"):
    """sum over k = -r .. r of wt[k + r] img[i + k] along `axis`; coordinates outside the picture clamp"""
    r = len(wt) // 2
    pad = [(0, 0)] * img.ndim
    pad[axis] = (r, r)
    p = np.pad(img, pad, mode="edge") if mode == "edge" else np.pad(img, pad, mode="constant")
    n = img.shape[axis]
    out = np.zeros(img.shape)
    for k in range(2 * r + 1):
        out += wt[k] * np.take(p, np.arange(k, k + n), axis=axis)
    return out


def sep(img, wx, wy, mode="edge"):
    """rows (the filter along x) then columns"""
    return filt1(filt1(img, wx, 1, mode), wy, 0, mode)


def spatial_filter(opp, ppd, mistake=None):
    r = radius(ppd)[0]
    if mistake == "radius_9":
        r = 9
    mode = "constant" if mistake == "zero_pad" else "edge"
    d = np.arange(-r, r + 1) / ppd

    def g(b):
        return np.exp(-math.pi ** 2 * d ** 2 / b)
    gy, gx, g1, g2 = g(0.0047), g(0.0053), g(0.04), g(0.025)
    a1, a2 = 34.1 * math.sqrt(math.pi / 0.04), 13.5 * math.sqrt(math.pi / 0.025)
    if mistake == "one_cz_gaussian":
        a2 = 0.0
    S = a1 * g1.sum() ** 2 + a2 * g2.sum() ** 2
    out = np.empty(opp.shape)
    out[..., 0] = sep(opp[..., 0], gy / gy.sum(), gy / gy.sum(), mode)
    out[..., 1] = sep(opp[..., 1], gx / gx.sum(), gx / gx.sum(), mode)
    out[..., 2] = a1 / S * sep(opp[..., 2], g1, g1, mode) + a2 / S * sep(opp[..., 2], g2, g2, mode)
    return out


def feature_norms(y, ppd, mistake=None):
    sd = 0.5 * 0.082 * ppd
    rf = radius(ppd)[1]
    mode = "constant" if mistake == "zero_pad" else "edge"
    k = np.arange(-rf, rf + 1).astype(np.float64)
    G = np.exp(-k ** 2 / (2 * sd ** 2))
    G /= G.sum()
    G1 = -k * G
    G2 = (k ** 2 / sd ** 2 - 1) * G

    def by_sign(v):
        if mistake == "normalise_total":
            return v / np.abs(v).sum()
        return np.where(v > 0, v / v[v > 0].sum(), v / -v[v < 0].sum())
    G1, G2 = by_sign(G1), by_sign(G2)
    edge = np.hypot(sep(y, G1, G, mode), sep(y, G, G1, mode))
    point = np.hypot(sep(y, G2, G, mode), sep(y, G, G2, mode))
    return edge, point


def flip(ref, dis, ppd=DEFAULT_PPD, mistake=None):
    assert mistake is None or mistake in MISTAKES
    ref, dis = np.asarray(ref), np.asarray(dis)
    assert ref.dtype == np.uint8 and ref.shape == dis.shape and ref.shape[2] == 3
    hunt = mistake != "no_hunt"
    side = []
    for img in (ref, dis):
        n = to_nxyz(srgb_to_linear(img))
        f = spatial_filter(ycxcz(n), ppd, mistake)
        yy = (f[..., 0] + 16) / 116
        back = np.stack([yy + f[..., 1] / 500, yy, yy - f[..., 2] / 200], -1)
        lin = (back * ILL) @ np.linalg.inv(M).T
        if mistake != "no_clamp":
            lin = np.clip(lin, 0, 1)
        side.append((hunt_lab(to_nxyz(lin), hunt), feature_norms(n[..., 1], ppd, mistake)))
    (lr, (er, pr)), (ld, (ed, pd)) = side
    cm = cmax(hunt)
    h = hyab(lr, ld)

    def redistribute(e, top):
        lim = PC * top
        return np.where(e < lim, e * PT / lim, PT + (e - lim) / (top - lim) * (1 - PT))
    if mistake == "redistribute_first":
        color = redistribute(h, cm ** (1 / 0.7)) ** 0.7
    else:
        color = redistribute(h ** 0.7, cm)
    pick = np.minimum if mistake == "min_feature" else np.maximum
    fd = pick(np.abs(er - ed), np.abs(pr - pd))
    feature = np.sqrt(fd if mistake == "no_sqrt2" else fd / math.sqrt(2))
    expo = feature if mistake == "exponent_def" else 1 - feature
    with np.errstate(divide="ignore", invalid="ignore"):
        fl = np.where(color > 0, np.power(np.maximum(color, 1e-300), expo), 0.0)
    return SimpleNamespace(flip=fl, color=color, feature=feature, mean=float(fl.sum() / fl.size), min=float(fl.min()), max=float(fl.max()))
