"""TEST INFRASTRUCTURE ONLY: VMAF's ADM as DESIGN.md section 11 states it, restated in plain numpy from that text (not from the
kernel).  Works on sample VALUES (int64 planes of depth D); the layouts are tests/adm_util.py's business.  Every plane is float32 and
every multiply and add is a separate float32 operation in the order of the text; the sums and the scores are float64."""
import math

import numpy as np

f32 = np.float32
LO = tuple(f32(v) for v in (0.482962913144690, 0.836516303737469, 0.224143868041857, -0.129409522550921))
HI = tuple(f32(v) for v in (-0.129409522550921, -0.224143868041857, 0.836516303737469, -0.482962913144690))
A = ((0.62171, 0.67234, 0.72709, 0.67234), (0.34537, 0.41317, 0.49428, 0.41317),
     (0.18004, 0.22727, 0.28688, 0.22727), (0.091401, 0.11792, 0.15214, 0.11792))
G = (1.501, 1.0, 0.534, 1.0)
COS2 = f32(math.cos(math.pi / 180.0) ** 2)
EPS = f32(1e-30)
W_CENTRE, W_NEIGHBOUR = f32(1.0 / 15.0), f32(1.0 / 30.0)
BANDS = ("h", "v", "d")


def supported(w, h, layout, bits):
    """what tm_adm_create accepts; everything else is TM_ERR_UNSUPPORTED"""
    if w < 32 or h < 32 or not 8 <= bits <= 16:
        return False
    return {"y8": bits == 8, "y16_msb": bits >= 9, "y16_low": bits >= 9, "y10_packed": bits == 10}[layout]


def mirror(p, n):
    return -p if p < 0 else (2 * n - p - 1 if p >= n else p)


def sizes(w, h):
    """[(w_s, h_s, bw_s, bh_s)] of the four scales"""
    out = []
    for _ in range(4):
        bw, bh = (w + 1) // 2, (h + 1) // 2
        out.append((w, h, bw, bh))
        w, h = bw, bh
    return out


def border(bw, bh):
    """(left, top, right, bottom): double arithmetic, C truncation"""
    left, top = int(bw * 0.1 - 0.5), int(bh * 0.1 - 0.5)
    return left, top, bw - left, bh - top


def q(lam, theta):
    r = 3.0 * 1080.0 * math.pi / 180.0
    t = math.log10(2.0 ** (lam + 1) * 0.401 * G[theta] / r)
    return 2.0 * 0.495 * 10.0 ** (0.466 * t * t) / A[lam][theta]


def weights(s):
    """rf_s of (h, v, d) as float32"""
    return f32(1.0 / q(s, 1)), f32(1.0 / q(s, 1)), f32(1.0 / q(s, 2))


def _taps(x, f):
    """tap sums over axis 0: out[i] = f0 x[m(2i-1)] + f1 x[m(2i)] + f2 x[m(2i+1)] + f3 x[m(2i+2)], one rounding per operation"""
    n = x.shape[0]
    rows = [[mirror(2 * i - 1 + k, n) for i in range((n + 1) // 2)] for k in range(4)]
    acc = f[0] * x[rows[0]]
    for k in (1, 2, 3):
        acc = acc + f[k] * x[rows[k]]
    assert acc.dtype == np.float32
    return acc


def dwt(x):
    """(a, v, h, d) of one picture (float32): vertical pass first"""
    L, Hh = _taps(x, LO), _taps(x, HI)
    # row-major copies: numpy adds a plane in memory order, and the sums of two planes are only comparable bit for bit in one order
    return tuple(np.ascontiguousarray(_taps(p.T, f).T) for p, f in ((L, LO), (L, HI), (Hh, LO), (Hh, HI)))


def decouple(o, t):
    """o, t: dicts of the h, v, d planes of reference and distorted -> (r, a) dicts"""
    r = {}
    with np.errstate(all="ignore"):
        for b in BANDS:
            k = t[b] / (o[b] + EPS)
            k = np.fmin(np.fmax(k, f32(0)), f32(1))
            r[b] = k * o[b]
        dp = o["h"] * t["h"] + o["v"] * t["v"]
        om = o["h"] * o["h"] + o["v"] * o["v"]
        tm = t["h"] * t["h"] + t["v"] * t["v"]
        flag = (dp >= 0) & (dp * dp >= (COS2 * om) * tm)
    for b in BANDS:
        e = r[b] * f32(100)
        lim = np.where(r[b] > 0, np.minimum(e, t[b]), np.where(r[b] < 0, np.maximum(e, t[b]), r[b]))
        r[b] = np.where(flag, lim, r[b]).astype(np.float32)
    a = {b: t[b] - r[b] for b in BANDS}
    return r, a


def threshold(a, rf):
    """thr plane: b outermost, rows top to bottom, columns left to right, one float32 accumulator; outside the plane: nothing"""
    bh, bw = a["h"].shape
    acc = np.zeros((bh, bw), np.float32)
    for rfb, b in zip(rf, BANDS):
        c = np.pad(np.abs(rfb * a[b]), 1)
        for dy in range(3):
            for dx in range(3):
                acc = acc + (W_CENTRE if dy == dx == 1 else W_NEIGHBOUR) * c[dy:dy + bh, dx:dx + bw]
    assert acc.dtype == np.float32
    return acc


def to_picture(samples, bits):
    x = np.asarray(samples).astype(np.float32) / f32(1 << (bits - 8)) - f32(128.0)
    assert x.dtype == np.float32
    return x


def adm(ref, dis, bits):
    """per scale: dict(a=(a_ref, a_dis), r=(h, v, d), add=(h, v, d), thr, o=(h, v, d), num=[3], den=[3], area)"""
    assert np.shape(ref) == np.shape(dis) and max(np.max(ref), np.max(dis)) < 1 << bits
    x, y = to_picture(ref, bits), to_picture(dis, bits)
    out = []
    for s in range(4):
        ax, vx, hx, dx = dwt(x)
        ay, vy, hy, dy = dwt(y)
        o, t = dict(h=hx, v=vx, d=dx), dict(h=hy, v=vy, d=dy)
        r, a = decouple(o, t)
        rf = weights(s)
        thr = threshold(a, rf)
        bh, bw = thr.shape
        left, top, right, bottom = border(bw, bh)
        num, den = [], []
        for rfb, b in zip(rf, BANDS):
            xx = np.maximum(np.abs(rfb * r[b]) - thr, f32(0)).astype(np.float64)[top:bottom, left:right]
            yy = np.abs(rfb * o[b]).astype(np.float64)[top:bottom, left:right]
            num.append(float(((xx * xx) * xx).sum()))
            den.append(float(((yy * yy) * yy).sum()))
        out.append(dict(a=(ax, ay), r=tuple(r[b] for b in BANDS), add=tuple(a[b] for b in BANDS), thr=thr, o=tuple(o[b] for b in BANDS),
                        num=num, den=den, area=(bottom - top) * (right - left)))
        x, y = ax, ay
    return out


def _cbrt(v):
    return float(np.cbrt(np.float64(v)))


def score(n, d):
    if n < 1e-10:
        n = 0.0
    if d < 1e-10:
        d = 0.0
    return 1.0 if d == 0.0 else n / d


def scores(num_cube, den_cube, w, h):
    """[adm_scale0 .. adm_scale3, adm2] from the 24 sums of a w x h pair"""
    nums, dens = [], []
    for s, (_, _, bw, bh) in enumerate(sizes(w, h)):
        left, top, right, bottom = border(bw, bh)
        c = _cbrt((bottom - top) * (right - left) / 32.0)
        n = d = 0.0
        for b in range(3):
            n += _cbrt(num_cube[s][b]) + c
            d += _cbrt(den_cube[s][b]) + c
        nums.append(n)
        dens.append(d)
    tn = td = 0.0
    for n, d in zip(nums, dens):
        tn, td = tn + n, td + d
    return [score(n, d) for n, d in zip(nums, dens)] + [score(tn, td)]
