"""TEST INFRASTRUCTURE ONLY: VMAF's VIF as DESIGN.md section 10 states it, restated in plain numpy from that text (not from the
kernel).  Works on sample VALUES (int64 planes of depth D); the layouts are tests/vif_util.py's business.  Integers in uint64 /
int64, the statistic in float64."""
import numpy as np

F = ((489, 935, 1640, 2640, 3896, 5274, 6547, 7455, 7784, 7455, 6547, 5274, 3896, 2640, 1640, 935, 489),
     (1244, 3663, 7925, 12590, 14692, 12590, 7925, 3663, 1244),
     (3571, 16004, 26386, 16004, 3571),
     (10904, 43728, 10904))


def supported(w, h, layout, bits):
    """what tm_vif_create accepts; everything else is TM_ERR_UNSUPPORTED"""
    if w < 32 or h < 32 or not 8 <= bits <= 16:
        return False
    return {"y8": bits == 8, "y16_msb": bits >= 9, "y16_low": bits >= 9, "y10_packed": bits == 10}[layout]


def mirror(i, n):
    return -i if i < 0 else (2 * (n - 1) - i if i >= n else i)


def sizes(w, h):
    out = [(w, h)]
    for _ in range(3):
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


def _vertical(p, f):
    """sum_k f[k] p[mirror(r - h + k)][c] for every r, c; uint64"""
    n, half = p.shape[0], len(f) // 2
    acc = np.zeros(p.shape, np.uint64)
    for k, c in enumerate(f):
        acc += np.uint64(c) * p[[mirror(r - half + k, n) for r in range(n)], :]
    return acc


def _horizontal(p, f):
    return _vertical(p.T, f).T


def decimate(x, s, bits):
    """the scale-s picture from the scale-(s-1) picture x (s >= 1): F_s, vertical pass first, even positions"""
    x = np.asarray(x, np.uint64)
    sh = bits if s == 1 else 16
    t = (_vertical(x, F[s]) + np.uint64(1 << (sh - 1))) >> np.uint64(sh)
    u = (_horizontal(t, F[s]) + np.uint64(32768)) >> np.uint64(16)
    h, w = x.shape
    return u[0:2 * (h // 2):2, 0:2 * (w // 2):2]


def moments(x, y, s, bits):
    """(s1, s2, s12) of one scale: int32 planes; also the intermediate planes for the hand-derived tests"""
    x, y = np.asarray(x, np.uint64), np.asarray(y, np.uint64)
    f = F[s]
    inb = bits if s == 0 else 16
    q = 2 * (bits - 8) if s == 0 else 16
    r = (1 << (q - 1)) if q else 0
    m1v = (_vertical(x, f) + np.uint64(1 << (inb - 1))) >> np.uint64(inb)
    m2v = (_vertical(y, f) + np.uint64(1 << (inb - 1))) >> np.uint64(inb)
    xxv = (_vertical(x * x, f) + np.uint64(r)) >> np.uint64(q)
    yyv = (_vertical(y * y, f) + np.uint64(r)) >> np.uint64(q)
    xyv = (_vertical(x * y, f) + np.uint64(r)) >> np.uint64(q)
    assert max(m1v.max(), m2v.max()) < 1 << 16 and max(xxv.max(), yyv.max(), xyv.max()) < 1 << 32
    m1, m2 = _horizontal(m1v, f), _horizontal(m2v, f)
    assert max(m1.max(), m2.max()) < 1 << 32
    xx = (_horizontal(xxv, f) + np.uint64(32768)) >> np.uint64(16)
    yy = (_horizontal(yyv, f) + np.uint64(32768)) >> np.uint64(16)
    xy = (_horizontal(xyv, f) + np.uint64(32768)) >> np.uint64(16)
    assert max(xx.max(), yy.max(), xy.max()) < 1 << 32
    half = np.uint64(1 << 31)

    def i32(a, b):  # (int32)(a - b) of two uint32 values
        return ((a.astype(np.int64) - b.astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    s1 = i32(xx, (m1 * m1 + half) >> np.uint64(32))
    s2 = i32(yy, (m2 * m2 + half) >> np.uint64(32))
    s12 = i32(xy, (m1 * m2 + half) >> np.uint64(32))
    return (s1, s2, s12), dict(m1v=m1v, m2v=m2v, xxv=xxv, yyv=yyv, xyv=xyv, m1=m1, m2=m2, xx=xx, yy=yy, xy=xy)


def statistic(s1, s2, s12):
    """(num, den) planes in float64, the operations in the definition's order"""
    a, b, c = np.maximum(s1, 0).astype(np.int64), np.maximum(s2, 0).astype(np.int64), s12.astype(np.int64)
    A, B, C = a / 65536.0, b / 65536.0, c / 65536.0
    low = a < 131072
    with np.errstate(all="ignore"):
        den = np.where(low, 1.0, np.log2(1.0 + A / 2.0))
        g = C / (A + 1e-10)
        sv = np.maximum(B - g * C, 1e-10)
        g = np.minimum(g, 100.0)
        hi = np.log2(1.0 + g * g * A / (sv + 2.0))
    num = np.where(low, 1.0 - B * (4.0 / 65025.0), np.where((c <= 0) | (b == 0), 0.0, hi))
    return num, den


def vif(ref, dis, bits):
    """per scale: dict(planes=(s1, s2, s12), num, den)"""
    x, y = np.asarray(ref, np.uint64), np.asarray(dis, np.uint64)
    assert x.shape == y.shape and max(x.max(), y.max()) < 1 << bits
    out = []
    for s in range(4):
        if s:
            x, y = decimate(x, s, bits), decimate(y, s, bits)
        planes, _ = moments(x, y, s, bits)
        num, den = statistic(*planes)
        out.append(dict(planes=planes, num=float(num.sum()), den=float(den.sum())))
    return out


def scores(per_scale):
    """[vif_scale0 .. vif_scale3, vif]"""
    num, den = [p["num"] for p in per_scale], [p["den"] for p in per_scale]
    n = d = 0.0
    for a, b in zip(num, den):
        n, d = n + a, d + b
    return [a / b for a, b in zip(num, den)] + [n / d]
