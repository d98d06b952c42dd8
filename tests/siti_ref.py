"""TEST INFRASTRUCTURE ONLY: ITU-T P.910 spatial / temporal information as DESIGN.md section 19 states it, restated from that text (not
from the kernel) twice: literally, in numpy int64 and Python integers (every sum exact), and independently in float64 (Sobel by slicing,
np.std).  Works on sample VALUES (int64 planes of depth D); the layouts are tests/siti_util.py's business.

`mistake=` seeds one wrong reading of the text into the integer restatement; tests/test_siti_cpu.py shows that each is caught."""
import math

import numpy as np

MAX_SAMPLES = 1 << 26
MISTAKES = ("same_kernel_twice", "border", "sample_std", "truncate", "ti_interior", "no_shift")


def supported(w, h, layout, bits):
    """what tm_siti_create accepts; everything else is TM_ERR_UNSUPPORTED"""
    if w < 3 or h < 3 or w * h > MAX_SAMPLES or not 8 <= bits <= 16:
        return False
    return {"y8": bits == 8, "y16_msb": bits >= 9, "y16_low": bits >= 9, "y10_packed": bits == 10}[layout]


def sobel(F, mistake=None):
    """(gx, gy) at the interior positions: [-1 0 1; -2 0 2; -1 0 1] and its transpose on the code values"""
    F = np.asarray(F, np.int64)
    if mistake == "border":  # replicate the edge and compute everywhere
        F = np.pad(F, 1, mode="edge")
    h, w = F.shape
    gx = np.zeros((h - 2, w - 2), np.int64)
    gy = np.zeros((h - 2, w - 2), np.int64)
    kx = ((-1, 0, 1), (-2, 0, 2), (-1, 0, 1))
    if mistake == "same_kernel_twice":  # gy computed with gx's kernel (a true swap of gx and gy could not be seen in gx^2 + gy^2)
        ky = kx
    else:
        ky = tuple(zip(*kx))
    for j in range(3):
        for i in range(3):
            win = F[j:h - 2 + j, i:w - 2 + i]
            gx += kx[j][i] * win
            gy += ky[j][i] * win
    return gx, gy


def quantise(M, mistake=None):
    """q of one Python integer M >= 0: the one integer with q^2 - q < M <= q^2 + q (M = 0: q = 0)"""
    q = math.isqrt(M)  # floor
    if mistake == "truncate":
        return q
    if M > q * q + q:
        q += 1
    assert M == 0 or q * q - q < M <= q * q + q
    return q


def quantise_plane(M, mistake=None):
    """quantise() of every element of an int64 array, by exact integer arithmetic: isqrt through a float estimate corrected with the
    defining inequalities, so that the result does not lean on any float rounding"""
    M = np.asarray(M, np.int64)
    q = np.floor(np.sqrt(M.astype(np.float64))).astype(np.int64)
    q = np.where(q * q > M, q - 1, q)
    q = np.where((q + 1) * (q + 1) <= M, q + 1, q)
    assert (q * q <= M).all() and ((q + 1) * (q + 1) > M).all()
    if mistake == "truncate":
        return q
    q = np.where(M > q * q + q, q + 1, q)
    assert ((M == 0) | ((q * q - q < M) & (M <= q * q + q))).all()
    return q


def si_sums(F, bits, mistake=None):
    """(S1, S2, n_si) of one picture, Python integers"""
    F = np.asarray(F, np.int64)
    assert F.min() >= 0 and F.max() < (1 << bits)
    gx, gy = sobel(F, mistake)
    m2 = gx * gx + gy * gy
    assert int(m2.max()) < 1 << (2 * bits + 5)
    M = m2 if mistake == "no_shift" else m2 << (2 * (16 - bits))
    assert int(M.max()) < 1 << 37
    q = quantise_plane(M, mistake)
    return sum(int(v) for v in q.ravel()), sum(int(v) * int(v) for v in q.ravel()), q.size


def ti_sums(F, P, mistake=None):
    """(T1, T2, n) of picture F after picture P, Python integers"""
    d = np.asarray(F, np.int64) - np.asarray(P, np.int64)
    if mistake == "ti_interior":
        d = d[1:-1, 1:-1]
    return int(d.sum()), int((d * d).sum()), d.size


def _std(a, b, n, mistake=None):
    """sqrt(n b - a^2) / n with the radicand an exact integer"""
    rad = n * b - a * a
    assert rad >= 0
    if mistake == "sample_std":
        return math.sqrt(rad / (n * (n - 1)))
    return math.sqrt(rad) / n


def si(s1, s2, n_si, gain=1.0, mistake=None):
    return gain * _std(s1, s2, n_si, mistake) / 256.0


def ti(t1, t2, n, bits, gain=1.0, mistake=None):
    return gain * _std(t1, t2, n, mistake) / 2.0 ** (bits - 8)


def sequence(pictures, bits, mistake=None):
    """[dict(s1, s2, t1, t2, ti_valid, si, ti)] of the luma planes of one sequence"""
    out, prev = [], None
    for p in pictures:
        p = np.asarray(p, np.int64)
        s1, s2, n_si = si_sums(p, bits, mistake)
        if prev is None:
            t1, t2, n, valid = 0, 0, p.size, 0
        else:
            t1, t2, n = ti_sums(p, prev, mistake)
            valid = 1
        out.append(dict(s1=s1, s2=s2, t1=t1, t2=t2, ti_valid=valid, si=si(s1, s2, n_si, 1.0, mistake),
                        ti=ti(t1, t2, n, bits, 1.0, mistake) if valid else 0.0))
        prev = p
    return out


def sums(pictures, bits):
    """[(s1, s2, t1, t2, ti_valid)]: what the device must reproduce exactly"""
    return [(f["s1"], f["s2"], f["t1"], f["t2"], f["ti_valid"]) for f in sequence(pictures, bits)]


def sequence_scores(frames):
    """P.910: SI = max over pictures, TI = max over pictures 1 .. n-1 (0 for a single picture)"""
    return max(f["si"] for f in frames), max([f["ti"] for f in frames if f["ti_valid"]], default=0.0)


# ---- the second, independent statement: float64 --------------------------------------------------------------------------------
def si_f64(F, bits):
    """np.std of the float Sobel magnitude over the interior, on the 8-bit scale"""
    F = np.asarray(F, np.float64)
    gx = (F[:-2, 2:] + 2 * F[1:-1, 2:] + F[2:, 2:]) - (F[:-2, :-2] + 2 * F[1:-1, :-2] + F[2:, :-2])
    gy = (F[2:, :-2] + 2 * F[2:, 1:-1] + F[2:, 2:]) - (F[:-2, :-2] + 2 * F[:-2, 1:-1] + F[:-2, 2:])
    return float(np.std(np.sqrt(gx * gx + gy * gy))) / 2.0 ** (bits - 8)


def ti_f64(F, P, bits):
    return float(np.std(np.asarray(F, np.float64) - np.asarray(P, np.float64))) / 2.0 ** (bits - 8)
