"""TEST INFRASTRUCTURE ONLY: VMAF's integer motion as DESIGN.md section 9 states it, restated in plain numpy from that text (not from
the kernel).  Works on sample VALUES (int64 planes of depth D); the layouts are tests/motion_util.py's business."""
import numpy as np

F = (3571, 16004, 26386, 16004, 3571)


def supported(w, h, layout, bits):
    """what tm_motion_create accepts; everything else is TM_ERR_UNSUPPORTED"""
    if w < 3 or h < 3 or not 8 <= bits <= 16:
        return False
    return {"y8": bits == 8, "y16_msb": bits >= 9, "y16_low": bits >= 9, "y10_packed": bits == 10}[layout]


def mirror(i, n):
    a = abs(i)
    return a if a < n else 2 * n - a - 1


def blur(s, bits):
    """B of one picture: the vertical pass first, rounded to 16 bits, then the horizontal pass on the rounded values"""
    s = np.asarray(s, np.int64)
    h, w = s.shape
    assert w >= 3 and h >= 3 and 0 <= s.min() and s.max() < (1 << bits)
    rows = [[mirror(y - 2 + k, h) for y in range(h)] for k in range(5)]
    v = (sum(F[k] * s[rows[k], :] for k in range(5)) + (1 << (bits - 1))) >> bits
    cols = [[mirror(x - 2 + k, w) for x in range(w)] for k in range(5)]
    b = (sum(F[k] * v[:, cols[k]] for k in range(5)) + 32768) >> 16
    assert b.max() <= 65535
    return b


def from_sad(sad, w, h):
    """libvmaf's normalize_and_scale_sad, float casts included"""
    return float(np.float32(sad / 256.0) / np.float32(w * h))


def motion2(motion):
    """motion2[i] = min(motion[i], motion[i + 1]); the last one is its motion"""
    return [min(m, motion[i + 1]) if i + 1 < len(motion) else m for i, m in enumerate(motion)]


def sequence(pictures, bits):
    """[(sad, motion)] of the luma planes of one sequence"""
    out, prev = [], None
    for p in pictures:
        b = blur(p, bits)
        sad = 0 if prev is None else int(np.abs(b - prev).sum())
        out.append((sad, 0.0 if prev is None else from_sad(sad, b.shape[1], b.shape[0])))
        prev = b
    return out


def scores(pictures, bits):
    """(mean motion, mean motion2): the sequence scores"""
    m = [f[1] for f in sequence(pictures, bits)]
    return float(np.mean(m)), float(np.mean(motion2(m)))
