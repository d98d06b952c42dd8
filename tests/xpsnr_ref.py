"""TEST INFRASTRUCTURE ONLY: a literal CPU restatement of XPSNR as DESIGN.md section 8 defines it (believed to match ffmpeg's vf_xpsnr;
unpinned).  A block loop in raster order with numpy int64 sums and float64 weights, written from the definition's text, not from the
kernels (turbo-metrics_amd/csrc/tm_xpsnr_kernels.h cites this file tap for tap, and the tests hold the two against each other).

Pictures are (Y, Cb, Cr) integer arrays holding the sample values the metric sees (D bits)."""
import math

import numpy as np


def block_size(w, h):
    r = w * h / (3840 * 2160)
    return 4 * int(32 * math.sqrt(r) + 0.5)


def avg_act(w, h, bits):
    r = w * h / (3840 * 2160)
    return math.sqrt(16 * 2 ** (2 * bits - 9) / math.sqrt(max(1e-5, r)))


def bval_of(w, h):
    return 2 if w * h > 2048 * 1152 else 1


def second_order(fps_num, fps_den):
    return fps_num // fps_den >= 32


def sa_hp1(o, xa, ya, wa, ha):
    """bval = 1: sum over ya <= y < ha, xa <= x < wa of |12 o - 2 (x-1, x+1, y-1, y+1 neighbours) - (4 diagonal neighbours)|.
    `o` is the reference luma padded so that o[y + 2, x + 2] is block-relative sample (x, y)."""
    c = lambda dx, dy: o[ya + 2 + dy:ha + 2 + dy, xa + 2 + dx:wa + 2 + dx]
    f = 12 * c(0, 0) - 2 * (c(-1, 0) + c(1, 0) + c(0, -1) + c(0, 1)) - (c(-1, -1) + c(1, -1) + c(-1, 1) + c(1, 1))
    return int(np.abs(f).sum())


def sa_hp2(o, xa, ya, wa, ha):
    """bval = 2: ffmpeg's `highds` taps (k_xpsnr_blocks states the same sum), over y = ya, ya+2, .. < ha and x = xa, xa+2, .. < wa"""
    c = lambda dx, dy: o[ya + 2 + dy:ha + 2 + dy:2, xa + 2 + dx:wa + 2 + dx:2]
    f = (12 * (c(0, 0) + c(1, 0) + c(0, 1) + c(1, 1))
         - 3 * (c(-1, 0) + c(2, 0) + c(-1, 1) + c(2, 1))
         - 3 * (c(0, -1) + c(1, -1) + c(0, 2) + c(1, 2))
         - 2 * (c(-1, -1) + c(2, -1) + c(-1, 2) + c(2, 2))
         - (c(-1, -2) + c(0, -2) + c(1, -2) + c(2, -2)
            + c(-1, 3) + c(0, 3) + c(1, 3) + c(2, 3)
            + c(-2, -1) + c(-2, 0) + c(-2, 1) + c(-2, 2)
            + c(3, -1) + c(3, 0) + c(3, 1) + c(3, 2)))
    return int(np.abs(f).sum())


def cells(a):
    """sums of the 2x2 cells at even (x, y)"""
    return a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]


def frame_wsse(ref, dis, m1, m2, bits, second):
    """one frame: (wsse64 of Y, Cb, Cr).  ref / dis: (Y, Cb, Cr); m1 / m2: the previous and second-previous reference luma."""
    Y = np.asarray(ref[0], np.int64)
    h, w = Y.shape
    b = block_size(w, h)
    if b < 4:
        return tuple(int(((np.asarray(r, np.int64) - np.asarray(d, np.int64)) ** 2).sum()) for r, d in zip(ref, dis))
    bval = bval_of(w, h)
    m1 = np.asarray(m1, np.int64); m2 = np.asarray(m2, np.int64)
    pad = np.zeros((h + 4, w + 4), np.int64)
    pad[2:-2, 2:-2] = Y
    wblk = -(-w // b)
    weights, sses = [], []
    i = 0
    for y0 in range(0, h, b):
        bh = min(b, h - y0)
        for x0 in range(0, w, b):
            bw = min(b, w - x0)
            o = Y[y0:y0 + bh, x0:x0 + bw]
            sses.append(int(((o - np.asarray(dis[0], np.int64)[y0:y0 + bh, x0:x0 + bw]) ** 2).sum()))
            xa = 0 if x0 > 0 else bval
            ya = 0 if y0 > 0 else bval
            wa = bw if x0 + bw < w else bw - bval
            ha = bh if y0 + bh < h else bh - bval
            ms = 1.0
            if not (wa <= xa or ha <= ya):
                op = pad[y0:y0 + bh + 4, x0:x0 + bw + 4]
                sa = sa_hp1(op, xa, ya, wa, ha) if bval == 1 else sa_hp2(op, xa, ya, wa, ha)
                p1 = m1[y0:y0 + bh, x0:x0 + bw]
                p2 = m2[y0:y0 + bh, x0:x0 + bw]
                if bval == 2:
                    o, p1, p2 = cells(o), cells(p1), cells(p2)
                t = o - 2 * p1 + p2 if second else o - p1
                ta = 2 * int(np.abs(t).sum())  # gamma = 2
                ms = sa / ((wa - xa) * (ha - ya)) + ta / (bw * bh)
                ms = max(ms, 2.0 ** (bits - 6))
                ms = ms * ms
            weights.append(1.0 / math.sqrt(ms))
            if w * h <= 640 * 480:  # ffmpeg's in-line minimum smoothing (k_xpsnr_finish)
                wt = weights
                prev = (wt[i - 2] if i > 1 else 0.0) if x0 == 0 else (max(wt[i - 2], wt[i]) if x0 > b else wt[i])
                if i > wblk:
                    prev = max(prev, wt[i - 1 - wblk])
                if i > 0 and wt[i - 1] > prev:
                    wt[i - 1] = prev
                if x0 + b >= w and y0 + b >= h and i > wblk:
                    prev = max(wt[i - 1], wt[i - wblk])
                    if wt[i] > prev:
                        wt[i] = prev
            i += 1
    aa = avg_act(w, h, bits)

    def rnd(t):
        return 0 if t <= 0 else int(t * aa + 0.5)

    out = [0.0, 0.0, 0.0]
    for k in range(len(sses)):
        out[0] += float(sses[k]) * weights[k]
    res = [rnd(out[0])]
    for c in (1, 2):
        R, D = np.asarray(ref[c], np.int64), np.asarray(dis[c], np.int64)
        hc, wc = R.shape
        bx, by = b * wc // w, b * hc // h
        assert -(-wc // bx) == wblk and -(-hc // by) == -(-h // b), "4:2:0: the chroma grid is the luma grid"
        t, k = 0.0, 0
        for cy in range(0, hc, by):
            for cx in range(0, wc, bx):
                e = R[cy:cy + by, cx:cx + bx] - D[cy:cy + by, cx:cx + bx]
                t += float(int((e * e).sum())) * weights[k]
                k += 1
        res.append(rnd(t))
    return tuple(res)


def from_wsse(wsse, pw, ph, bits):
    if wsse == 0:
        return math.inf
    s = math.sqrt(float(wsse))
    return 10.0 * math.log10(float(pw * ph * (2 ** bits - 1) ** 2) / (s * s))


def sequence(sum_sqrt, sum_xpsnr, n, pw, ph, bits):
    if sum_sqrt >= n:
        m = sum_sqrt / n
        return 10.0 * math.log10(float(pw * ph * (2 ** bits - 1) ** 2) / (m * m))
    return sum_xpsnr / n


class Sequence:
    """the restatement over a sequence: feed pictures in order, read per-frame (wsse, xpsnr) and the sequence scores"""

    def __init__(self, w, h, bits, fps=(25, 1)):
        self.w, self.h, self.bits = w, h, bits
        self.second = second_order(*fps)
        self.reset()

    def reset(self):
        self.m1 = np.zeros((self.h, self.w), np.int64)
        self.m2 = np.zeros((self.h, self.w), np.int64)
        self.frames = []

    def push(self, ref, dis):
        wsse = frame_wsse(ref, dis, self.m1, self.m2, self.bits, self.second)
        self.m2, self.m1 = self.m1, np.asarray(ref[0], np.int64)
        cw, ch = (self.w + 1) // 2, (self.h + 1) // 2
        sc = tuple(from_wsse(wsse[c], self.w if c == 0 else cw, self.h if c == 0 else ch, self.bits) for c in range(3))
        self.frames.append((wsse, sc))
        return wsse, sc

    def sequence_scores(self):
        cw, ch = (self.w + 1) // 2, (self.h + 1) // 2
        out = []
        for c in range(3):
            s = sum(math.sqrt(float(f[0][c])) for f in self.frames)
            x = sum(f[1][c] for f in self.frames)
            out.append(sequence(s, x, len(self.frames), self.w if c == 0 else cw, self.h if c == 0 else ch, self.bits))
        return out
