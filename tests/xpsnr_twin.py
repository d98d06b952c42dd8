"""TEST INFRASTRUCTURE ONLY: a second, vectorised restatement of XPSNR, written from the text of DESIGN.md section 8 and not from
tests/xpsnr_ref.py or the kernels.  The high-pass runs over the whole zero-padded luma plane with numpy slicing; the integer block sums
come from reshaping zero-padded planes into (block rows, b, block columns, b); only the weights, their smoothing and the three weighted
sums are sequential float64 loops in raster order, the order the definition fixes, so that the results are bit-equal with the
restatement.  Fast enough to stand as the reference of 8K pictures and batches of 130.

Pictures are (Y, Cb, Cr) integer arrays of the D-bit sample values."""
import math

import numpy as np


def block_size(w, h):
    return 4 * int(32 * math.sqrt(w * h / (3840 * 2160)) + 0.5)


def _block_sums(a, by, bx):
    """a (rows, cols) -> (ceil(rows / by), ceil(cols / bx)) int64 sums of its by x bx tiles (zero padded past the edges)"""
    r, c = a.shape
    nr, nc = -(-r // by), -(-c // bx)
    z = np.zeros((nr * by, nc * bx), np.int64)
    z[:r, :c] = a
    return z.reshape(nr, by, nc, bx).sum(axis=(1, 3))


def highpass(Y, bval):
    """|f| at every position the definition evaluates: every sample (bval 1), or the even (x, y) of every 2x2 cell (bval 2); the taps
    read a plane padded by 3 zero samples, and the caller keeps only the positions whose taps stay inside the picture"""
    h, w = Y.shape
    P = np.zeros((h + 6, w + 6), np.int64)
    P[3:-3, 3:-3] = Y
    s = 2 if bval == 2 else 1

    def o(dx, dy):
        return P[3 + dy:3 + dy + h:s, 3 + dx:3 + dx + w:s]
    if bval == 1:
        # 12 o - 2 (four direct neighbours) - (four diagonal neighbours)
        f = 12 * o(0, 0) - 2 * (o(-1, 0) + o(1, 0) + o(0, -1) + o(0, 1)) - (o(-1, -1) + o(1, -1) + o(-1, 1) + o(1, 1))
    else:
        # highds at the cell whose top-left sample is (x, y): 12 x the cell, -3 x the four samples beside its left and right columns
        # and above / below its rows, -2 x its four diagonal corners, -1 x the sixteen samples two away along each side
        cell = o(0, 0) + o(1, 0) + o(0, 1) + o(1, 1)
        side = o(-1, 0) + o(-1, 1) + o(2, 0) + o(2, 1) + o(0, -1) + o(1, -1) + o(0, 2) + o(1, 2)
        corner = o(-1, -1) + o(2, -1) + o(-1, 2) + o(2, 2)
        outer = sum(o(dx, -2) + o(dx, 3) for dx in (-1, 0, 1, 2)) + sum(o(-2, dy) + o(3, dy) for dy in (-1, 0, 1, 2))
        f = 12 * cell - 3 * side - 2 * corner - outer
    return np.abs(f)


def smooth_weights(w, wblk):
    """ffmpeg's in-line minimum smoothing (pictures of at most 640 x 480 samples), in the raster pass that computes the weights:
    once weight i exists, weight i-1 is lowered to the largest of weight i (unless i starts a row), weight i-2 (unless i is a row's
    second block; 0 for i <= 1) and the weight above-left of i; the picture's last block is then lowered to the larger of its left
    and upper neighbours"""
    w = list(w)
    n = len(w)
    for i in range(n):
        x = i % wblk
        if x == 0:
            prev = w[i - 2] if i > 1 else 0.0
        elif x == 1:
            prev = w[i]
        else:
            prev = max(w[i - 2], w[i])
        if i > wblk:
            prev = max(prev, w[i - 1 - wblk])
        if i > 0 and w[i - 1] > prev:
            w[i - 1] = prev
        if i == n - 1 and i > wblk:
            prev = max(w[i - 1], w[i - wblk])
            if w[i] > prev:
                w[i] = prev
    return w


class Sequence:
    """feed pictures in order; push -> ((wsse Y, Cb, Cr), (XPSNR Y, Cb, Cr)); sequence_scores() at any point"""

    def __init__(self, w, h, bits, fps=(25, 1)):
        self.w, self.h, self.bits = w, h, bits
        self.second = fps[0] // fps[1] >= 32
        self.b = block_size(w, h)
        self.bval = 2 if w * h > 2048 * 1152 else 1
        r = w * h / (3840 * 2160)
        self.avg_act = math.sqrt(16 * 2.0 ** (2 * bits - 9) / math.sqrt(max(1e-5, r)))
        self.m1 = self.m2 = np.zeros((h, w), np.int64)
        self.frames = []

    def wsse(self, ref, dis):
        Y, D = (np.asarray(p, np.int64) for p in (ref[0], dis[0]))
        h, w, b, bval = self.h, self.w, self.b, self.bval
        if b < 4:
            return tuple(int(((np.asarray(r, np.int64) - np.asarray(d, np.int64)) ** 2).sum()) for r, d in zip(ref, dis))
        wblk, hblk = -(-w // b), -(-h // b)
        sse = _block_sums((Y - D) ** 2, b, b)
        # spatial activity: the window drops the picture's outer bval rows and columns, which keeps every tap inside the picture
        f = highpass(Y, bval)
        keep = np.zeros_like(f, dtype=bool)
        s = bval
        keep[-(-bval // s):(h - bval + s - 1) // s, -(-bval // s):(w - bval + s - 1) // s] = True
        sa = _block_sums(np.where(keep, f, 0), b // s, b // s)
        # temporal activity, gamma = 2: on samples (bval 1) or on the sums of the 2x2 cells (bval 2)
        t = Y - 2 * self.m1 + self.m2 if self.second else Y - self.m1
        if bval == 2:
            t = t[0::2, 0::2] + t[0::2, 1::2] + t[1::2, 0::2] + t[1::2, 1::2]
        ta = 2 * _block_sums(np.abs(t), b // s, b // s)
        # the blocks' sizes and windows
        bw = np.minimum(b, w - b * np.arange(wblk))
        bh = np.minimum(b, h - b * np.arange(hblk))
        ww = bw - bval * ((np.arange(wblk) == 0).astype(int) + (np.arange(wblk) == wblk - 1).astype(int))
        wh = bh - bval * ((np.arange(hblk) == 0).astype(int) + (np.arange(hblk) == hblk - 1).astype(int))
        weights = []
        floor = 2.0 ** (self.bits - 6)
        for by in range(hblk):
            for bx in range(wblk):
                if ww[bx] <= 0 or wh[by] <= 0:
                    weights.append(1.0)
                    continue
                ms = int(sa[by, bx]) / (int(ww[bx]) * int(wh[by])) + int(ta[by, bx]) / (int(bw[bx]) * int(bh[by]))
                ms = max(ms, floor)
                weights.append(1.0 / math.sqrt(ms * ms))
        if w * h <= 640 * 480:
            weights = smooth_weights(weights, wblk)
        out = []
        for c in range(3):
            if c == 0:
                e = sse.reshape(-1)
            else:
                R, Dc = (np.asarray(p[c], np.int64) for p in (ref, dis))
                hc, wc = R.shape
                e = _block_sums((R - Dc) ** 2, b * hc // h, b * wc // w)
                assert e.shape == (hblk, wblk), "4:2:0: the chroma grid is the luma grid"
                e = e.reshape(-1)
            acc = 0.0
            for k in range(len(weights)):
                acc += float(int(e[k])) * weights[k]
            out.append(0 if acc <= 0 else int(acc * self.avg_act + 0.5))
        return tuple(out)

    def push(self, ref, dis):
        ws = self.wsse(ref, dis)
        self.m2, self.m1 = self.m1, np.asarray(ref[0], np.int64)
        sizes = [(self.w, self.h)] + 2 * [((self.w + 1) // 2, (self.h + 1) // 2)]
        peak = 2 ** self.bits - 1
        sc = tuple(math.inf if v == 0 else 10.0 * math.log10(float(pw * ph * peak * peak) / (math.sqrt(float(v)) ** 2))
                   for v, (pw, ph) in zip(ws, sizes))
        self.frames.append((ws, sc))
        return ws, sc

    def sequence_scores(self):
        sizes = [(self.w, self.h)] + 2 * [((self.w + 1) // 2, (self.h + 1) // 2)]
        n, out = len(self.frames), []
        for c, (pw, ph) in enumerate(sizes):
            S = sum(math.sqrt(float(f[0][c])) for f in self.frames)
            if S >= n:
                out.append(10.0 * math.log10(float(pw * ph * (2 ** self.bits - 1) ** 2) / ((S / n) * (S / n))))
            else:
                out.append(sum(f[1][c] for f in self.frames) / n)
        return out
