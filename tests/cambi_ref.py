"""TEST INFRASTRUCTURE ONLY: CAMBI as DESIGN.md section 13 states it, in plain numpy, written from that text and from nothing else.
Slow and literal: the window counts are counted (counts_direct), the division is np.float32's, the sums are math.fsum.

    r = compute(Y, bits, window=7)   -> Result: .mask[s] .plane[s] .cmap[s] .t .n_gt .k .sum_gt .scores .cambi
"""
import math
from types import SimpleNamespace

import numpy as np

SCALES = 5
WEIGHTS = (16, 8, 4, 2, 1)


def window_of(w, requested=0):
    return requested if requested else max(63 * w // 3840, 3)


def mask_index(w, h):
    return (49 + 3 * (math.ceil(math.log2(min(w, h))) - 11) - 1) >> 1


def luminance(x):
    Lw, Lb = 300.0, 0.01
    rw, rb = Lw ** (1 / 2.4), Lb ** (1 / 2.4)
    a, b = (rw - rb) ** 2.4, rb / (rw - rb)
    v = min(max((x - 64) / 876, 0.0), 1.0)
    return a * max(v + b, 0.0) ** 2.4


def tvi(threshold=0.019):
    out = []
    for d in (1, 2, 3, 4):
        ok = [x for x in range(64, 940) if luminance(x + d) - luminance(x) > threshold * luminance(x)]
        out.append(max(ok) if ok else 0)
    return tuple(out)


def to10(Y, bits):
    """step 1: the 10-bit plane, anti-dither filtered below 10 bits"""
    Y = np.asarray(Y, np.int64)
    if bits >= 10:
        return Y >> (bits - 10)
    S = Y << (10 - bits)
    P = S.copy()
    P[:-1, :-1] = (S[:-1, :-1] + S[:-1, 1:] + S[1:, :-1] + S[1:, 1:]) >> 2
    P[:-1, -1] = (S[:-1, -1] + S[1:, -1]) >> 1
    P[-1, :-1] = (S[-1, :-1] + S[-1, 1:]) >> 1
    return P


def mask0(P):
    """step 2"""
    h, w = P.shape
    Z = np.ones((h, w), np.int64)
    Z[:, :-1] &= P[:, :-1] == P[:, 1:]
    Z[:-1, :] &= P[:-1, :] == P[1:, :]
    Zp = np.pad(Z, 3).astype(np.int32)
    rows = sum(Zp[:, b:b + w] for b in range(7))  # the 7 x 7 sum, rows first
    B = sum(rows[a:a + h, :] for a in range(7))
    return B > mask_index(w, h)


def mode3x3(P):
    """the most frequent of the nine neighbours, ties to the smallest value; the outermost rows and columns unchanged"""
    h, w = P.shape
    out = P.copy()
    for i in range(1, h - 1):
        for j in range(1, w - 1):
            vals, cnt = np.unique(P[i - 1:i + 2, j - 1:j + 2], return_counts=True)  # ascending: argmax takes the smallest of a tie
            out[i, j] = vals[np.argmax(cnt)]
    return out


def mode3x3_planes(P):
    """the same filter, whole planes at a time (for the large pictures of the GPU tier); test_cambi_cpu holds it to mode3x3"""
    h, w = P.shape
    out = P.copy()
    if h < 3 or w < 3:
        return out
    Q = P.astype(np.int16)  # 10-bit codes
    nb = [Q[a:a + h - 2, b:b + w - 2] for a in range(3) for b in range(3)]
    cnt = [sum((x == y).astype(np.int8) for y in nb) for x in nb]
    best = np.maximum.reduce(cnt)
    cand = np.minimum.reduce([np.where(c == best, x, np.int16(1 << 14)) for x, c in zip(nb, cnt)])
    out[1:-1, 1:-1] = cand
    return out


def counts_direct(P, M, pad):
    """n[k][i][j] = masked pixels of value P[i][j] + k - 4 in the window of (i, j), clipped to the picture: one shifted comparison per
    window position and k"""
    h, w = P.shape
    V = np.where(M, P, -(1 << 20))
    n = np.zeros((9, h, w), np.int64)
    for dr in range(-pad, pad + 1):
        for dc in range(-pad, pad + 1):
            r0, r1, c0, c1 = max(0, -dr), min(h, h - dr), max(0, -dc), min(w, w - dc)
            if r0 >= r1 or c0 >= c1:
                continue
            diff = V[r0 + dr:r1 + dr, c0 + dc:c1 + dc] - P[r0:r1, c0:c1]
            for k in range(9):
                n[k, r0:r1, c0:c1] += diff == k - 4
    return n


def counts_by_value(P, M, pad):
    """the same counts from one summed-area table per code value in use (for the large pictures of the GPU tier); test_cambi_cpu
    holds it to counts_direct"""
    h, w = P.shape
    n = np.zeros((9, h, w), np.int64)
    ii, jj = np.indices((h, w))
    r0, r1 = np.maximum(ii - pad, 0), np.minimum(ii + pad + 1, h)
    c0, c1 = np.maximum(jj - pad, 0), np.minimum(jj + pad + 1, w)
    for u in np.unique(P[M]):
        T = np.zeros((h + 1, w + 1), np.int64)
        T[1:, 1:] = np.cumsum(np.cumsum(M & (P == u), axis=0), axis=1)
        box = T[r1, c1] - T[r0, c1] - T[r1, c0] + T[r0, c0]
        for k in range(9):
            sel = P == u - (k - 4)  # pixels of value v with v + k - 4 == u
            n[k][sel] = box[sel]
    return n


def cvalues(P, M, pad, tv, counts=counts_direct):
    """step 5: float32 plane"""
    n = counts(P, M, pad)
    p0 = n[4]
    C = np.zeros(P.shape, np.float32)
    for d in (1, 2, 3, 4):
        m = np.maximum(n[4 + d], n[4 - d])
        N = (d * p0 * m).astype(np.uint32).astype(np.float32)
        Q = np.maximum(p0 + m, 1).astype(np.uint32).astype(np.float32)
        cd = np.where(M & (P <= tv[d - 1]), N / Q, np.float32(0)).astype(np.float32)
        C = np.maximum(C, cd)
    return C


def pool(C, topk):
    """step 6: (t bits, n_gt, k, sum_gt)"""
    v = np.sort(C.ravel())[::-1]
    k = min(max(int(math.floor(topk * v.size)), 1), v.size)
    t = v[k - 1]
    gt = v[v > t]
    return int(np.float32(t).view(np.uint32)), int(gt.size), k, math.fsum(float(x) for x in gt)


def scores(t, n_gt, k, sum_gt, window):
    area = (2 * (window >> 1) + 1) ** 2
    sc = [(sum_gt[s] + (k[s] - n_gt[s]) * float(np.uint32(t[s]).view(np.float32))) / k[s] for s in range(SCALES)]
    return sc, min(sum(WEIGHTS[s] * sc[s] for s in range(SCALES)) / area, 1000.0)


def compute(Y, bits, window=0, topk=0.6, tvi_threshold=0.019, fast=False, scales=range(SCALES)):
    """fast: whole-plane mode filter and summed-area counts; scales: the scales whose c-values are wanted (the others' cmap, t ...
    are None)"""
    Y = np.asarray(Y, np.int64)
    h, w = Y.shape
    win = window_of(w, window)
    pad = win >> 1
    tv = tvi(tvi_threshold)
    P = to10(Y, bits)
    M = mask0(P)
    r = SimpleNamespace(window=win, mask=[], plane=[], cmap=[], t=[], n_gt=[], k=[], sum_gt=[])
    for s in range(SCALES):
        if s:
            P, M = P[::2, ::2], M[::2, ::2]
        P = (mode3x3_planes if fast else mode3x3)(P)
        r.mask.append(M)
        r.plane.append(P)
        if s in scales:
            C = cvalues(P, M, pad, tv, counts_by_value if fast else counts_direct)
            t, n_gt, k, sm = pool(C, topk)
        else:
            C = t = n_gt = k = sm = None
        r.cmap.append(C); r.t.append(t); r.n_gt.append(n_gt); r.k.append(k); r.sum_gt.append(sm)
    if all(c is not None for c in r.cmap):
        r.scores, r.cambi = scores(r.t, r.n_gt, r.k, r.sum_gt, win)
    return r
