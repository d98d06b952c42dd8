"""TEST INFRASTRUCTURE ONLY: the definition of DESIGN.md section 12 in numpy, written from its text -- the 256-bin luma histogram, the
bin merge, the distance, the score, the verdict and the stats.  Takes sample VALUES (int arrays), never a layout's bytes."""
import numpy as np

BINS = (8, 16, 32, 64, 128, 256)


def supported(w, h, layout, bits):
    if w == 0 or h == 0 or w * h > 1 << 31 or not 8 <= bits <= 16:
        return False
    return {"y8": bits == 8, "y16_msb": bits >= 9, "y16_low": bits >= 9, "y10_packed": bits == 10}.get(layout, False)


def hist(Y, bits):
    """hist[b] = the number of samples with sample >> (D - 8) == b"""
    Y = np.asarray(Y, np.int64)
    assert Y.min() >= 0 and Y.max() < 1 << bits
    return np.bincount((Y >> (bits - 8)).ravel(), minlength=256).astype(np.uint32)


def merge(h, bins):
    if bins not in BINS:
        raise ValueError(bins)
    return np.asarray(h, np.uint64).astype(object).reshape(bins, 256 // bins).sum(axis=1)  # python integers: no width to overflow


def distance(a, b, bins=64):
    return int(sum(abs(int(x) - int(y)) for x, y in zip(merge(a, bins), merge(b, bins))))


def score(dist, w, h):
    return float(dist) / (2.0 * float(w) * float(h))


def is_cut(s, threshold=0.5):
    return s >= threshold


def cuts(hists, w, h, bins=64, threshold=0.5):
    scores = [0.0] + [score(distance(hists[i - 1], hists[i], bins), w, h) for i in range(1, len(hists))]
    return scores, [i > 0 and is_cut(s, threshold) for i, s in enumerate(scores)]


def stats(h):
    h = [int(v) for v in h]
    used = [b for b, v in enumerate(h) if v]
    return used[0], used[-1], sum(b * v for b, v in enumerate(h)) / sum(h)
