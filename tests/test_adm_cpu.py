"""No-GPU tier of VMAF's ADM (include/turbo_metrics_adm.h, libturbometrics_adm.so): the weights and the wavelet pair, the properties
and hand-derived answers of DESIGN.md section 11 as literals against the numpy restatement (tests/adm_ref.py) and against the kernel
SOURCE executed lane by lane on the CPU (tests/adm_emul); emulated kernel == restatement, the a bands and the restored, additive and
threshold planes of all four scales bit-exact and the 24 sums within the derived bound, on all four layouts, with dirty bytes;
create-time refusals; the ABI (C99 header, exports); tm_adm_scores; the binding's checks; the CLI's option parsing."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import adm_ref as R
from tests import adm_util as U
from tests import vif_ref
from tm_pkg import tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIB = os.path.join(ROOT, "turbo-metrics_amd", "libturbometrics_adm.so")
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
SEEN = {"rel": 0.0}  # the largest relative difference between the emulated kernel's sums and the restatement's (printed at the end)
f32 = np.float32


def rtol(n):
    """Derived, not measured.  Every f32 plane is bit-exact and the cube of a term is the same two double multiplications on both
    sides, so the kernel and the restatement add the SAME n non-negative doubles, in different orders (per lane, wave tree, cells in
    a fixed order; numpy's pairwise sum).  A sum of n non-negative terms in any order is within (1 + u)^(n - 1) - 1 of the exact one,
    u = 2^-53; two orders differ by at most twice that: 2 n u to first order, and the second-order term n^2 u^2 is below n u / 2
    for n < 2^52.  So 2.5 n u, n the number of pixels the sum runs over (2^19 at 1080p, scale 0: 1.5e-10)."""
    return 2.5 * n * 2.0 ** -53


def declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(2) for m in re.finditer(r" ([A-Za-z]) (\S+)", out) if m.group(1) in "TDBRW" and not m.group(2).startswith(("_init", "_fini", "__bss", "_edata", "_end")))


def emul(w, h, layout, bits, ref, dis, pad=0, dirty=None):
    return U.emulate(w, h, layout, bits, U.luma_plane(layout, ref, bits, pad=pad, dirty=dirty),
                     U.luma_plane(layout, dis, bits, pad=pad, dirty=None if dirty is None else dirty + 1))


def same(a, b):
    """bit-exact as values: equal everywhere, no NaN (the sign of a zero is not a value)"""
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and not np.isnan(a).any() and np.array_equal(a, b)


def check_against_restatement(got, want, what):
    for s in range(4):
        planes = [("a_ref", got[s]["a"][0], want[s]["a"][0]), ("a_dis", got[s]["a"][1], want[s]["a"][1]), ("thr", got[s]["thr"], want[s]["thr"])]
        planes += [(f"r_{b}", got[s]["r"][i], want[s]["r"][i]) for i, b in enumerate(R.BANDS)]
        planes += [(f"a_{b}", got[s]["add"][i], want[s]["add"][i]) for i, b in enumerate(R.BANDS)]
        for name, a, b in planes:
            assert same(a, b), (what, s, name, float(np.nanmax(np.abs(a - b))), np.argwhere(a != b)[:4].tolist())
        for k in ("num", "den"):
            for b in range(3):
                g, w = got[s][k][b], want[s][k][b]
                rel = abs(g - w) / max(abs(w), 1e-300) if g != w else 0.0
                SEEN["rel"] = max(SEEN["rel"], rel)
                print(f"{what} scale {s} {k}[{R.BANDS[b]}]: kernel {g!r} restatement {w!r} rel {rel:.3e} bound {rtol(want[s]['area']):.3e}")
                assert rel <= rtol(want[s]["area"]), (what, s, k, b, g, w)


def sums_of(res):
    return [p["num"] for p in res], [p["den"] for p in res]


# ---- constants and geometry ----------------------------------------------------------------------------------------------------
def test_weights_are_the_eight_values():
    hv = (0.0173815, 0.0319848, 0.0433727, 0.0456734)
    d = (0.00589069, 0.0142991, 0.0243969, 0.0313127)
    g = U.geom(64, 64)
    for tab in ([R.weights(s) for s in range(4)], g["rf"]):
        for s in range(4):
            assert all(isinstance(v, np.float32) for v in tab[s])
            assert float(f"{float(tab[s][0]):.6g}") == hv[s] and tab[s][1] == tab[s][0], (s, tab[s])
            assert float(f"{float(tab[s][2]):.6g}") == d[s], (s, tab[s])
    assert [tuple(x) for x in g["rf"]] == [R.weights(s) for s in range(4)]
    assert g["cos2"] == R.COS2 == f32(math.cos(math.pi / 180) ** 2) and 0.99969 < float(R.COS2) < 0.9997


def test_filter_pair_and_its_mirror():
    lo, hi = U.filters()
    assert lo == R.LO and hi == R.HI
    assert hi == (lo[3], -lo[2], lo[1], -lo[0])                     # the quadrature mirror of db2
    assert abs(sum(float(v) for v in lo) - math.sqrt(2.0)) < 1e-6 and abs(sum(float(v) for v in hi)) < 1e-6
    L = U.emul_lib()
    for n in (4, 5, 32, 135):
        # below 0 the edge sample is not repeated, at and beyond n it is
        assert [R.mirror(p, n) for p in (-1, 0, n - 1, n, n + 1)] == [1, 0, n - 1, n - 1, n - 2]
        assert all(L.ae_mirror(p, n) == R.mirror(p, n) for p in range(-1, n + 2))
    assert vif_ref.mirror(32, 32) == 30 and R.mirror(32, 32) == 31 and vif_ref.mirror(-1, 32) == R.mirror(-1, 32) == 1  # not VIF's on the high side


@pytest.mark.parametrize("w,h,want", [(32, 32, [(16, 16), (8, 8), (4, 4), (2, 2)]), (33, 47, [(17, 24), (9, 12), (5, 6), (3, 3)]),
                                      (1920, 1080, [(960, 540), (480, 270), (240, 135), (120, 68)]), (101, 75, [(51, 38), (26, 19), (13, 10), (7, 5)])])
def test_scale_sizes(w, h, want):
    assert [(bw, bh) for _, _, bw, bh in R.sizes(w, h)] == want
    assert U.geom(w, h)["sizes"] == R.sizes(w, h)
    assert R.sizes(w, h)[1][:2] == want[0]  # the pictures of scale s + 1 are the a bands of scale s


def test_border_is_truncated_by_hand():
    """left = (int)(bw 0.1 - 0.5) in double, C truncation:
      bw = 14: 1.4000000000000001 - 0.5 = 0.9000000000000001 -> 0 (rounding would give 1)      bw = 15: 1.5 - 0.5 = 1.0 -> 1
      bw = 16: 1.6 - 0.5 = 1.1 -> 1      bw = 24: 1.9000000000000004 -> 1      bw = 25: 2.0 -> 2      bw = 26: 2.1 -> 2
      bw = 4:  0.4 - 0.5 = -0.09999999999999998 -> 0 (towards zero; a floor would give -1)      bw = 5: 0.0 -> 0
      1080p: bw = 960, 480, 240, 120 -> 95.5, 47.5, 23.5, 11.5 -> 95, 47, 23, 11; bh = 540, 270, 135, 68 -> 53.5, 26.5, 13.0, 6.3 -> 53, 26, 13, 6"""
    want = {14: 0, 15: 1, 16: 1, 24: 1, 25: 2, 26: 2, 4: 0, 5: 0, 2: 0, 960: 95, 480: 47, 240: 23, 120: 11, 540: 53, 270: 26, 135: 13, 68: 6}
    for n, left in want.items():
        assert R.border(n, n) == (left, left, n - left, n - left), n
    # the kernel's geometry at sizes whose bands are 14 / 15 / 16 / 24 / 25 / 4 wide or high
    for w, h in ((32, 50), (28 + 4, 30 + 2), (48, 50), (1920, 1080), (33, 47), (64, 32)):
        g = U.geom(w, h)
        assert g["border"] == [R.border(bw, bh) for _, _, bw, bh in R.sizes(w, h)], (w, h)
    assert U.geom(1920, 1080)["border"] == [(95, 53, 865, 487), (47, 26, 433, 244), (23, 13, 217, 122), (11, 6, 109, 62)]
    assert U.geom(28, 32) is None
    g = U.geom(32, 50)  # bands 16 x 25, 8 x 13, 4 x 7, 2 x 4
    assert g["border"] == [(1, 2, 15, 23), (0, 0, 8, 13), (0, 0, 4, 7), (0, 0, 2, 4)]


# ---- properties that follow from the text, exactly ------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,bits", U.CASES)
def test_identical_and_flat_pictures_are_exactly_one(layout, bits):
    """dis = ref: t = o, k = o / (o + 1e-30f) = 1 for every |o| above 2e-23 (and r = 0 = o where o = 0), the angle test passes and
    min(100 o, o) = o, so r = o, a = 0, thr = 0 and every term of N is the same f32 as the term of Dn."""
    w, h = 53, 37  # odd, and not a multiple of the tile
    M = (1 << bits) - 1
    pics = [U.pair(w, h, bits, "noise", seed=2)[0], U.pair(w, h, bits, "blurred", seed=2)[0]] + [np.full((h, w), v, np.int64) for v in (1, M // 3, M)]
    for ref in pics:
        want = R.adm(ref, ref, bits)
        got = emul(w, h, layout, bits, ref, ref, pad=3, dirty=7)
        for res in (want, got):
            for s in range(4):
                assert res[s]["num"] == res[s]["den"], (s, res[s]["num"], res[s]["den"])
                assert all((p == 0).all() for p in res[s]["add"]) and (res[s]["thr"] == 0).all()
            assert R.scores(*sums_of(res), w, h) == [1.0] * 5
            assert tm.adm.scores(*sums_of(res), w, h) == [1.0] * 5
        check_against_restatement(got, want, f"identical {layout} {bits}")


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_mid_grey_distorted_gives_no_numerator(layout, bits):
    """dis flat at mid-grey: its scale-0 picture is 0.0f everywhere, every t_b = 0, k = 0, r = 0, a = 0, thr = 0, x = 0: N = 0 at every
    scale and adm_scale_s = 3 cbrt(area_s / 32) / den_s."""
    w, h = 61, 34
    ref = U.pair(w, h, bits, "blurred", seed=4)[0]
    dis = np.full((h, w), 1 << (bits - 1), np.int64)
    want, got = R.adm(ref, dis, bits), emul(w, h, layout, bits, ref, dis, pad=2, dirty=3)
    check_against_restatement(got, want, f"mid-grey {layout} {bits}")
    for res in (want, got):
        sc = tm.adm.scores(*sums_of(res), w, h)
        tn = td = 0.0
        for s in range(4):
            assert res[s]["num"] == [0.0, 0.0, 0.0] and min(res[s]["den"]) > 0.0
            c = float(np.cbrt(want[s]["area"] / 32.0))
            den = 0.0
            for b in range(3):
                den += float(np.cbrt(res[s]["den"][b])) + c
            assert abs(sc[s] - ((c + c) + c) / den) <= 5e-15  # cbrt: see test_scores_match_the_formula
            tn, td = tn + ((c + c) + c), td + den
        assert abs(sc[4] - tn / td) <= 5e-15 and 0.0 < sc[4] < 1.0


@pytest.mark.parametrize("layout,bits", [("y8", 8), ("y16_msb", 10), ("y16_low", 16), ("y10_packed", 10)])
def test_half_contrast_is_one_eighth(layout, bits):
    """ref - 128 even (on the 8-bit scale) and dis - 128 = (ref - 128) / 2.  Halving is exact in f32 and commutes with every rounding
    (no value here is near the subnormal range), so every plane of dis is exactly half that of ref at every scale: t_b = o_b / 2,
    k = 0.5 exactly (or 0 where o_b = 0), r_b = t_b; dp = om / 2 >= 0 and dp^2 = om^2 / 4 >= C om^2 / 4 (C < 1 by 3e-4, far more
    than the roundings), so the gain limit gives min(100 t_b, t_b) = t_b; a_b = 0 and thr = 0.  Each term of N is then exactly the
    term of Dn divided by 8, and so is every partial sum taken in the same order: the bound on |N - Dn / 8| derived from the text is
    0 for a given order of adding (both implementations add N and Dn in one order each)."""
    w, h = 75, 45
    rng = np.random.default_rng(11)
    half = rng.integers(-60, 61, (h, w))
    unit = 1 << (bits - 8)
    ref, dis = (128 + 2 * half) * unit, (128 + half) * unit
    want, got = R.adm(ref, dis, bits), emul(w, h, layout, bits, ref, dis, pad=1, dirty=5)
    check_against_restatement(got, want, f"half contrast {layout} {bits}")
    for res in (want, got):
        for s in range(4):
            assert all((p == 0).all() for p in res[s]["add"]) and (res[s]["thr"] == 0).all()
            assert [8.0 * n for n in res[s]["num"]] == res[s]["den"] and min(res[s]["den"]) > 0.0, (s, res[s]["num"], res[s]["den"])
    for s in range(4):
        for r, o in zip(want[s]["r"], want[s]["o"]):
            assert np.array_equal(r, o / f32(2))


# ---- by hand ---------------------------------------------------------------------------------------------------------------------
# With dis = ref the restored planes r_h, r_v, r_d ARE the reference's bands (see above), so the emulated kernel's hook shows them.
# db2: lo = (1 + q, 3 + q, 3 - q, 1 - q) / (4 sqrt 2) with q = sqrt 3; hi = (lo3, -lo2, lo1, -lo0).  A single sample of value X at
# row y, column x of a field of 0.0f reaches band row i through tap k = y + 1 - 2 i and band column j through tap x + 1 - 2 j;
# band values are f32(f32(F_row[k] X) F_col[k']) with F = lo or hi: a = lo.lo, v = lo rows then hi columns, h = hi rows then lo
# columns, d = hi.hi.  X = 64 (sample 192 on a field of 128) keeps the first product exact.  The literals below are these products
# in exact arithmetic (12 = 64 lo1 lo2 = 64 * 6 / 32, -4 = 64 lo0 lo3 = 64 * -2 / 32, ...); three f32 roundings (two coefficients,
# one product; for the high mirror two sums more) are each below 2^-24 relative: 1e-6 covers them.
HAND_RTOL = 1e-6


def _bands_of_identical(w, h, ref):
    want = R.adm(ref, ref, 8)[0]
    got = emul(w, h, "y8", 8, ref, ref)[0]
    out = []
    for res in (want, got):
        hh, vv, dd = res["r"]
        out.append(dict(a=res["a"][0], v=vv, h=hh, d=dd))
    for b in "hvd":
        assert same(out[0][b], out[1][b]) and same(out[0][b], want["o"]["hvd".index(b)])
    assert same(out[0]["a"], out[1]["a"])
    return out


def _expect(bands, table, shape):
    for res in bands:
        for b in "avhd":
            nz = {(i, j) for i, j in np.argwhere(res[b] != 0).tolist()}
            assert res[b].shape == shape and nz == set(table), (b, sorted(nz))
            for (i, j), vals in table.items():
                want = vals["avhd".index(b)]
                assert abs(float(res[b][i, j]) - want) <= HAND_RTOL * abs(want), (b, i, j, float(res[b][i, j]), want)


def test_single_bright_sample_in_the_interior_by_hand():
    """sample (row 21, column 18) of a 48 x 48 picture.  Row 21 is tap k = 22 - 2 i: i = 10 (k = 2), i = 11 (k = 0); column 18 is tap
    19 - 2 j: j = 8 (k = 3), j = 9 (k = 1).  E.g. a[10][9] = 64 lo2 lo1 = 12, a[11][8] = 64 lo0 lo3 = -4, d[10][9] = 64 hi2 hi1 =
    -64 lo1 lo2 = -12, h[10][9] = 64 hi2 lo1 = 64 lo1^2 = 64 (12 + 6 q) / 32 = 44.78460969."""
    w = h = 48
    ref = np.full((h, w), 128, np.int64)
    ref[21, 18] = 192
    table = {(10, 8): (-1.8564064605, -6.9282032303, -6.9282032303, -25.8564064605),
             (10, 9): (12.0, -3.2153903092, 44.7846096908, -12.0),
             (11, 8): (-4.0, -14.9282032303, 1.0717967697, 4.0),
             (11, 9): (25.8564064605, -6.9282032303, -6.9282032303, 1.8564064605)}
    _expect(_bands_of_identical(w, h, ref), table, (24, 24))


def test_top_left_corner_by_hand_needs_the_low_mirror_not_to_repeat():
    """sample (0, 0): position -1 reads sample 1, so sample 0 is read once, by band row 0 through tap 1 (2 * 0 - 1 + 1 = 0), and the
    same for columns: ONE non-zero pixel per band, a = 64 lo1^2 = 44.78460969, v = h = 64 lo1 hi1 = -64 lo1 lo2 = -12,
    d = 64 hi1^2 = 64 lo2^2 = 64 (12 - 6 q) / 32 = 3.21539031.  A mirror that repeats the edge would add tap 0: 64 (lo0 + lo1)^2 = 111.4."""
    w = h = 48
    ref = np.full((h, w), 128, np.int64)
    ref[0, 0] = 192
    _expect(_bands_of_identical(w, h, ref), {(0, 0): (44.7846096908, -12.0, -12.0, 3.2153903092)}, (24, 24))


def test_last_row_and_column_of_an_odd_picture_by_hand_needs_the_high_mirror_to_repeat():
    """47 x 45, sample (44, 46).  Rows, n = 45, bh = 23: band row 22 reads positions 43, 44, 45 -> 44, 46 -> 43, so row 44 comes
    through taps 1 AND 2 (lo1 + lo2 = 6 / (4 sqrt 2), hi1 + hi2 = lo1 - lo2 = 2 q / (4 sqrt 2)); band row 21 reads 41 .. 44: tap 3.
    Columns, n = 47, bw = 24: band column 23 reads 45, 46, 47 -> 46, 48 -> 45: taps 1 and 2; band column 22 reads 43 .. 46: tap 3.
    a[22][23] = 64 (lo1 + lo2)^2 = 64 * 36 / 32 = 72, d[22][23] = 64 (hi1 + hi2)^2 = 64 * 12 / 32 = 24, v = h = 64 * 6 * 2 q / 32 =
    41.56921938; a[21][22] = 64 lo3^2 = 64 (4 - 2 q) / 32 = 1.07179677, v[21][22] = h[21][22] = 64 lo3 hi3 = -64 lo3 lo0 = 4."""
    w, h = 47, 45
    ref = np.full((h, w), 128, np.int64)
    ref[44, 46] = 192
    table = {(21, 22): (1.0717967697, 4.0, 4.0, 14.9282032303),
             (21, 23): (-8.7846096908, -5.0717967697, -32.7846096908, -18.9282032303),
             (22, 22): (-8.7846096908, -32.7846096908, -5.0717967697, -18.9282032303),
             (22, 23): (72.0, 41.5692193816, 41.5692193816, 24.0)}
    _expect(_bands_of_identical(w, h, ref), table, (23, 24))


def test_decoupling_and_threshold_by_hand():
    """One band pixel, in numbers that f32 holds exactly.  o = (h 8, v 0, d -4), t = (2, 0, -8): k_h = 0.25, k_v = 0 / 1e-30 = 0,
    k_d = 2 -> 1; r = (2, 0, -4).  dp = 16, om = 64, tm = 4: 256 >= C 256, the angle test passes: r_h = min(200, 2) = 2, r_v stays,
    r_d = max(-400, -8) = -8; a = (0, 0, 0).  With t = (2, 1, -8): dp = 16, tm = 5, 256 < C 320: no limit, r = (2, 0, -4),
    a = (0, 1, -4).  Threshold of a lone c = 1 in band h at (1, 1) of a 3 x 3 plane: 1/15 at (1, 1), 1/30 around it."""
    o = dict(h=np.array([[8.0]], f32), v=np.array([[0.0]], f32), d=np.array([[-4.0]], f32))
    t = dict(h=np.array([[2.0]], f32), v=np.array([[0.0]], f32), d=np.array([[-8.0]], f32))
    r, a = R.decouple(o, t)
    assert [float(r[b][0, 0]) for b in "hvd"] == [2.0, 0.0, -8.0] and [float(a[b][0, 0]) for b in "hvd"] == [0.0, 0.0, 0.0]
    t["v"] = np.array([[1.0]], f32)
    r, a = R.decouple(o, t)
    assert [float(r[b][0, 0]) for b in "hvd"] == [2.0, 0.0, -4.0] and [float(a[b][0, 0]) for b in "hvd"] == [0.0, 1.0, -4.0]
    z = np.zeros((3, 3), f32)
    one = z.copy()
    one[1, 1] = 1.0
    thr = R.threshold(dict(h=one, v=z, d=z), (f32(1), f32(1), f32(1)))
    assert thr[1, 1] == f32(1.0 / 15.0) and (np.delete(thr.ravel(), 4) == f32(1.0 / 30.0)).all()
    corner = z.copy()
    corner[0, 0] = 1.0
    thr = R.threshold(dict(h=z, v=z, d=corner), (f32(1), f32(1), f32(2)))
    assert thr[0, 0] == f32(1.0 / 15.0) * f32(2) and thr[1, 1] == f32(1.0 / 30.0) * f32(2) and thr[2, 2] == 0 and thr[0, 2] == 0


# ---- emulated kernel vs restatement ------------------------------------------------------------------------------------------
SIZES = ((32, 32), (33, 47), (75, 35), (131, 70))  # the smallest; odd x odd; a band width that is not a multiple of the tile; 3 x 3 tiles


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("layout,bits", U.CASES)
def test_emulated_kernel_matches_the_restatement(layout, bits, w, h):
    kind = U.CONTENTS[(U.CASES.index((layout, bits)) + SIZES.index((w, h))) % len(U.CONTENTS)]
    ref, dis = U.pair(w, h, bits, kind)
    check_against_restatement(emul(w, h, layout, bits, ref, dis, pad=5, dirty=11), R.adm(ref, dis, bits), f"{layout} {bits} {w}x{h} {kind}")


@pytest.mark.parametrize("kind", U.CONTENTS)
@pytest.mark.parametrize("layout,bits", [("y8", 8), ("y16_msb", 16), ("y10_packed", 10)])
def test_every_content_on_several_tiles(layout, bits, kind):
    w, h = 141, 99
    ref, dis = U.pair(w, h, bits, kind, seed=3)
    want = R.adm(ref, dis, bits)
    check_against_restatement(emul(w, h, layout, bits, ref, dis), want, f"{layout} {bits} {kind}")
    sc = R.scores(*sums_of(want), w, h)
    assert all(0.0 < v < 1.5 for v in sc), sc
    if kind in ("blurred", "noisy", "negative"):
        assert all(v < 1.0 for v in sc), sc
    if kind == "enhanced":  # the gain limit is what lets an enhancement score above 1
        assert sc[4] > 1.0 and any((np.abs(r) > np.abs(o)).any() for r, o in zip(want[0]["r"], want[0]["o"])), sc
    if kind == "negative":  # every k clamps at 0
        assert all((r == 0).all() for r in want[0]["r"])


def test_1080p_once():
    w, h = 1920, 1080
    ref, dis = U.pair(w, h, 8, "noisy", seed=1)
    want = R.adm(ref, dis, 8)
    assert want[3]["thr"].shape == (68, 120) and want[3]["area"] == (62 - 6) * (109 - 11)  # 135 rows -> 68: the odd size at scale 3
    check_against_restatement(emul(w, h, "y8", 8, ref, dis), want, "1080p noisy")


def test_largest_difference_seen():
    """prints what DESIGN.md section 11 records (run after the comparisons above: pytest keeps file order)"""
    print(f"largest relative difference of the 24 sums, emulated kernel vs restatement: {SEEN['rel']:.3e}")
    assert SEEN["rel"] <= rtol(2 ** 19)


@pytest.mark.parametrize("layout,bits", [("y16_low", 10), ("y16_msb", 12), ("y8", 8), ("y10_packed", 10)])
def test_dirty_bytes_do_not_change_a_bit(layout, bits):
    """high bits above D in y16_low, low bits below D in y16_msb, and the padding beyond W of a pitched row"""
    w, h = 61, 34
    ref, dis = U.pair(w, h, bits, "noisy", seed=5)
    clean = emul(w, h, layout, bits, ref, dis)
    for pad, dirty in ((9, 1), (1, 99)):
        got = emul(w, h, layout, bits, ref, dis, pad=pad, dirty=dirty)
        for s in range(4):
            assert got[s]["num"] == clean[s]["num"] and got[s]["den"] == clean[s]["den"]
            assert all(same(a, b) for a, b in zip(got[s]["r"] + got[s]["add"] + got[s]["a"] + (got[s]["thr"],),
                                                  clean[s]["r"] + clean[s]["add"] + clean[s]["a"] + (clean[s]["thr"],)))
    if layout in ("y16_low", "y16_msb"):
        a, b = U.luma_plane(layout, ref, bits, dirty=1), U.luma_plane(layout, ref, bits)
        assert not np.array_equal(a, b)  # the dirty planes do differ in the bits the kernel must ignore


# ---- refusals, ABI, host function, binding, CLI -------------------------------------------------------------------------------
def test_refusals_match_the_restatement():
    z = np.zeros((64, 64), np.uint16)
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 12, 16, 17):
            for w, h in ((32, 32), (31, 32), (32, 31), (64, 40)):
                assert (U.geom(w, h, layout, bits) is not None) == R.supported(w, h, layout, bits), (layout, bits, w, h)
    assert U.emulate(31, 40, "y8", 8, z, z) is None


def test_create_refuses_before_touching_the_device():
    L = tm.adm.lib()
    h = C.c_void_p()
    for w, hh, lay, bits in ((31, 32, 0, 8), (32, 31, 0, 8), (64, 64, 0, 10), (64, 64, 1, 8), (64, 64, 1, 17), (64, 64, 3, 12), (64, 64, 4, 8), (64, 64, 2, 7)):
        assert L.tm_adm_create(C.byref(h), w, hh, lay, bits, 1) == tm.ffi.TM_ERR_UNSUPPORTED, (w, hh, lay, bits)
        assert h.value is None
    assert L.tm_adm_create(None, 64, 64, 0, 8, 1) == tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_adm_create(C.byref(h), 64, 64, 0, 8, 0) == tm.ffi.TM_ERR_INVALID_ARG
    assert h.value is None


def test_header_is_plain_c99_and_the_library_exports_exactly_it(tmp_path):
    want = declared("turbo_metrics_adm.h")
    assert len(want) == 8 and all(n.startswith("tm_adm") for n in want)
    assert exported(ALIB) == want
    assert sorted(tm.adm.SYMBOLS) == want
    src = tmp_path / "c.c"
    # 64 x 64: the bands of scale 0 are 32 x 32, left = top = (int)2.7 = 2, area = 28 * 28 = 784; 784 / 32 = 24.5
    src.write_text('#include "turbo_metrics_adm.h"\n#include <stdio.h>\n'
                   "int main(void) { tm_adm *v = NULL; tm_adm_frame f; double o[5]; int s, b; (void)v;\n"
                   "  for (s = 0; s < 4; ++s) for (b = 0; b < 3; ++b) { f.num_cube[s][b] = 0.0; f.den_cube[s][b] = s ? 0.0 : 8.0 * 24.5; }\n"
                   "  tm_adm_scores(&f, 64, 64, o); printf(\"%.6f %.1f %.1f %.1f\\n\", o[0], o[1], o[2], o[3]); return 0; }\n")
    exe = str(tmp_path / "c")
    lib_dir = os.path.dirname(ALIB)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                           "-L" + lib_dir, "-lturbometrics_adm", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    # scale 0: num = 3 c, den = 3 (2 c + c) with c = cbrt(24.5): 1 / 3; scales 1 .. 3: num == den: 1
    assert out.returncode == 0 and out.stdout.strip() == "0.333333 1.0 1.0 1.0", (out.returncode, out.stdout, out.stderr)


def test_the_other_libraries_are_unchanged_in_what_they_export():
    for lib in (tm.ffi.SHIP_LIB_PATH, tm.ffi.LIB_PATH, tm.xpsnr.LIB_PATH, tm.motion.LIB_PATH, tm.vif.LIB_PATH):
        assert not [n for n in exported(lib) if "adm" in n], lib
    assert not [n for n in tm.ffi.SYMBOLS if "adm" in n]
    assert exported(tm.vif.LIB_PATH) == declared("turbo_metrics_vif.h")


def test_scores_match_the_formula():
    rng = np.random.default_rng(4)
    for w, h in ((64, 64), (1920, 1080), (33, 47)):
        for _ in range(30):
            den = rng.uniform(1.0, 1e9, (4, 3))
            num = den * rng.uniform(0.0, 1.2, (4, 3))
            got, want = tm.adm.scores(num, den, w, h), R.scores(num, den, w, h)
            # cbrt is within 1 ulp in the C library and in numpy, not correctly rounded: a numerator or denominator (seven cube roots,
            # up to nine additions) is within about 10 * 2^-53 on each side, the quotient of two such within 2 * 2 * 10 * 2^-53 = 4.4e-15
            assert all(abs(g - x) <= 5e-15 * x for g, x in zip(got, want)), (got, want)
    z = np.zeros((4, 3))
    assert tm.adm.scores(z, z, 64, 64) == [1.0] * 5     # num == den
    tiny = np.full((4, 3), 1e-40)
    # 32 x 32: the bands of scale 3 are 2 x 2 and area / 32 = 0.125, cbrt 0.5: num_3 = den_3 = 3 (cbrt(1e-40) + 0.5)
    assert tm.adm.scores(tiny, tiny, 32, 32) == [1.0] * 5
    assert R.score(5e-11, 2.0) == 0.0 and R.score(1.0, 5e-11) == 1.0 and R.score(1.0, 4.0) == 0.25


class _FakeLib:
    """stands in for the library under an Adm object: any call after the plane checks is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_binding_rejects_bad_planes_before_the_library():
    def obj(w, h, layout, bits):
        v = tm.Adm.__new__(tm.Adm)
        v._L, v._h, v._keep = _FakeLib(), None, {}
        v.w, v.h, v.layout, v.bits, v.batch = w, h, layout, bits, 2
        return v
    v = obj(48, 32, "y8", 8)
    good = np.zeros((32, 48), np.uint8)
    for bad in (np.zeros((32, 48), np.uint16), np.zeros((32, 48), np.int8), np.zeros((32, 48), np.float32), np.zeros((31, 48), np.uint8),
                np.zeros((32, 47), np.uint8), np.zeros((32, 96), np.uint8)[:, ::2], np.zeros(48 * 32, np.uint8), [[0] * 48] * 32):
        for pair in ((bad, good), (good, bad)):
            with pytest.raises(ValueError):
                v.set_pair(0, *pair)
    with pytest.raises(ValueError):
        v.set_pair(2, good, good)
    v = obj(48, 32, "y16_low", 10)
    for bad in (np.zeros((32, 48), np.uint8), np.zeros((32, 48), np.int64), np.zeros((32, 40), np.uint16)):
        with pytest.raises(ValueError):
            v.set_pair(0, bad, bad)
    v = obj(400, 32, "y10_packed", 10)
    assert v.plane_shape() == ((32, 256), 4)
    for bad in (np.zeros((32, 400), np.uint16), np.zeros((32, 255), np.uint32)):
        with pytest.raises(ValueError):
            v.set_pair(0, bad, bad)
    import torch
    v = obj(48, 32, "y16_msb", 10)
    for bad in (torch.zeros((32, 48), dtype=torch.uint8), torch.zeros((32, 48), dtype=torch.float16), torch.zeros((48, 32), dtype=torch.int16).t()):
        with pytest.raises(ValueError):
            v.set_pair(0, bad, bad)
    assert tm.Adm is tm.adm.Adm and tm.AdmFrame is tm.adm.AdmFrame and tm.AdmFrame._fields == ("num_cube", "den_cube", "scales", "adm2")


def test_cli_names_adm_and_refuses_what_it_cannot_do_before_touching_the_device(tmp_path):
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    for p in (a, b):
        with open(p, "wb") as f:
            f.write(b"YUV4MPEG2 W32 H32 F25:1 C420jpeg\nFRAME\n" + bytes(32 * 32 + 2 * 256))
    for extra in (["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
        for sel in ([], ["-m", "psnr"], ["-m", "vif"]):
            out = subprocess.run([CLI, a, b, "-m", "adm", *sel, *extra], capture_output=True, text=True, timeout=60)
            assert out.returncode != 0 and "does not run with" in out.stderr and ("-m adm" in out.stderr or "-m vif" in out.stderr), (extra, out.returncode, out.stderr)
        out = subprocess.run([CLI, a, b, "-madm", *extra], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "-m adm does not run with" in out.stderr, (extra, out.returncode, out.stderr)
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "adm" in out.stdout
    out = subprocess.run([CLI, a, "-m", "adm"], capture_output=True, text=True, timeout=60)  # the distorted argument is still required
    assert out.returncode == 2 and "<DISTORTED>" in out.stderr
