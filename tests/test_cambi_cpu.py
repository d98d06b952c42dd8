"""CPU tier of CAMBI: the host functions, hand-derived pictures, and the SOURCE of the kernels run lane by
lane on the CPU (tests/cambi_emul) against the plain numpy restatement (tests/cambi_ref.py) -- masks, filtered planes and c-values
equal plane by plane, t, n_gt and k equal, sum_gt within the bound of a naive f64 sum.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import cambi_ref as R
from tests import cambi_util as U
from tm_pkg import tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbo-metrics_amd", "libturbometrics_cambi.so")
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
f32 = np.float32


def _emul1(Y, layout, bits, window, **kw):
    h, w = Y.shape
    pad = kw.pop("pad", 3)
    pad = 0 if layout == "y10_packed" else pad
    return U.emulate(w, h, layout, bits, [1], [U.luma_plane(layout, Y, bits, pad=pad, dirty=kw.pop("dirty", 9))], window=window, **kw)[0]


# ---- host functions ----------------------------------------------------------------------------------------------------------
def test_host_functions():
    assert tm.cambi.tvi(0.019) == (178, 305, 432, 559) == R.tvi(0.019)
    assert [tm.cambi.mask_index(a, b) for a, b in ((1920, 1080), (3840, 2160), (1280, 720), (64, 64), (32, 32))] == [24, 25, 22, 16, 15]
    assert [R.mask_index(a, b) for a, b in ((1920, 1080), (3840, 2160), (1280, 720), (64, 64), (32, 32))] == [24, 25, 22, 16, 15]
    assert tm.cambi.window(1920, 0) == 31 and tm.cambi.window(3840, 0) == 63 and tm.cambi.window(64, 0) == 3 and tm.cambi.window(64, 9) == 9
    for w in (32, 64, 1280, 1920, 2560, 3840):
        assert tm.cambi.window(w) == R.window_of(w)
    # no x is within 1e-4 relative of a tie at the default threshold: libm differences cannot move the table
    for d, x in zip((1, 2, 3, 4), (178, 305, 432, 559)):
        for xx in (x, x + 1):
            L = R.luminance(xx)
            assert abs((R.luminance(xx + d) - L) / (0.019 * L) - 1.0) > 1e-4


def test_scores_host_function():
    t = [int(f32(v).view(np.uint32)) for v in (2.5, 0.0, 1.0, 7.0, 0.25)]
    n_gt, k, sm = [3, 0, 1, 0, 2], [10, 5, 4, 1, 3], [30.0, 0.0, 2.0, 0.0, 1.0]
    sc, total = tm.cambi.scores(t, n_gt, k, sm, 7)
    want = [(30 + 7 * 2.5) / 10, 0.0, (2 + 3 * 1.0) / 4, 7.0, (1 + 0.25) / 3]
    assert list(sc) == want == R.scores(t, n_gt, k, sm, 7)[0]
    assert total == sum(w * s for w, s in zip((16, 8, 4, 2, 1), want)) / 49 == R.scores(t, n_gt, k, sm, 7)[1]
    assert tm.cambi.scores([int(f32(1e6).view(np.uint32))] * 5, [0] * 5, [1] * 5, [0.0] * 5, 3)[1] == 1000.0  # the cap
    with pytest.raises(ValueError):
        tm.cambi.scores(t, k, k, sm, 7)  # n_gt == k cannot be


# ---- by hand -----------------------------------------------------------------------------------------------------------------
def test_flat_picture_is_zero():
    Y = np.full((64, 64), 100, np.int64)
    for r in (R.compute(Y, 10, 7), _emul1(Y, "y16_msb", 10, 7)):
        # Z = 1 everywhere; B counts zero outside the picture: 49 inside, 4 x 7 = 28 at an edge, 4 x 4 = 16 in a corner, and
        # mask_index(64, 64) = 16: B > 16 everywhere but at the four corner pixels
        want_mask = np.ones((64, 64), bool)
        want_mask[[0, 0, -1, -1], [0, -1, 0, -1]] = False
        assert (r.mask[0] == want_mask).all() and all((m == want_mask[::1 << s, ::1 << s]).all() for s, m in enumerate(r.mask))
        assert all((c == 0).all() for c in r.cmap)  # n(v +- d) = 0 everywhere
        assert r.t == [0] * 5 and r.n_gt == [0] * 5 and r.sum_gt == [0.0] * 5
    assert R.compute(Y, 10, 7).cambi == 0.0


def test_two_flat_halves():
    # columns 0 .. 31 hold 100, columns 32 .. 63 hold 101; window 7 (pad 3); D = 10, so P0 is the picture.
    # Mask: Z = 0 only in column 31 (its right neighbour differs).  B at (i, j) for rows 3 .. 60 is 49 minus the 7 zeros of column 31
    # when |j - 31| <= 3, so at least 42 > 16; at the top edge next to column 31 it is 4 x 7 - 4 = 24 > 16: every pixel near the edge
    # is masked (the four corner pixels of the picture, B = 16, are not).  The mode filter changes nothing: of the nine
    # neighbours of a pixel in column 31 six are 100, of one in column 32 six are 101.
    # The pixel (20, 31): v = 100, its window is rows 17 .. 23 x columns 28 .. 34: the 100s are columns 28 .. 31, 4 x 7 = 28 = p0; the
    # 101s are columns 32 .. 34, 3 x 7 = 21 = n(v + 1); n(v - 1) = 0; n(v + 2 ..) = 0.  c = fl32(1 * 28 * 21) / fl32(28 + 21).
    # The pixel (20, 32): v = 101, p0 = 21, m = n(v - 1) = 28: the same c.  (20, 29): columns 26 .. 32: p0 = 6 * 7 = 42, m = 7: c = 294 / 49,
    # and the same at (20, 34).  (20, 28): the window ends at column 31: no 101 in it: c = 0; (20, 35) likewise.  (0, 31): rows 0 .. 3: p0 = 16, m = 12: c = 192 / 28.
    Y = np.full((64, 64), 100, np.int64)
    Y[:, 32:] = 101
    for r in (R.compute(Y, 10, 7), _emul1(Y, "y16_low", 10, 7)):
        assert r.mask[0][:, 1:-1].all() and not r.mask[0][0, 0]
        c = r.cmap[0]
        assert c[20, 31] == f32(28 * 21) / f32(49) == c[20, 32]
        assert c[20, 29] == f32(294) / f32(49) == c[20, 34] and c[20, 28] == 0 and c[20, 35] == 0
        assert c[0, 31] == f32(192) / f32(28)
        assert float(c.max()) == float(f32(28 * 21) / f32(49))
    # the same step above every visibility threshold: 601 > 559
    for r in (R.compute(Y + 500, 10, 7), _emul1(Y + 500, "y16_low", 10, 7)):
        assert all((c == 0).all() for c in r.cmap) and r.mask[0][:, 1:-1].all()
    # 559 | 560: only d = 4 qualifies at 559 and n(v +- 4) = 0; 558 | 559 likewise: zero.  178 | 179: the left half qualifies for d = 1
    # (178 <= 178), the right half (179) does not: c is non-zero in the columns left of the edge only
    c = R.compute(Y + 78, 10, 7).cmap[0]
    assert c[20, 31] == f32(28 * 21) / f32(49) and c[20, 32] == 0
    assert (_emul1(Y + 78, "y10_packed", 10, 7).cmap[0] == c).all()


def test_anti_dither_written_out():
    Y = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 13], [20, 30, 40, 50]], np.int64)  # D = 8: S = 4 Y
    want = np.array([[(1 + 2 + 5 + 6), (2 + 3 + 6 + 7), (3 + 4 + 7 + 8), (4 + 8) * 2],
                     [(5 + 6 + 9 + 10), (6 + 7 + 10 + 11), (7 + 8 + 11 + 13), (8 + 13) * 2],
                     [(9 + 10 + 20 + 30), (10 + 11 + 30 + 40), (11 + 13 + 40 + 50), (13 + 50) * 2],
                     [(20 + 30) * 2, (30 + 40) * 2, (40 + 50) * 2, 50 * 4]], np.int64)  # (4a + 4b + 4c + 4d) >> 2, (4a + 4b) >> 1, 4a
    assert (R.to10(Y, 8) == want).all()
    assert (R.to10(Y, 10) == Y).all() and (R.to10(Y << 2, 12) == Y).all() and (R.to10((Y << 6) + 63, 16) == Y).all()
    # the kernel: the same 4 x 4 block as the bottom-right corner of a 32 x 32 picture, whose last row and column take the border rules
    big = np.random.default_rng(3).integers(0, 256, (32, 32), dtype=np.int64)
    big[-4:, -4:] = Y
    got = _emul1(big, "y8", 8, 3)
    # scale 0's plane is the mode-filtered P0: its outermost rows and columns are P0 itself
    assert (got.plane[0][-1, -4:] == want[-1]).all() and (got.plane[0][-4:, -1] == want[:, -1]).all()
    assert (got.plane[0] == R.mode3x3(R.to10(big, 8))).all()


def test_mode_filter_tie_rule():
    P = np.array([[7, 7, 3], [3, 9, 5], [1, 2, 4]], np.int64)  # two pairs: 7, 7 and 3, 3 -> the smaller, 3
    assert R.mode3x3(P)[1, 1] == 3 and R.mode3x3_planes(P)[1, 1] == 3
    out = R.mode3x3(P)
    out[1, 1] = 9
    assert (out == P).all()  # the border is unchanged
    P = np.array([[5, 1, 2], [3, 4, 6], [7, 8, 9]], np.int64)  # all different: nine ties -> the smallest, 1
    assert R.mode3x3(P)[1, 1] == 1 == R.mode3x3_planes(P)[1, 1]
    rng = np.random.default_rng(11)
    for _ in range(4):
        P = rng.integers(0, 4, (17, 23), dtype=np.int64)
        assert (R.mode3x3(P) == R.mode3x3_planes(P)).all()


def test_fast_reference_paths_equal_the_literal_ones():
    for w, h, kind, win in ((33, 47, "mixed", 7), (64, 40, "stairs_lo", 15), (40, 36, "noise", 3), (50, 40, "stairs_hi", 63)):
        Y = U.picture(w, h, 10, kind, 2)
        assert U.same(R.compute(Y, 10, win, fast=True), R.compute(Y, 10, win))
    # counts on a plane with a random mask
    rng = np.random.default_rng(5)
    P, M = rng.integers(100, 108, (30, 41), dtype=np.int64), rng.integers(0, 3, (30, 41)) > 0
    assert (R.counts_direct(P, M, 4) == R.counts_by_value(P, M, 4)).all()


# ---- emulated kernels against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", U.SIZES)
@pytest.mark.parametrize("window", U.WINDOWS)
def test_emulated_kernels_equal_the_restatement(w, h, window):
    # the literal restatement where it is quick, its whole-plane form (held to it above) for the larger pictures and windows
    fast = w * h * window * window > 64 * 64 * 15 * 15
    layouts = (("y8", 8), ("y16_msb", 10), ("y16_low", 12), ("y10_packed", 10))
    for i, kind in enumerate(U.KINDS):
        layout, bits = layouts[(i + w + window) % 4]
        Y = U.picture(w, h, bits, kind, seed=w + window)
        want = R.compute(Y, bits, window, fast=fast)
        assert U.same(_emul1(Y, layout, bits, window), want), (kind, layout)


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_layouts_dirty_bits_pitches_and_the_sample_path(layout, bits):
    w, h, window = 33, 47, 7
    for kind in ("stairs_lo", "mixed"):
        Y = U.picture(w, h, bits, kind, seed=bits)
        want = R.compute(Y, bits, window)
        for pad, dirty, vec in ((0, None, None), (5, 3, None), (1, 4, False)):
            assert U.same(_emul1(Y, layout, bits, window, pad=pad, dirty=dirty, vec=vec), want), (kind, pad, dirty, vec)
        plane = U.aligned_copy(U.luma_plane(layout, Y, bits, dirty=6), 3 if layout != "y10_packed" else 0)
        assert U.same(U.emulate(w, h, layout, bits, [1], [plane], window=window, vec=True)[0], want)


def test_topk_and_threshold_parameters():
    Y = U.picture(64, 64, 10, "mixed", 4)
    for topk in (1.0, 0.6, 0.1, 1e-9):
        want = R.compute(Y, 10, 7, topk=topk)
        assert U.same(_emul1(Y, "y16_msb", 10, 7, topk=topk), want)
        assert want.k[4] == max(1, int(math.floor(topk * 16)))
    want = R.compute(Y, 10, 7, tvi_threshold=0.05)
    assert R.tvi(0.05) != R.tvi(0.019)
    assert U.same(_emul1(Y, "y16_msb", 10, 7, thr=0.05), want)


def test_batches_slots_and_repeated_computes():
    w, h, layout, bits, window = 65, 40, "y16_msb", 10, 7
    pics = [U.picture(w, h, bits, U.KINDS[i % 5], seed=20 + i) for i in range(7)]
    want = [R.compute(Y, bits, window, fast=True) for Y in pics]
    assert len({(tuple(r.t), tuple(r.n_gt)) for r in want}) >= 4
    planes = [U.luma_plane(layout, Y, bits, pad=i % 3, dirty=i + 1) for i, Y in enumerate(pics)]
    # one object of 3 slots: computes of 3, 1, 2 and 1 pictures -- slot 0 is computed four times, with other content each time
    got = U.emulate(w, h, layout, bits, [3, 1, 2, 1], planes, window=window, cap=3)
    for g, r in zip(got, want):
        assert U.same(g, r)
    # three computes of the same picture into one slot: identical bits in every field
    three = U.emulate(w, h, layout, bits, [1, 1, 1], [planes[2]] * 3, window=window)
    for g in three[1:]:
        assert g.t == three[0].t and g.n_gt == three[0].n_gt and g.k == three[0].k
        assert np.array(g.sum_gt).tobytes() == np.array(three[0].sum_gt).tobytes()
        assert all((a.view(np.uint32) == b.view(np.uint32)).all() for a, b in zip(g.cmap, three[0].cmap))


def test_geometry_strips_and_bands_are_exercised():
    # what the sizes above stand on: more than one strip of columns and more than one band of rows per picture
    g = U.geom(200, 96, "y8", 8, 3)
    assert g.oc < 200 and g.band_rows < 96 and g.w == [200, 100, 50, 25, 13] and g.h == [96, 48, 24, 12, 6]
    g = U.geom(200, 96, "y8", 8, 63)
    assert g.oc == 156 - 62 and 2 * g.oc < 200 and g.w[3] < 63 and g.h[2] < 63  # three strips; the window covers the small scales
    g = U.geom(129, 67, "y8", 8, 15)
    assert g.band_rows < 67
    assert U.geom(33, 47, "y8", 8, 0).window == 3 and U.geom(33, 47, "y8", 8, 7).band_rows < 47


# ---- refusals, exports, binding, CLI -------------------------------------------------------------------------------------------------
def test_refusals():
    ok = dict(w=64, h=64, layout="y16_msb", bits=10, window=0, topk=0.6)
    bad = [dict(w=31), dict(h=31), dict(w=1 << 16, h=(1 << 15) + 1), dict(bits=7), dict(bits=17), dict(layout="y8"), dict(layout="y16_msb", bits=8),
           dict(layout="y10_packed", bits=12), dict(layout=7), dict(window=1), dict(window=2), dict(window=128), dict(topk=0.0), dict(topk=1.0001),
           dict(topk=-0.5), dict(topk=float("nan"))]
    L = tm.cambi.lib()
    for b in [{}] + bad:
        a = {**ok, **b}
        lay = tm.cambi.LAYOUTS.get(a["layout"], a["layout"])
        refused = U.geom(a["w"], a["h"], lay, a["bits"], a["window"], a["topk"]) is None
        assert refused == bool(b), a
        if b:  # before any device call: there is no device here
            h_ = C.c_void_p()
            assert L.tm_cambi_create(C.byref(h_), a["w"], a["h"], lay, a["bits"], a["window"], a["topk"], 0.019, 1) == tm.ffi.TM_ERR_UNSUPPORTED, a
            assert not h_.value
    h_ = C.c_void_p()
    assert L.tm_cambi_create(None, 64, 64, 1, 10, 0, 0.6, 0.019, 1) == tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_cambi_create(C.byref(h_), 64, 64, 1, 10, 0, 0.6, 0.019, 0) == tm.ffi.TM_ERR_INVALID_ARG


def test_library_exports_exactly_its_header():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    got = sorted(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert got == sorted(tm.cambi.SYMBOLS)
    header = open(os.path.join(ROOT, "include", "turbo_metrics_cambi.h")).read()
    assert all(name + "(" in header for name in tm.cambi.SYMBOLS)
    # no symbol of it in another library
    for other in ("libturbometrics_hip.so", "libturbometrics_scene.so", "libturbometrics_adm.so"):
        o = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "turbo-metrics_amd", other)], capture_output=True, text=True, check=True).stdout
        assert "tm_cambi" not in o


def test_binding_checks_its_arguments_before_the_library():
    assert C.sizeof(tm.cambi.CambiFrameC) == 104
    assert tm.Cambi is tm.cambi.Cambi and tm.CambiFrame._fields == ("cambi", "scales", "t", "n_gt", "k", "sum_gt")
    with pytest.raises(tm.cambi.CambiError) as e:
        tm.Cambi(16, 64, "y8", 8)
    assert e.value.code == tm.ffi.TM_ERR_UNSUPPORTED
    with pytest.raises(KeyError):
        tm.Cambi(64, 64, "nv12", 8)


def test_cli_option_parsing():
    def run(*a):
        return subprocess.run([CLI, *a], capture_output=True, text=True, timeout=60)
    assert "cambi" in run("--help").stdout and "--cambi-window" in run("--help").stdout and "--cambi-topk" in run("--help").stdout
    for bad in (["--cambi-window", "2"], ["--cambi-window", "128"], ["--cambi-window", "x"], ["--cambi-topk", "0"], ["--cambi-topk", "1.5"],
                ["--cambi-window"], ["--cambi-topk"]):
        out = run("a.y4m", "b.y4m", "-m", "cambi", *bad)
        assert out.returncode != 0 and "cambi" in out.stderr, bad
    for alone in (["--cambi-window", "7"], ["--cambi-topk", "0.5"], ["--cambi-ref"]):
        out = run("a.y4m", "b.y4m", "-m", "psnr", *alone)
        assert out.returncode != 0 and "-m cambi" in out.stderr, alone
