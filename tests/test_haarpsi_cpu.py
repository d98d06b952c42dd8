"""HaarPSI without a GPU: the float64 restatement in the paper's form (tests/haarpsi_ref.py), hand values derived on
paper, the kernel SOURCE run lane by lane on the CPU (tests/haarpsi_emul) against the restatement with the measured tolerance of
tests/haarpsi_util.py, seeded mistakes, the library's ABI and refusals, the binding's plane checks and the CLI's usage."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import haarpsi_ref as R
from tests import haarpsi_util as U
from tm_pkg import tm

P = tm.haarpsi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLIB = P.LIB_PATH
F = np.float32


def _emul1(a, b, layout, bits, maps=False, pad=0):
    h, w = a.shape
    out = U.emulate(w, h, layout, bits, [1], U.planes_of(layout, [(a, b)], bits, pad=pad), maps=maps)
    return (out[0][0], out[1][0]) if maps else out[0]


def _s32(e1, e2):
    """the kernel's s = 1 - (e_1 + e_2) / 2 in f32"""
    return float(F(1.0) - F(0.5) * (F(e1) + F(e2)))


# ---- hand values ---------------------------------------------------------------------------------------------------------------
def test_the_restatements_convolution_is_matlabs_same():
    a = np.arange(12, dtype=np.float64).reshape(3, 4)
    # conv2(a, ones(2), 'same'): out(i, j) = a(i, j) + a(i, j+1) + a(i+1, j) + a(i+1, j+1), zeros beyond the end
    assert R.conv2_same(a, np.ones((2, 2))).tolist() == [[10, 14, 18, 10], [26, 30, 34, 18], [17, 19, 21, 11]]
    # scipy's convolve2d(mode='same') reaches the other way: out(i, j) = a(i-1, j-1) + a(i-1, j) + a(i, j-1) + a(i, j)
    assert R.conv2_same(a, np.ones((2, 2)), scipy_centring=True).tolist() == [[0, 1, 3, 5], [4, 10, 14, 18], [12, 26, 30, 34]]
    # conv2 flips the kernel: [1 0 -1] gives a(j+1) - a(j-1); an odd kernel is centred alike in both
    for sc in (False, True):
        assert R.conv2_same(a, np.array([[1.0, 0.0, -1.0]]), scipy_centring=sc).tolist() == [[1, 2, 2, -2], [5, 2, 2, -6], [9, 2, 2, -10]]
    # a window of 4: rows y-1 .. y+2; the vertical Haar filter of scale 2 on a column 1, 2, 3, 4, 5: conv2 flips it, so
    # out(y) = (a(y+1) + a(y+2)) - (a(y-1) + a(y)), each row summed over 4 columns (1 here: one column in, the rest zeros) and times 1/4
    col = np.arange(1.0, 6.0).reshape(5, 1)
    assert (R.conv2_same(col, R.haar(2)) * 4).ravel().tolist() == [(2 + 3) - 1, (3 + 4) - (1 + 2), (4 + 5) - (2 + 3), 5 - (3 + 4), 0 - (4 + 5)]


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_identical_pictures_score_one(layout, bits):
    """e = 0 at every position, scale and orientation, so s = 1 and q is ONE constant, 1 - sigmoid(4.2): the weights cancel and the
    score is (logit(sigmoid(4.2)) / 4.2)^2 = 1.  The restatement gives it within 1e-12; in the kernel q is the f32
    1 / (1 + exp_pos(4.2f)), so Q / WS is that constant and the score is 1 to q's f32 rounding (6e-8 / 4.2 relative)."""
    a, _ = U.pair(33, 19, bits, "noise", 3)
    r = R.haarpsi(a, a, bits)
    assert abs(r.haarpsi - 1.0) < 1e-12 and (r.sim == 1.0).all()
    (q, ws), m = _emul1(a, a, layout, bits, maps=True)
    assert ws > 0 and (m == F(1.0)).all() and abs(q / ws - U.kernel_q(1.0)) < 1e-12
    assert abs(U.score(q, ws) - 1.0) <= U.ABS_TOL and abs(P.score(q, ws) - 1.0) <= U.ABS_TOL


def test_two_black_pictures_have_no_weight_and_score_nan():
    """WS = 0 needs every scale-3 coefficient of both pictures to be 0: under the zero border that is two all-zero pictures (a flat
    picture of another value has coefficients where a window straddles the border).  0 / 0: NaN, as MATLAB gives."""
    z = np.zeros((9, 12), np.int64)
    r = R.haarpsi(z, z, 8)
    assert math.isnan(r.haarpsi) and r.den == 0.0
    for layout, bits in U.CASES:
        q, ws = _emul1(z, z, layout, bits)
        assert (q, ws) == (0.0, 0) and math.isnan(U.score(q, ws)) and math.isnan(P.score(q, ws))
    flat = np.full((9, 12), 50, np.int64)
    assert _emul1(flat, flat, "y8", 8)[1] > 0 and abs(R.haarpsi(flat, flat, 8).haarpsi - 1.0) < 1e-12


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_zero_against_a_flat_4x4_picture(layout, bits):
    """R = 0, D = v everywhere, 4 x 4: the decimated plane is 2 x 2 with S = 4 v; |H| of R is 0 everywhere.  Of D, with windows of rows
    y - K/2 + 1 .. y + K/2 (columns alike) and zeros outside:
      K = 2:  Hv_1 = (S(y, x) + S(y, x+1)) - (S(y+1, x) + S(y+1, x+1)):  0 in row 0 (both rows inside), 8 v at (1, 0), 4 v at (1, 1)
      K = 4:  both columns lie in every window; upper rows y-1 .. y, lower y+1 .. y+2:  0 in row 0 (8 v - 8 v), 16 v in row 1
      K = 8:  likewise: 0 in row 0, 16 v in row 1
    and Hh is the transpose.  So W_v = 16 v in row 1, W_h = 16 v in column 1, WS = 64 v, and with a = 0, e_k = d^2 / (d^2 + C_k),
    C_1 = 1920, C_2 = 7680:
      v at (1, 0) and h at (0, 1):  e_1 = 64 v^2 / (64 v^2 + 1920) = e_2 = 256 v^2 / (256 v^2 + 7680) = v^2 / (v^2 + 30)
      v and h at (1, 1):            e_1 = 16 v^2 / (16 v^2 + 1920) = v^2 / (v^2 + 120), e_2 = v^2 / (v^2 + 30)
    Q = 32 v (q_A + q_B), x = (q_A + q_B) / 2.  At depth b the same content is v * 2^(b - 8) and C grows by 4^(b - 8): every e has the
    same bits, Q and WS grow by 2^(b - 8) exactly."""
    k = 1 << (bits - 8)
    for v in (1, 7, 100, 255):
        sA = 30.0 / (v * v + 30.0)
        sB = 1.0 - (v * v / (v * v + 120.0) + v * v / (v * v + 30.0)) / 2
        want = R.logit((R.sigmoid(sA) + R.sigmoid(sB)) / 2) ** 2
        a, b = np.zeros((4, 4), np.int64), np.full((4, 4), v * k, np.int64)
        r = R.haarpsi(a, b, bits)
        assert abs(r.haarpsi - want) < 1e-12 and abs(r.den - 4 * v / 2) < 1e-12  # four weights of the paper's scale-3 coefficient 16 v / (4 * 8)
        # the kernel's own f32 values of the two kinds of position, from the 8-bit integers
        eA = U.kernel_e(0, 8 * v, 1920)
        assert eA == U.kernel_e(0, 16 * v, 7680) == U.kernel_e(8 * v, 0, 1920) == U.kernel_e(0, 8 * v * k, 1920 * k * k)
        qA = U.kernel_q(_s32(eA, eA))
        sB32 = _s32(U.kernel_e(0, 4 * v, 1920), U.kernel_e(0, 16 * v, 7680))
        qB = U.kernel_q(sB32)
        for x, y in ((a, b), (b, a)):
            (q, ws), m = _emul1(x, y, layout, bits, maps=True)
            assert ws == 64 * v * k and q == 16.0 * v * k * (2 * qA + 2 * qB)  # products and sums of few f32 values: exact in f64
            assert abs(U.score(q, ws) - want) <= U.ABS_TOL and P.score(q, ws) == U.score(q, ws)
            # the map: (s_v + s_h) / 2; s = 1 where both coefficients of both scales are 0
            sA32 = _s32(eA, eA)
            assert m.tolist() == [[1.0, float(F(0.5) * (F(1.0) + F(sA32)))], [float(F(0.5) * (F(sA32) + F(1.0))), float(F(0.5) * (F(sB32) + F(sB32)))]]
            assert np.abs(m - r.sim).max() < 2e-7


def test_zero_against_flat_100_at_16x16_is_the_recorded_value():
    a, b = np.zeros((16, 16), np.int64), np.full((16, 16), 100, np.int64)
    assert abs(R.haarpsi(a, b, 8).haarpsi - 0.141890556) < 1e-9
    assert abs(U.score(*_emul1(a, b, "y8", 8)) - 0.141890556) <= U.ABS_TOL + 1e-9


def test_an_odd_sized_picture_takes_zeros_beyond_its_edges():
    """5 x 7, R = 0, D = 60: w2 = 3, h2 = 4; S = 240 where the 2 x 2 cell lies inside, 120 in column 2 (sample column 5 is 0) and in row 3
    (sample row 7 is 0), 60 at their crossing.  Whatever lies behind a row or below the picture in memory changes nothing."""
    a, b = np.zeros((7, 5), np.int64), np.full((7, 5), 60, np.int64)
    r = R.haarpsi(a, b, 8)
    # scale-3 weights by hand: every window holds all 3 columns / all 4 rows of its direction.  Hv_3(y): rows <= y minus rows > y of the
    # column sums 600 = 240 + 240 + 120 (rows 0 .. 2) and 300 (row 3): |600 - 1500|, |1200 - 900|, |1800 - 300|, 2100; Hh_3(x): columns
    # <= x minus columns > x of the row sums 840, 840, 420: |840 - 1260|, |1680 - 420|, 2100
    ws = 3 * (900 + 300 + 1500 + 2100) + 4 * (420 + 1260 + 2100)
    base = _emul1(a, b, "y8", 8)
    assert base[1] == ws and abs(r.den - ws / 32.0) < 1e-9
    for pad in (1, 3):
        assert _emul1(a, b, "y8", 8, pad=pad) == base  # garbage right behind each row
    assert abs(U.score(*base) - r.haarpsi) <= U.ABS_TOL
    assert math.isnan(R.haarpsi(a, b, 8, "replicate").haarpsi)  # a replicated border leaves two flat pictures no coefficient at all


def test_host_function():
    assert math.isnan(P.score(0.0, 0)) and math.isnan(P.score(1.0, 0))
    for q, ws in ((0.25, 1), (1.0, 3), (104756.64780139923, 614400), (5e9, 10 ** 12)):
        x = q / ws
        assert P.score(q, ws) == U.score(q, ws) == (math.log((1 - x) / x) / U.ALPHA_F32) ** 2
    assert U.ALPHA_F32 == 4.19999980926513671875 == float(U.emul_lib().he_alpha())
    # logit(sigmoid(A s)) / A = s holds when the host divides by the f32 alpha the device multiplied by
    for s in (0.1, 0.5, 0.9, 1.0):
        x = 1.0 / (1.0 + math.exp(U.ALPHA_F32 * s))
        assert abs(P.score(x * 1000, 1000) - s * s) < 1e-12
    # a sequence: the same function of the summed sums
    refs = [R.haarpsi(*U.pair(21, 14, 8, "blur", s), 8) for s in range(3)]
    got = [_emul1(*U.pair(21, 14, 8, "blur", s), "y8", 8) for s in range(3)]
    assert abs(P.score(sum(g[0] for g in got), sum(g[1] for g in got)) - R.pooled(refs)) <= U.ABS_TOL


def test_the_kernels_exponential():
    """exp_pos against float64 on [0, 4.2]: the degree-7 polynomial leaves 5e-9, the f32 operations about 1.5 ulp"""
    z = np.linspace(0.0, U.ALPHA_F32, 4001).astype(F)
    got = np.array([U.kernel_exp(v) for v in z])
    assert np.abs(got / np.exp(z.astype(np.float64)) - 1).max() < 2.5e-7
    assert U.kernel_exp(0.0) == 1.0 and U.kernel_q(0.0) == 0.5


# ---- the kernel source against the restatement -----------------------------------------------------------------------------------
def test_emulation_against_restatement(capsys):
    """every shape, layout / depth and kind, several slots per compute on reused buffers, both load paths.  Prints the largest absolute
    error of the score: haarpsi_util.ABS_TOL is that figure times 4, and the figure may not exceed 1e-5."""
    worst = 0.0
    for w, h in U.shapes():
        for layout, bits in U.CASES:
            pairs = [U.pair(w, h, bits, k) for k in U.KINDS]
            want = [R.haarpsi(a, b, bits) for a, b in pairs]
            for aligned in (False, True):
                frames = U.planes_of(layout, pairs, bits, pad=0 if aligned else 3, aligned=aligned)
                got = U.emulate(w, h, layout, bits, [3, len(pairs) - 3], frames, cap=4)
                for kind, wt, g in zip(U.KINDS, want, got):
                    unit = 32 << (bits - 8)  # integer units per unit of the paper's scale-3 coefficient
                    assert abs(g[1] - wt.den * unit) <= 1e-9 * max(1.0, wt.den * unit), (w, h, layout, bits, kind, aligned)
                    e = abs(U.score(*g) - wt.haarpsi)
                    assert e <= U.ABS_TOL, (w, h, layout, bits, kind, aligned, e)
                    worst = max(worst, e)
    with capsys.disabled():
        print(f"\nHaarPSI emulation against restatement: largest absolute error of the score {worst:.3g}; tolerance {U.ABS_TOL:.3g}")
    assert worst <= U.MEASURED_ABS * 1.0001 and U.ABS_TOL == 4 * U.MEASURED_ABS and U.MEASURED_ABS <= 1e-5


def test_the_map_is_the_unweighted_local_similarity():
    w, h = U.shapes()[6]
    for layout, bits in (("y8", 8), ("y16_low", 12), ("y10_packed", 10)):
        pairs = [U.pair(w, h, bits, k, seed=2) for k in ("noise", "blur")]
        got, maps = U.emulate(w, h, layout, bits, [2], U.planes_of(layout, pairs, bits), maps=True)
        assert U.emulate(w, h, layout, bits, [2], U.planes_of(layout, pairs, bits)) == got  # the sums with maps on and off
        for (a, b), m in zip(pairs, maps):
            want = R.haarpsi(a, b, bits)
            # f32: four e of relative error 2^-23 each, two sums, three roundings near 1
            assert m.shape == want.sim.shape and np.abs(m.astype(np.float64) - want.sim).max() < 3e-7 and m.max() <= 1.0 and m.min() > 0.0


def test_load_paths_slots_and_repeats_give_the_same_bits():
    w, h = U.shapes()[8]
    for layout, bits in U.CASES:
        pairs = [U.pair(w, h, bits, k, seed=5) for k in ("noise", "blur", "near_peak")]
        tight = U.planes_of(layout, pairs, bits)
        one = [U.emulate(w, h, layout, bits, [1], [f])[0] for f in tight]
        assert U.emulate(w, h, layout, bits, [3], tight) == one
        assert U.emulate(w, h, layout, bits, [2, 1], tight, cap=5) == one  # a second compute owes nothing to the first
        assert U.emulate(w, h, layout, bits, [3], U.planes_of(layout, pairs, bits, pad=2, aligned=True)) == one
        assert U.emulate(w, h, layout, bits, [3], tight, vec=False) == one


def test_nothing_behind_a_row_or_below_the_picture_is_read():
    """an odd width and height: whatever lies right behind a row and in the rows below changes nothing"""
    w, h = 2 * U.tile()[0] + 1, 9
    a, b = U.pair(w, h, 8, "noise", 2)
    base = U.emulate(w, h, "y8", 8, [1], U.planes_of("y8", [(a, b)], 8, dirty=False))
    for pad, aligned in ((1, False), (3, False), (2, True)):
        assert U.emulate(w, h, "y8", 8, [1], U.planes_of("y8", [(a, b)], 8, pad=pad, aligned=aligned)) == base
    big = []  # the planes inside taller arrays whose extra rows are garbage
    for p in U.planes_of("y8", [(a, b)], 8)[0]:
        q = np.full((h + 2, p.shape[1]), 255, p.dtype)
        q[:h] = p
        big.append(q[:h])
    assert U.emulate(w, h, "y8", 8, [1], [tuple(big)]) == base


# ---- seeded mistakes -------------------------------------------------------------------------------------------------------------
MISTAKE_PICTURE = {"scipy_centring": ((24, 16), 8, "blur"), "replicate": ((24, 16), 8, "blur"), "weights_scale2": ((24, 16), 8, "blur"),
                   "logistic_per_scale": ((24, 16), 8, "blur"), "c_unscaled": ((24, 16), 10, "blur")}


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_seeded_mistakes_are_caught(mistake):
    """each mistake moves the restatement's score of one fixed picture by more than the tolerance"""
    (w, h), bits, kind = MISTAKE_PICTURE[mistake]
    a, b = U.pair(w, h, bits, kind, seed=9)
    right, wrong = R.haarpsi(a, b, bits), R.haarpsi(a, b, bits, mistake)
    assert abs(wrong.haarpsi - right.haarpsi) > U.ABS_TOL, (mistake, right.haarpsi, wrong.haarpsi)
    assert R.haarpsi(a, b, bits, None).haarpsi == right.haarpsi


def test_the_emulation_agrees_where_each_mistake_bites():
    """the pictures of the seeded mistakes: the kernel source is on the right side of every one"""
    for (w, h), bits, kind in sorted(set(MISTAKE_PICTURE.values())):
        a, b = U.pair(w, h, bits, kind, seed=9)
        got = _emul1(a, b, "y8" if bits == 8 else "y16_msb", bits, pad=1)
        assert abs(U.score(*got) - R.haarpsi(a, b, bits).haarpsi) <= U.ABS_TOL


# ---- refusals and ABI ------------------------------------------------------------------------------------------------------------
def _supported(w, h, layout, bits):
    return 4 <= w <= 32768 and 4 <= h <= 32768 and {"y8": bits == 8, "y16_msb": 9 <= bits <= 16, "y16_low": 9 <= bits <= 16, "y10_packed": bits == 10}[layout]


GEOMS = ((4, 4), (3, 4), (4, 3), (0, 0), (32768, 4), (32769, 4), (4, 32769), (1920, 1080))


def test_create_refuses_before_touching_the_device():
    L = P.lib()
    h = C.c_void_p()
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 12, 16, 17):
            for w, hh in GEOMS + ((0xFFFFFFFF, 0xFFFFFFFF),):
                ok = _supported(w, hh, layout, bits)
                assert (U.geom(w, hh, layout, bits) is not None) == ok
                if not ok:
                    for flags in (0, P.TM_HAARPSI_MAPS):
                        assert L.tm_haarpsi_create(C.byref(h), w, hh, U.LAYOUT[layout], bits, 1, flags) == tm.ffi.TM_ERR_UNSUPPORTED, (layout, bits, w, hh)
    assert L.tm_haarpsi_create(C.byref(h), 16, 16, 4, 8, 1, 0) == tm.ffi.TM_ERR_UNSUPPORTED
    assert L.tm_haarpsi_create(None, 16, 16, 0, 8, 1, 0) == tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_haarpsi_create(C.byref(h), 16, 16, 0, 8, 0, 0) == tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_haarpsi_create(C.byref(h), 16, 16, 0, 8, 65536, 0) == tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_haarpsi_create(C.byref(h), 16, 16, 0, 8, 1, 2) == tm.ffi.TM_ERR_INVALID_ARG
    assert h.value is None
    # C_k at every depth: 30 * 16 * 4^k * 4^(b - 8)
    for bits in range(9, 17):
        assert U.geom(64, 64, "y16_low", bits)[3:] == (30 * 16 * 4 * 4 ** (bits - 8), 30 * 16 * 16 * 4 ** (bits - 8))
    assert U.geom(64, 64, "y8", 8) == (32, 32, 1, 1920, 7680) and U.geom(5, 7, "y8", 8)[:2] == (3, 4)


def declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(2) for m in re.finditer(r" ([A-Za-z]) (\S+)", out) if m.group(1) in "TDBRW" and not m.group(2).startswith(("_init", "_fini", "__bss", "_edata", "_end")))


def test_header_is_plain_c99_and_the_library_exports_exactly_it(tmp_path):
    want = declared("turbo_metrics_haarpsi.h")
    assert len(want) == 9 and all(n.startswith("tm_haarpsi") for n in want)
    assert exported(PLIB) == want
    assert sorted(P.SYMBOLS) == want
    listed = re.findall(r"^\s*(tm_[a-z0-9_]+);", open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "haarpsi.map")).read(), flags=re.M)
    assert sorted(listed) == want
    assert P.LAYOUTS == tm.gmsd.LAYOUTS == U.LAYOUT
    src = tmp_path / "c.c"
    src.write_text('#include "turbo_metrics_haarpsi.h"\n#include "turbo_metrics_gmsd.h"\n#include <stdio.h>\n'
                   "int main(void) { tm_haarpsi *s = NULL; tm_haarpsi_frame f; (void)s; (void)f;\n"
                   "  if ((int)TM_HAARPSI_Y8 != (int)TM_GMSD_Y8 || (int)TM_HAARPSI_Y16_MSB != (int)TM_GMSD_Y16_MSB || (int)TM_HAARPSI_Y16_LOW != (int)TM_GMSD_Y16_LOW ||\n"
                   "      (int)TM_HAARPSI_Y10_PACKED != (int)TM_GMSD_Y10_PACKED || TM_HAARPSI_MAPS != 1 || sizeof f != 16) return 3;\n"
                   "  if (tm_haarpsi_score(0.0, 0) == tm_haarpsi_score(0.0, 0)) return 4; /* NaN */\n"
                   "  printf(\"%.12f %.12f\\n\", tm_haarpsi_score(0.25, 1), tm_haarpsi_score(1.0, 3)); return 0; }\n")
    exe = str(tmp_path / "c")
    lib_dir = os.path.dirname(PLIB)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                           "-L" + lib_dir, "-lturbometrics_haarpsi", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "%.12f %.12f" % (U.score(0.25, 1), U.score(1.0, 3)), (out.returncode, out.stdout, out.stderr)
    assert C.sizeof(P.HaarPsiFrameC) == 16


def test_the_other_libraries_export_nothing_of_it():
    for lib in (tm.ffi.SHIP_LIB_PATH, tm.ffi.LIB_PATH, tm.xpsnr.LIB_PATH, tm.motion.LIB_PATH, tm.vif.LIB_PATH, tm.adm.LIB_PATH, tm.scene.LIB_PATH,
                tm.cambi.LIB_PATH, tm.flip.LIB_PATH, tm.yuv.LIB_PATH, tm.hvs.LIB_PATH, tm.ciede.LIB_PATH, tm.siti.LIB_PATH, tm.gmsd.LIB_PATH):
        assert not [n for n in exported(lib) if "tm_haarpsi" in n], lib


def test_the_kernel_source_keeps_to_plain_stores_and_calls_no_libm_transcendental():
    src = open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "tm_haarpsi_kernels.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code.lower() and "asm" not in code and "hipMemset" not in open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "tm_haarpsi.hip")).read()
    assert not re.search(r"\b(expf?|exp2f?|__expf|logf?|powf?|tanhf?|sqrtf?)\s*\(", code)


class _FakeLib:
    """stands in for the library under a HaarPsi object: any call after the plane checks is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_binding_rejects_bad_planes_before_the_library():
    m = tm.HaarPsi.__new__(tm.HaarPsi)
    m._L, m._h, m._keep = _FakeLib(), None, {}
    m.w, m.h, m.layout, m.bits, m.batch, m.maps = 16, 16, "y8", 8, 2, True
    y = np.zeros((16, 16), np.uint8)
    for bad in (y.astype(np.uint16), y.astype(np.float32), y[:15], y[:, :15], np.zeros((16, 32), np.uint8)[:, ::2], np.zeros(256, np.uint8), [[0] * 16] * 16,
                y.astype(np.int8)):
        with pytest.raises(ValueError):
            m.set_pair(0, y, bad)
        with pytest.raises(ValueError):
            m.set_pair(0, bad, y)
    with pytest.raises(ValueError):
        m.set_pair(2, y, y)
    for bad in (np.zeros((8, 8), np.float64), np.zeros((7, 8), np.float32), np.zeros((8, 7), np.float32), np.zeros((8, 16), np.float32)[:, ::2], np.zeros(64, np.float32)):
        with pytest.raises(ValueError):
            m.map(0, out=bad)
    assert tm.haarpsi.HaarPsi is tm.HaarPsi and tm.HaarPsiFrame is P.HaarPsiFrame and P.HaarPsiFrame._fields == ("haarpsi", "q", "ws")


# ---- CLI -------------------------------------------------------------------------------------------------------------------------
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
VALUES = "possible values: psnr, ssim, msssim, ssimulacra2, xpsnr, vif, adm, cambi, flip, psnr-yuv, ssim-yuv"


def test_cli_names_the_value_and_refuses_what_it_cannot_do_before_touching_the_device(tmp_path):
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    for p in (a, b):
        with open(p, "wb") as f:
            f.write(b"YUV4MPEG2 W16 H16 F25:1 C420jpeg\nFRAME\n" + bytes(16 * 16 + 2 * 64))

    def run(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)
    out = run("--help")
    assert out.returncode == 0 and all(s in out.stdout for s in ("-m haarpsi ", "--haarpsi-map <PREFIX>", "[and: haarpsi]"))
    lines = out.stdout.splitlines()
    at = [i for i, x in enumerate(lines) if x.endswith("[possible values: psnr, ssim, msssim, ssimulacra2, xpsnr]")]
    assert len(at) == 1  # the earlier lines stay byte for byte, haarpsi goes on a further line below them
    assert [x.strip() for x in lines[at[0] + 1:at[0] + 6]] == ["[further values, each described below: vif, adm, cambi, flip, psnr-yuv, ssim-yuv]", "[and: psnr-hvs, psnr-hvs-m]",
                                                               "[and: ciede2000]", "[and: gmsd]", "[and: haarpsi]"]
    for sel in (["-m", "haarpsi"], ["-mhaarpsi", "-m", "psnr"], ["--metrics", "haarpsi", "--motion"], ["-m", "haarpsi", "--haarpsi-map", str(tmp_path / "m")]):
        for extra in (["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
            out = run(a, b, *sel, *extra)
            assert out.returncode != 0 and out.returncode != 2 and "-m haarpsi does not run with" in out.stderr, (sel, extra, out.returncode, out.stderr)
    assert not list(tmp_path.glob("m*.pfm"))
    # usage errors: exit code 2
    for bad in ("HaarPSI", "haar", "haarpsi,psnr", "haarpsi-map"):
        for form in (["-m", bad], ["-m" + bad], ["--metrics", bad]):
            out = run(a, b, *form)
            assert out.returncode == 2 and f"'{bad}'" in out.stderr, (form, out.returncode, out.stderr)
            assert "[" + VALUES + ", psnr-hvs, psnr-hvs-m] [and: ciede2000] [and: gmsd] [and: haarpsi]" in out.stderr
    for opts in (["--haarpsi-map", "x"], ["--haarpsi-map=x", "-m", "psnr"], ["--haarpsi-map", "x", "-m", "gmsd"]):
        out = run(a, b, *opts)
        assert out.returncode == 2 and "belongs to '-m haarpsi'" in out.stderr, (opts, out.returncode, out.stderr)
    out = run(a, b, "-m", "haarpsi", "--haarpsi-map")
    assert out.returncode == 2 and "--haarpsi-map <PREFIX>" in out.stderr
    out = run(a, "-m", "haarpsi")  # the distorted argument is still required
    assert out.returncode == 2 and "<DISTORTED>" in out.stderr
