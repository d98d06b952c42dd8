"""CIEDE2000 without a GPU: the 34 published pairs against the library's double functions, the float64
restatement (tests/ciede_ref.py) and the kernel's f32 device function; hand values; the kernel SOURCE run lane by lane on the CPU
(tests/ciede_emul) against the restatement with the measured tolerance of tests/ciede_util.py; seeded mistakes; the library's ABI and
refusals; the CLI's usage."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ciede_ref as R
from tests import ciede_util as U
from tm_pkg import tm

D = tm.ciede
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DLIB = D.LIB_PATH
BOUNDARY_ROWS = range(8, 16)  # rows 9 .. 16 of the table: on the mean-hue branch boundary (row 10 exactly 180 degrees apart)


# ---- the published pairs ---------------------------------------------------------------------------------------------------------
def test_double_functions_reproduce_the_sharma_table_in_both_orders():
    T = U.sharma()
    assert T.shape == (34, 7)
    worst = 0.0
    for r in T:
        for a, b in ((r[:3], r[3:6]), (r[3:6], r[:3])):
            for got in (D.de00(a, b), float(R.de00(a, b))):
                worst = max(worst, abs(got - r[6]))
                assert abs(got - r[6]) <= U.SHARMA_TOL, (r, got)
            assert abs(D.de00(a, b) - float(R.de00(a, b))) < 1e-11
    print(f"sharma: largest |double - printed| {worst:.3e}")
    assert D.de00((50, 2.5, 0), (50, 2.5, 0)) == 0.0
    assert math.isnan(D.de00((50, 0, 0), (60, 0, 0), (0, 1, 1))) and math.isnan(D.de00((50, 0, 0), (60, 0, 0), (1, 1, -1)))


def test_device_function_reproduces_the_sharma_table():
    T = U.sharma()
    for i, r in enumerate(T):
        for a, b in ((r[:3], r[3:6]), (r[3:6], r[:3])):
            got = U.kernel_de00(a, b)
            wants = [float(R.de00(a, b))] + ([float(R.de00(a, b, flip=True))] if i in BOUNDARY_ROWS else [])
            assert any(abs(got - w) <= U.ATOL + U.RTOL * w for w in wants), (i + 1, got, wants)
    assert U.kernel_de00((50, 2.5, 0), (50, 2.5, 0)) == 0.0


# ---- hand values -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (8, 10, 16))
def test_mid_grey(bits):
    s = 1 << (bits - 8)
    L, a, b = D.lab(126 * s, 128 * s, 128 * s, "bt709", bits)
    lin = ((110 / 219 + 0.055) / 1.055) ** 2.4
    want_L = 116 * (lin * (0.2126729 + 0.7151522 + 0.0721750)) ** (1 / 3) - 16
    assert abs(L - want_L) < 1e-9 and abs(a) < 1e-4 and abs(b) < 1e-4  # (the luminance row of the matrix sums to 1.0000001)
    for m in R.MATRIX:  # neutral chroma: the matrix takes no part
        assert np.allclose(D.lab(126 * s, 128 * s, 128 * s, m, bits), (L, a, b), atol=1e-12)
        assert np.allclose([float(t) for t in R.lab(126 * s, 128 * s, 128 * s, bits, m)], (L, a, b), atol=1e-9)
    k = U.kernel_lab(126 * s, 128 * s, 128 * s, "bt709", bits)
    assert abs(k[0] - want_L) < 2e-5 and abs(k[1]) < 1e-4 and abs(k[2]) < 1e-4


def test_luma_step_on_grey_is_dl_over_sl():
    w, h, bits = 6, 4, 8
    g = (np.full((h, w), 126), np.full((2, 3), 128), np.full((2, 3), 128))
    d = (g[0].copy(), g[1], g[2])
    d[0][:, 3:] = 140
    want = R.picture(g, d, bits)
    L1, L2 = D.lab(126, 128, 128)[0], D.lab(140, 128, 128)[0]
    Lb = (L1 + L2) / 2
    closed = abs(L2 - L1) / (1 + 0.015 * (Lb - 50) ** 2 / math.sqrt(20 + (Lb - 50) ** 2))
    assert np.all(want.map[:, :3] == 0) and np.allclose(want.map[:, 3:], closed, atol=1e-6)
    got = U.emulate(w, h, "i420", bits, [1], U.frames_of("i420", [(g, d)], w, h, bits))[0]
    assert U.agrees(got[2], want, U.ATOL, U.RTOL) is None and np.all(got[2][:, :3] == 0)
    assert abs(D.de00(D.lab(126, 128, 128), D.lab(140, 128, 128)) - closed) < 1e-6


def test_colours_that_differ_only_in_chroma_have_no_lightness_term():
    """two Lab colours of one L: dL' = 0 and dE00 does not depend on kL.  (Of Y'CbCr pictures that differ only in Cb / Cr this does NOT
    hold: the sRGB curve makes L depend on the chroma samples.)"""
    a, b = (61.0, 12.0, -7.0), (61.0, -3.0, 22.0)
    de, _, _, dl = R.de00(a, b, parts=True)
    assert dl == 0 and de > 1
    assert D.de00(a, b, (1, 1, 1)) == D.de00(a, b, (0.65, 1, 1)) == D.de00(a, b, (7, 1, 1))
    assert U.kernel_de00(a, b, (1, 1, 1)) == U.kernel_de00(a, b, (0.65, 1, 1))
    assert D.de00(a, b, (1, 1, 1)) != D.de00(a, b, (1, 1, 4))
    ya, yb = D.lab(126, 100, 160), D.lab(126, 160, 100)  # the same luma code, other chroma: L moves
    assert abs(ya[0] - yb[0]) > 0.1


def test_score_and_the_libvmaf_parameters():
    assert D.score(0.0, 100) == 100.0 and D.score(1e-9, 10 ** 6) == 100.0
    assert abs(D.score(250.0, 100) - (45 - 20 * math.log10(2.5))) < 1e-12 and math.isnan(D.score(1.0, 0))
    assert D.score(3.0, 4) == R.score(3.0, 4)
    assert D.K_LIBVMAF == (0.65, 1.0, 4.0) and D.MATRICES == U.MATRIX and D.LAYOUTS == U.LAYOUT == tm.yuv.LAYOUTS
    for m, c in R.MATRIX.items():  # the matrices as the library holds them: one sample triple through each
        assert np.allclose(D.lab(100, 90, 200, m, 8), [float(t) for t in R.lab(100, 90, 200, 8, m)], atol=1e-10)
    assert D.lab(100, 90, 200, "bt709", 8) != D.lab(100, 90, 200, "libvmaf", 8)


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_identical_pictures_give_exactly_zero_and_100(layout, bits):
    for (w, h), kind in (((17, 9), "noise"), ((3, 3), "primaries"), ((U.tile()[0] + 1, 5), "hue_sweep")):
        a, _ = U.pair(w, h, bits, kind, 3)
        fr = U.frames_of(layout, [(a, a)], w, h, bits)  # the two sides differ in the bits the kernel must ignore
        for vec in (None, False):
            s, mx, m = U.emulate(w, h, layout, bits, [1], fr, vec=vec)[0]
            assert s == 0.0 and mx == 0.0 and not m.any()
        assert D.score(s, w * h) == 100.0
        assert R.picture(a, a, bits).de_sum == 0.0


# ---- the emulated kernel against the restatement -----------------------------------------------------------------------------------
_WANT = {}


def want_of(w, h, bits, kind, matrix="bt709", k=(1.0, 1.0, 1.0), seed=0):
    key = (w, h, bits, kind, matrix, k, seed)
    if key not in _WANT:
        pr = U.pair(w, h, bits, kind, seed)
        _WANT[key] = (pr, R.picture(pr[0], pr[1], bits, matrix, k))
    return _WANT[key]


def test_emulation_against_restatement():
    """every shape, layout, depth and kind; prints the measured figures that tests/ciede_util.py records"""
    worst_a = worst_r = worst_m = 0.0
    both = {True: 0, False: 0}
    for (w, h) in U.shapes():
        for layout, bits in U.CASES:
            items = [want_of(w, h, bits, kind) for kind in U.KINDS]
            fr = U.frames_of(layout, [pr for pr, _ in items], w, h, bits, aligned=True)
            got = U.emulate(w, h, layout, bits, [len(items)], fr)
            for kind, (pr, want), (s, mx, m) in zip(U.KINDS, items, got):
                a, r = U.errors(m, want)
                mr = U.mean_rel_map(s, m, want)
                worst_a, worst_r, worst_m = max(worst_a, a), max(worst_r, r), max(worst_m, mr)
                assert U.agrees(m, want, U.ATOL, U.RTOL) is None, (w, h, layout, bits, kind, U.agrees(m, want, U.ATOL, U.RTOL))
                assert mr <= U.MEAN_REL_TOL, (w, h, layout, bits, kind, mr)
                assert abs(mx - float(m.max())) == 0.0 and abs(s - float(m.astype(np.float64).sum())) <= 1e-6 * max(s, 1.0)
                share = float(want.near.mean())
                if kind == "hue_sweep":
                    if w >= 16:
                        assert want.wrapped.any() and (~want.wrapped).any(), (w, h, bits)
                    both[True] += int(want.wrapped.sum()); both[False] += int((~want.wrapped).sum())
                elif w * h >= 1000:
                    assert share <= U.NEAR_SHARE, (w, h, layout, bits, kind, share)
    print(f"measured: atol {worst_a:.3e} (want < 1), rtol {worst_r:.3e} (want >= 1), de_mean rel {worst_m:.3e}")
    assert both[True] and both[False]
    # the recorded figures are what this test measures (to the two digits they are written with)
    assert worst_a <= U.MEASURED_ATOL_CPU and worst_r <= U.MEASURED_RTOL_CPU and worst_m <= U.MEASURED_MEAN_REL_CPU
    assert worst_a >= 0.9 * U.MEASURED_ATOL_CPU and worst_r >= 0.9 * U.MEASURED_RTOL_CPU and worst_m >= 0.9 * U.MEASURED_MEAN_REL_CPU
    assert (U.ATOL, U.RTOL, U.MEAN_REL_TOL) == (4 * U.MEASURED_ATOL_CPU, 4 * U.MEASURED_RTOL_CPU, 4 * U.MEASURED_MEAN_REL_CPU)


@pytest.mark.parametrize("matrix,k", (("bt601", (1.0, 1.0, 1.0)), ("libvmaf", D.K_LIBVMAF), ("bt709", (2.0, 0.5, 1.5))))
def test_matrix_and_factors_reach_the_kernel(matrix, k):
    w, h = 17, 9
    for layout, bits in (("nv12", 8), ("i420", 10)):
        items = [want_of(w, h, bits, kind, matrix, k) for kind in ("noise", "primaries", "hue_sweep")]
        got = U.emulate(w, h, layout, bits, [3], U.frames_of(layout, [pr for pr, _ in items], w, h, bits), matrix=matrix, k=k)
        for (pr, want), (s, mx, m) in zip(items, got):
            assert U.agrees(m, want, U.ATOL, U.RTOL) is None
            other = R.picture(pr[0], pr[1], bits, "bt709", (1.0, 1.0, 1.0))
            assert U.agrees(m, other, U.ATOL, U.RTOL) is not None


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_load_paths_pitches_slots_and_repeats_give_the_same_bits(layout, bits):
    """tight, padded and aligned planes, the wide and the sample-by-sample path, slot positions, batch sizes, a second compute on the
    same buffers: bit for bit the same; garbage in the padding and in the ignored bits changes nothing"""
    tw, th = U.tile()
    for (w, h) in ((17, 9), (tw + 3, 5)):
        pairs = [U.pair(w, h, bits, kind, 5) for kind in ("noise", "hue_sweep", "near_black")]
        tight = U.frames_of(layout, pairs, w, h, bits)
        one = [U.emulate(w, h, layout, bits, [1], [f])[0] for f in tight]

        def same(got):
            return all(a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)) for a, b in zip(got, one))
        assert same(U.emulate(w, h, layout, bits, [3], tight))
        assert same(U.emulate(w, h, layout, bits, [2, 1], tight, cap=5))  # a second compute owes nothing to the first
        assert same(U.emulate(w, h, layout, bits, [3], U.frames_of(layout, pairs, w, h, bits, pad=3, aligned=True)))
        assert same(U.emulate(w, h, layout, bits, [3], U.frames_of(layout, pairs, w, h, bits, pad=5, dirty=False)))
        assert same(U.emulate(w, h, layout, bits, [3], U.frames_of(layout, pairs, w, h, bits, aligned=True), vec=False))
        nomap = U.emulate(w, h, layout, bits, [3], tight, maps=False)
        assert [g[:2] for g in nomap] == [g[:2] for g in one]


def test_nothing_beyond_an_odd_edge_is_read():
    """planes one row and one column larger than the picture, the extra samples garbage: the same bits as the picture alone"""
    w, h = 17, 9
    for layout, bits in (("i420", 8), ("i420", 12), ("i420p10", 10)):
        a, b = U.pair(w, h, bits, "noise", 1)
        big_a, big_b = U.pair(w + 3, h + 3, bits, "noise", 2)
        ch, cw = (h + 1) // 2, (w + 1) // 2
        for big, small in ((big_a, a), (big_b, b)):
            big[0][:h, :w] = small[0]
            big[1][:ch, :cw], big[2][:ch, :cw] = small[1], small[2]
        want = U.emulate(w, h, layout, bits, [1], U.frames_of(layout, [(a, b)], w, h, bits))[0]
        fr = U.frames_of(layout, [(big_a, big_b)], w + 3, h + 3, bits)
        views = [tuple([p[0][:h, :w], p[1][:ch, :cw], p[2][:ch, :cw]] for p in fr[0])]
        got = U.emulate(w, h, layout, bits, [1], views)[0]
        assert got[0] == want[0] and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))


# ---- seeded mistakes -------------------------------------------------------------------------------------------------------------
MISTAKE_PICTURES = (((17, 9), 8, "noise"), ((17, 9), 10, "hue_sweep"), ((17, 9), 10, "near_black"), ((16, 8), 8, "primaries"))
MISTAKE_K = (0.65, 1.0, 4.0)


def _moved(mistake):
    """does the mistake move some position of some small test picture beyond the tolerance?"""
    for (w, h), bits, kind in MISTAKE_PICTURES:
        pr, right = want_of(w, h, bits, kind, "bt709", MISTAKE_K, 9)
        wrong = R.picture(pr[0], pr[1], bits, "bt709", MISTAKE_K, mistake)
        if U.agrees(wrong.map, right, U.ATOL, U.RTOL) is not None:
            return True
    return False


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_seeded_mistakes_are_caught(mistake):
    assert _moved(mistake)


def test_no_mistake_moves_nothing():
    assert len(R.MISTAKES) >= 10 and not _moved(None)


# ---- refusals and ABI ------------------------------------------------------------------------------------------------------------
def _supported(w, h, layout, bits):
    return 2 <= w <= 32768 and 2 <= h <= 32768 and {"nv12": bits == 8, "p016": 9 <= bits <= 16, "i420": 8 <= bits <= 16, "i420p10": bits == 10}[layout]


GEOMS = ((2, 2), (1, 2), (2, 1), (0, 0), (32768, 2), (32769, 2), (2, 32769), (1920, 1080), (0xFFFFFFFF, 0xFFFFFFFF))


def test_create_refuses_before_touching_the_device():
    L = D.lib()
    h = C.c_void_p()
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 12, 16, 17):
            for w, hh in GEOMS:
                ok = _supported(w, hh, layout, bits)
                assert (U.geom(w, hh, layout, bits) is not None) == ok
                if not ok:
                    assert L.tm_ciede_create(C.byref(h), w, hh, U.LAYOUT[layout], bits, 0, 1.0, 1.0, 1.0, 0, 0, 1) == tm.ffi.TM_ERR_UNSUPPORTED, (layout, bits, w, hh)
    U_, I_ = tm.ffi.TM_ERR_UNSUPPORTED, tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_ciede_create(C.byref(h), 16, 16, 4, 8, 0, 1.0, 1.0, 1.0, 0, 0, 1) == U_
    assert L.tm_ciede_create(C.byref(h), 16, 16, 0, 8, 0, 1.0, 1.0, 1.0, 1, 0, 1) == U_  # full range
    assert L.tm_ciede_create(None, 16, 16, 0, 8, 0, 1.0, 1.0, 1.0, 0, 0, 1) == I_
    assert L.tm_ciede_create(C.byref(h), 16, 16, 0, 8, 0, 1.0, 1.0, 1.0, 0, 0, 0) == I_
    assert L.tm_ciede_create(C.byref(h), 16, 16, 0, 8, 0, 1.0, 1.0, 1.0, 0, 0, 65536) == I_
    for m in (-1, 3):
        assert L.tm_ciede_create(C.byref(h), 16, 16, 0, 8, m, 1.0, 1.0, 1.0, 0, 0, 1) == I_
    for k in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0)):
        assert L.tm_ciede_create(C.byref(h), 16, 16, 0, 8, 0, *k, 0, 0, 1) == I_
    assert h.value is None
    out = (C.c_double * 3)()
    assert L.tm_ciede_lab(16, 128, 128, 0, 7, out) == U_ and L.tm_ciede_lab(16, 128, 128, 3, 8, out) == I_ and L.tm_ciede_lab(16, 128, 128, 0, 8, None) == I_


def declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(2) for m in re.finditer(r" ([A-Za-z]) (\S+)", out) if m.group(1) in "TDBRW" and not m.group(2).startswith(("_init", "_fini", "__bss", "_edata", "_end")))


def test_header_is_plain_c99_and_the_library_exports_exactly_it(tmp_path):
    want = declared("turbo_metrics_ciede.h")
    assert len(want) == 11 and all(n.startswith("tm_ciede") for n in want)
    assert exported(DLIB) == want
    assert sorted(D.SYMBOLS) == want
    listed = re.findall(r"^\s*(tm_[a-z0-9_]+);", open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "ciede.map")).read(), flags=re.M)
    assert sorted(listed) == want
    src = tmp_path / "c.c"
    src.write_text('#include "turbo_metrics_ciede.h"\n#include "turbo_metrics_yuv.h"\n#include <stdio.h>\n'
                   "int main(void) { tm_ciede *s = NULL; tm_ciede_frame f; double a[3] = {50, 2.5, 0}, b[3] = {73, 25, -18}; (void)s; (void)f;\n"
                   "  if ((int)TM_CIEDE_NV12 != (int)TM_YUV_NV12 || (int)TM_CIEDE_P016 != (int)TM_YUV_P016 || (int)TM_CIEDE_I420 != (int)TM_YUV_I420 ||\n"
                   "      (int)TM_CIEDE_I420P10_PACKED != (int)TM_YUV_I420P10_PACKED || sizeof f != 40 || TM_CIEDE_LIBVMAF != 2) return 3;\n"
                   "  printf(\"%.4f %.4f\\n\", tm_ciede_de00(a, b, 1, 1, 1), tm_ciede_score(250.0, 100)); return 0; }\n")
    exe = str(tmp_path / "c")
    lib_dir = os.path.dirname(DLIB)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                           "-L" + lib_dir, "-lturbometrics_ciede", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "27.1492 37.0412", (out.returncode, out.stdout, out.stderr)


def test_the_other_libraries_export_nothing_of_it():
    libs = (tm.ffi.SHIP_LIB_PATH, tm.ffi.LIB_PATH, tm.xpsnr.LIB_PATH, tm.motion.LIB_PATH, tm.vif.LIB_PATH, tm.adm.LIB_PATH, tm.scene.LIB_PATH,
            tm.cambi.LIB_PATH, tm.flip.LIB_PATH, tm.yuv.LIB_PATH, tm.hvs.LIB_PATH)
    assert len(set(libs)) == 11
    for lib in libs:
        assert not [n for n in exported(lib) if "tm_ciede" in n], lib


class _FakeLib:
    """stands in for the library under a Ciede object: any call after the plane checks is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_binding_rejects_bad_planes_before_the_library():
    m = tm.Ciede.__new__(tm.Ciede)
    m._L, m._h, m._keep = _FakeLib(), None, {}
    m.w, m.h, m.layout, m.bits, m.batch = 16, 16, "i420", 8, 2
    y, c = np.zeros((16, 16), np.uint8), np.zeros((8, 8), np.uint8)
    for bad in (y.astype(np.uint16), y.astype(np.float32), y[:15], y[:, :15], np.zeros((16, 32), np.uint8)[:, ::2], np.zeros(256, np.uint8), [[0] * 16] * 16,
                y.astype(np.int8)):
        with pytest.raises(ValueError):
            m.set_frame(0, 0, (bad, c, c))
    for bad in (c[:7], c[:, :7], c.astype(np.uint16), np.zeros((8, 16), np.uint8)[:, ::2]):
        with pytest.raises(ValueError):
            m.set_frame(0, 1, (y, bad, c))
        with pytest.raises(ValueError):
            m.set_frame(0, 1, (y, c, bad))
    with pytest.raises(ValueError):
        m.set_frame(0, 0, (y, c))
    m.layout = "nv12"
    with pytest.raises(ValueError):
        m.set_frame(0, 0, (y, c, c))
    with pytest.raises(ValueError):
        m.set_frame(0, 0, (y, c))  # the interleaved plane is 16 elements wide
    assert tm.ciede.Ciede is tm.Ciede and tm.CiedeFrame is D.CiedeFrame


# ---- CLI -------------------------------------------------------------------------------------------------------------------------
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
VALUES = "[possible values: psnr, ssim, msssim, ssimulacra2, xpsnr, vif, adm, cambi, flip, psnr-yuv, ssim-yuv, psnr-hvs, psnr-hvs-m]"


def test_cli_names_the_value_and_refuses_what_it_cannot_do_before_touching_the_device(tmp_path):
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    for p in (a, b):
        with open(p, "wb") as f:
            f.write(b"YUV4MPEG2 W16 H16 F25:1 C420jpeg\nFRAME\n" + bytes(16 * 16 + 2 * 64))

    def run(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)
    out = run("--help")
    assert out.returncode == 0 and all(s in out.stdout for s in ("-m ciede2000 ", "--ciede-libvmaf", "--ciede-map <PREFIX>", "[and: ciede2000]"))
    lines = out.stdout.splitlines()
    at = [i for i, x in enumerate(lines) if x.endswith("vif, adm, cambi, flip, psnr-yuv, ssim-yuv]")]
    assert len(at) == 1 and lines[at[0] + 1].strip() == "[and: psnr-hvs, psnr-hvs-m]" and lines[at[0] + 2].strip() == "[and: ciede2000]"
    for sel in (["-m", "ciede2000"], ["-mciede2000", "-m", "psnr"], ["--metrics", "ciede2000", "--motion"], ["-m", "ciede2000", "--ciede-libvmaf"]):
        for extra in (["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
            out = run(a, b, *sel, *extra)
            assert out.returncode != 0 and "-m ciede2000 does not run with" in out.stderr, (sel, extra, out.returncode, out.stderr)
    # usage errors: exit code 2
    for bad in ("ciede", "ciede-2000", "CIEDE2000", "ciede2000,psnr", "de2000"):
        for form in (["-m", bad], ["-m" + bad], ["--metrics", bad]):
            out = run(a, b, *form)
            assert out.returncode == 2 and f"'{bad}'" in out.stderr, (form, out.returncode, out.stderr)
            assert VALUES in out.stderr and "ciede2000" in out.stderr.split(VALUES)[1]
    for opt in (["--ciede-libvmaf"], ["--ciede-map", str(tmp_path / "m_")]):  # the options belong to -m ciede2000
        out = run(a, b, "-m", "psnr", *opt)
        assert out.returncode == 2 and "ciede2000" in out.stderr, (opt, out.returncode, out.stderr)
    out = run(a, "-m", "ciede2000")  # the distorted argument is still required
    assert out.returncode == 2 and "<DISTORTED>" in out.stderr
