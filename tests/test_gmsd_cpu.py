"""GMSD without a GPU: the float64 restatement in the paper's form (tests/gmsd_ref.py), hand values derived on paper,
the kernel SOURCE run lane by lane on the CPU (tests/gmsd_emul) against the restatement with the measured tolerance of
tests/gmsd_util.py, seeded mistakes, the library's ABI and refusals, the binding's plane checks and the CLI's usage."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gmsd_ref as R
from tests import gmsd_util as U
from tm_pkg import tm

G = tm.gmsd
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLIB = G.LIB_PATH


def _emul1(a, b, layout, bits, maps=False, pad=0):
    h, w = a.shape
    out = U.emulate(w, h, layout, bits, [1], U.planes_of(layout, [(a, b)], bits, pad=pad), maps=maps)
    return (out[0][0], out[1][0]) if maps else out[0]


# ---- hand values ---------------------------------------------------------------------------------------------------------------
def test_the_restatements_convolution_is_matlabs_same():
    a = np.arange(12, dtype=np.float64).reshape(3, 4)
    # conv2(a, ones(2), 'same'): out(i, j) = a(i, j) + a(i, j+1) + a(i+1, j) + a(i+1, j+1), zeros beyond the end
    assert R.conv2_same(a, np.ones((2, 2))).tolist() == [[10, 14, 18, 10], [26, 30, 34, 18], [17, 19, 21, 11]]
    # conv2 flips the kernel: [1 0 -1] gives a(j+1) - a(j-1)
    assert R.conv2_same(a, np.array([[1.0, 0.0, -1.0]])).tolist() == [[1, 2, 2, -2], [5, 2, 2, -6], [9, 2, 2, -10]]


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_identical_pictures_give_exactly_zero(layout, bits):
    a, _ = U.pair(33, 19, bits, "noise", 3)
    r = R.gmsd(a, a, bits)
    assert r.gmsd == 0.0 and r.gmsm == 1.0
    e1, e2, mx, n = _emul1(a, a, layout, bits)
    assert (e1, e2, mx, n) == (0.0, 0.0, 0.0, 17 * 10) and G.score(e1, e2, n) == 0.0 and G.mean(e1, n) == 1.0


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_zero_against_a_flat_4x4_picture(layout, bits):
    """R = 0, D = v everywhere, 4 x 4: the decimated plane is 2 x 2 with S = 4 v; at each of the four positions one horizontal and one
    vertical neighbour pair lies inside, so |gx| = |gy| = 8 v and A_d = 128 v^2, A_r = 0: e = 128 v^2 / (128 v^2 + 24480) at all four,
    gmsd = 0, gmsm = 1 - e.  At depth b the same content is v * 2^(b - 8) and C grows by 4^(b - 8): the same e to the f32 rounding."""
    k = 1 << (bits - 8)
    for v in (1, 7, 100, 255):
        e = 128.0 * v * v / (128.0 * v * v + 24480.0)
        a, b = np.zeros((4, 4), np.int64), np.full((4, 4), v * k, np.int64)
        r = R.gmsd(a, b, bits)
        assert r.n == 4 and abs(r.gmsd) < 1e-15 and abs(r.gmsm - (1 - e)) < 1e-15
        for x, y in ((a, b), (b, a)):
            (e1, e2, mx, n), m = _emul1(x, y, layout, bits, maps=True)
            assert n == 4 and abs(mx - e) < 1e-6 and e1 == 4 * mx and e2 == 4 * mx * mx  # four equal f32 values, added exactly
            assert G.score(e1, e2, n) == 0.0 and G.score(e1, e2, n, True) == 0.0 and abs(G.mean(e1, n) - (1 - e)) < 1e-6
            assert (m == np.float32(1.0) - np.float32(mx)).all()
            assert mx == U.kernel_e(128 * (v * k) ** 2, 0, 24480 * k * k) == U.kernel_e(0, 128 * (v * k) ** 2, 24480 * k * k)
        if bits > 8:  # the 8-bit value of the same content: equal bits, the scaling is by powers of two throughout
            assert mx == U.kernel_e(128 * v * v, 0, 24480)


def test_an_odd_sized_picture_takes_zeros_beyond_its_edges():
    """5 x 7, R = 0, D = 60 everywhere: w2 = 3, h2 = 4.  S = 240 where the 2 x 2 cell lies inside, 120 in column 2 (sample column 5 is 0)
    and in row 3 (sample row 7 is 0), 60 at their crossing.  Position (0, 0): gx = S(0, 1) + S(1, 1) = 480 = gy, A = 2 * 480^2.  Position
    (3, 2), the crossing: gx = -(S(2, 1) + S(3, 1)) = -360, gy = -(S(2, 1) + S(2, 2)) = -360, A = 2 * 360^2.  Position (1, 1), inside:
    gx = (120 - 240) * 3 = -360, gy = 0, A = 360^2."""
    a, b = np.zeros((7, 5), np.int64), np.full((7, 5), 60, np.int64)
    want = {(0, 0): 2 * 480 ** 2, (3, 2): 2 * 360 ** 2, (1, 1): 360 ** 2}
    r = R.gmsd(a, b, 8)
    assert r.n == 12
    (e1, e2, mx, n), m = _emul1(a, b, "y8", 8, maps=True, pad=3)  # garbage right behind each row
    assert n == 12 and m.shape == (4, 3)
    for (y, x), A in want.items():
        assert abs(r.gms[y, x] - 24480.0 / (A + 24480.0)) < 1e-15  # (2 * 0 * m_d + c) / (m_d^2 + c), A = 144 m_d^2 on 9 * 16 c
        assert m[y, x] == np.float32(1.0) - np.float32(U.kernel_e(0, A, 24480))
    assert abs(G.score(e1, e2, n) - r.gmsd) <= U.ABS_TOL and abs(G.mean(e1, n) - r.gmsm) <= U.ABS_TOL
    assert abs(R.gmsd(a, b, 8, "byte_behind").gmsd - r.gmsd) > 1e-3 and abs(R.gmsd(a, b, 8, "replicate").gmsd - r.gmsd) > 1e-3


def test_host_functions():
    assert math.isnan(G.score(1.0, 1.0, 1)) and math.isnan(G.score(0.0, 0.0, 0)) and math.isnan(G.mean(1.0, 1)) and math.isnan(G.mean(0.0, 0))
    assert G.score(1.0, 1.0, 2) == math.sqrt(0.5) and G.score(1.0, 1.0, 2, True) == 0.5 and G.mean(1.0, 2) == 0.5
    assert G.score(2.0, 0.999999, 4) == 0.0  # a radicand that rounding left below zero
    rng = np.random.default_rng(5)
    e = rng.random(1000) * 0.3
    for pop in (False, True):
        assert abs(G.score(e.sum(), (e * e).sum(), e.size, pop) - np.std(e, ddof=0 if pop else 1)) < 1e-12
        assert G.score(e.sum(), (e * e).sum(), e.size, pop) == U.score(float(e.sum()), float((e * e).sum()), e.size, pop) == R.score(float(e.sum()), float((e * e).sum()), e.size, pop)
    # a sequence: the same functions of the summed sums = pooled over all positions
    refs = [R.gmsd(*U.pair(21, 14, 8, "blur", s), 8) for s in range(3)]
    e1 = sum(float((1 - r.gms).sum()) for r in refs)
    e2 = sum(float(((1 - r.gms) ** 2).sum()) for r in refs)
    n = sum(r.n for r in refs)
    pg, pm = R.pooled(refs)
    assert abs(G.score(e1, e2, n) - pg) < 1e-12 and abs(G.mean(e1, n) - pm) < 1e-12


# ---- the kernel source against the restatement -----------------------------------------------------------------------------------
def test_emulation_against_restatement(capsys):
    """every shape, layout / depth and kind, several slots per compute on reused buffers, both load paths.  Prints the largest absolute
    error of gmsd and of gmsm: gmsd_util.ABS_TOL is that figure times 4, and the figure may not exceed 1e-5."""
    worst = [0.0, 0.0]
    for w, h in U.shapes():
        for layout, bits in U.CASES:
            pairs = [U.pair(w, h, bits, k) for k in U.KINDS]
            for aligned in (False, True):
                frames = U.planes_of(layout, pairs, bits, pad=0 if aligned else 3, aligned=aligned)
                got = U.emulate(w, h, layout, bits, [3, len(pairs) - 3], frames, cap=4)
                for kind, (a, b), g in zip(U.KINDS, pairs, got):
                    want = R.gmsd(a, b, bits)
                    assert g[3] == want.n == ((w + 1) // 2) * ((h + 1) // 2)
                    e = (abs(U.score(g[0], g[1], g[3]) - want.gmsd), abs(U.mean(g[0], g[3]) - want.gmsm))
                    assert max(e) <= U.ABS_TOL, (w, h, layout, bits, kind, aligned, e)
                    if kind == "identical":  # where the exact value is 0 the kernel gives exactly 0
                        assert g[:3] == (0.0, 0.0, 0.0)
                    worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    with capsys.disabled():
        print(f"\nGMSD emulation against restatement: largest absolute error gmsd {worst[0]:.3g}, gmsm {worst[1]:.3g}; tolerance {U.ABS_TOL:.3g}")
    assert max(worst) <= U.MEASURED_ABS * 1.0001 and U.ABS_TOL == 4 * U.MEASURED_ABS and U.MEASURED_ABS <= 1e-5


def test_the_map_is_one_minus_e_at_every_position():
    w, h = U.shapes()[5]
    for layout, bits in (("y8", 8), ("y16_low", 12), ("y10_packed", 10)):
        pairs = [U.pair(w, h, bits, k, seed=2) for k in ("noise", "blur")]
        got, maps = U.emulate(w, h, layout, bits, [2], U.planes_of(layout, pairs, bits), maps=True)
        assert U.emulate(w, h, layout, bits, [2], U.planes_of(layout, pairs, bits)) == got  # the sums with maps on and off
        for (a, b), g, m in zip(pairs, got, maps):
            want = R.gmsd(a, b, bits)
            assert m.shape == want.gms.shape and np.abs(m.astype(np.float64) - want.gms).max() < 2e-7  # f32: half an ulp of 1 from 1 - e, and e's own error
            assert abs((1.0 - m.astype(np.float64)).max() - g[2]) < 1e-7


def test_load_paths_slots_and_repeats_give_the_same_bits():
    w, h = U.shapes()[-1]
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
def _moved(mistake):
    """does the mistake move gmsd or gmsm of some test picture beyond the tolerance?"""
    tw, th = U.tile()
    for (w, h), bits, kind in (((5, 7), 8, "noise"), ((24, 16), 8, "blur"), ((24, 16), 10, "blur"), ((4 * tw + 1, 9), 8, "noise")):
        a, b = U.pair(w, h, bits, kind, seed=9)
        right, wrong = R.gmsd(a, b, bits, tile=(tw, th)), R.gmsd(a, b, bits, mistake, tile=(tw, th))
        if right.n != wrong.n or abs(wrong.gmsd - right.gmsd) > U.ABS_TOL or abs(wrong.gmsm - right.gmsm) > U.ABS_TOL:
            return True
    return False


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_seeded_mistakes_are_caught(mistake):
    assert _moved(mistake)


def test_no_mistake_moves_nothing():
    assert not _moved(None)


def test_the_emulation_agrees_where_each_mistake_bites():
    """the pictures of _moved: the kernel source is on the right side of every seeded mistake"""
    tw, th = U.tile()
    for (w, h), bits, kind in (((5, 7), 8, "noise"), ((24, 16), 10, "blur"), ((4 * tw + 1, 9), 8, "noise")):
        a, b = U.pair(w, h, bits, kind, seed=9)
        layout = "y8" if bits == 8 else "y16_msb"
        e1, e2, _, n = _emul1(a, b, layout, bits, pad=1)
        want = R.gmsd(a, b, bits)
        assert abs(U.score(e1, e2, n) - want.gmsd) <= U.ABS_TOL and abs(U.mean(e1, n) - want.gmsm) <= U.ABS_TOL


# ---- refusals and ABI ------------------------------------------------------------------------------------------------------------
def _supported(w, h, layout, bits):
    return 4 <= w <= 32768 and 4 <= h <= 32768 and {"y8": bits == 8, "y16_msb": 9 <= bits <= 16, "y16_low": 9 <= bits <= 16, "y10_packed": bits == 10}[layout]


GEOMS = ((4, 4), (3, 4), (4, 3), (0, 0), (32768, 4), (32769, 4), (4, 32769), (1920, 1080))


def test_create_refuses_before_touching_the_device():
    L = G.lib()
    h = C.c_void_p()
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 12, 16, 17):
            for w, hh in GEOMS + ((0xFFFFFFFF, 0xFFFFFFFF),):
                ok = _supported(w, hh, layout, bits)
                assert (U.geom(w, hh, layout, bits) is not None) == ok
                if not ok:
                    for flags in (0, G.TM_GMSD_MAPS):
                        assert L.tm_gmsd_create(C.byref(h), w, hh, U.LAYOUT[layout], bits, 1, flags) == tm.ffi.TM_ERR_UNSUPPORTED, (layout, bits, w, hh)
    assert L.tm_gmsd_create(C.byref(h), 16, 16, 4, 8, 1, 0) == tm.ffi.TM_ERR_UNSUPPORTED
    assert L.tm_gmsd_create(None, 16, 16, 0, 8, 1, 0) == tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_gmsd_create(C.byref(h), 16, 16, 0, 8, 0, 0) == tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_gmsd_create(C.byref(h), 16, 16, 0, 8, 65536, 0) == tm.ffi.TM_ERR_INVALID_ARG
    assert h.value is None
    # C at every depth: 170 * 144 * 4^(b - 8)
    for bits in range(9, 17):
        assert U.geom(64, 64, "y16_low", bits)[3] == 170 * 144 * 4 ** (bits - 8)
    assert U.geom(64, 64, "y8", 8) == (32, 32, 1, 24480) and U.geom(5, 7, "y8", 8)[:2] == (3, 4)


def declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(2) for m in re.finditer(r" ([A-Za-z]) (\S+)", out) if m.group(1) in "TDBRW" and not m.group(2).startswith(("_init", "_fini", "__bss", "_edata", "_end")))


def test_header_is_plain_c99_and_the_library_exports_exactly_it(tmp_path):
    want = declared("turbo_metrics_gmsd.h")
    assert len(want) == 10 and all(n.startswith("tm_gmsd") for n in want)
    assert exported(GLIB) == want
    assert sorted(G.SYMBOLS) == want
    listed = re.findall(r"^\s*(tm_[a-z0-9_]+);", open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "gmsd.map")).read(), flags=re.M)
    assert sorted(listed) == want
    assert G.LAYOUTS == tm.hvs.LAYOUTS == U.LAYOUT
    src = tmp_path / "c.c"
    src.write_text('#include "turbo_metrics_gmsd.h"\n#include "turbo_metrics_hvs.h"\n#include <stdio.h>\n'
                   "int main(void) { tm_gmsd *s = NULL; tm_gmsd_frame f; (void)s; (void)f;\n"
                   "  if ((int)TM_GMSD_Y8 != (int)TM_HVS_Y8 || (int)TM_GMSD_Y16_MSB != (int)TM_HVS_Y16_MSB || (int)TM_GMSD_Y16_LOW != (int)TM_HVS_Y16_LOW ||\n"
                   "      (int)TM_GMSD_Y10_PACKED != (int)TM_HVS_Y10_PACKED || TM_GMSD_MAPS != 1 || sizeof f != 32) return 3;\n"
                   "  printf(\"%.6f %.6f %.2f\\n\", tm_gmsd_score(1.0, 1.0, 2, 0), tm_gmsd_score(1.0, 1.0, 2, 1), tm_gmsd_mean(1.0, 4)); return 0; }\n")
    exe = str(tmp_path / "c")
    lib_dir = os.path.dirname(GLIB)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                           "-L" + lib_dir, "-lturbometrics_gmsd", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "0.707107 0.500000 0.75", (out.returncode, out.stdout, out.stderr)
    assert C.sizeof(G.GmsdFrameC) == 32


def test_the_other_libraries_export_nothing_of_it():
    for lib in (tm.ffi.SHIP_LIB_PATH, tm.ffi.LIB_PATH, tm.xpsnr.LIB_PATH, tm.motion.LIB_PATH, tm.vif.LIB_PATH, tm.adm.LIB_PATH, tm.scene.LIB_PATH,
                tm.cambi.LIB_PATH, tm.flip.LIB_PATH, tm.yuv.LIB_PATH, tm.hvs.LIB_PATH, tm.ciede.LIB_PATH, tm.siti.LIB_PATH):
        assert not [n for n in exported(lib) if "tm_gmsd" in n], lib


def test_the_kernel_source_keeps_to_plain_stores_and_no_atomics():
    src = open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "tm_gmsd_kernels.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code.lower() and "asm" not in code and "hipMemset" not in open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "tm_gmsd.hip")).read()


class _FakeLib:
    """stands in for the library under a Gmsd object: any call after the plane checks is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_binding_rejects_bad_planes_before_the_library():
    m = tm.Gmsd.__new__(tm.Gmsd)
    m._L, m._h, m._keep = _FakeLib(), None, {}
    m.w, m.h, m.layout, m.bits, m.batch, m.maps, m.population = 16, 16, "y8", 8, 2, True, False
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
    assert tm.gmsd.Gmsd is tm.Gmsd and tm.GmsdFrame is G.GmsdFrame and G.GmsdFrame._fields == ("e1", "e2", "e_max", "n", "gmsd", "gmsm")


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
    assert out.returncode == 0 and all(s in out.stdout for s in ("-m gmsd ", "--gmsd-population ", "--gmsd-map <PREFIX>", "[and: gmsd]"))
    lines = out.stdout.splitlines()
    at = [i for i, x in enumerate(lines) if x.endswith("[possible values: psnr, ssim, msssim, ssimulacra2, xpsnr]")]
    assert len(at) == 1  # the earlier lines stay byte for byte, gmsd goes on a further line below them
    assert [x.strip() for x in lines[at[0] + 1:at[0] + 5]] == ["[further values, each described below: vif, adm, cambi, flip, psnr-yuv, ssim-yuv]", "[and: psnr-hvs, psnr-hvs-m]",
                                                               "[and: ciede2000]", "[and: gmsd]"]
    for sel in (["-m", "gmsd"], ["-mgmsd", "-m", "psnr"], ["--metrics", "gmsd", "--motion"], ["-m", "gmsd", "--gmsd-population", "--gmsd-map", str(tmp_path / "m")]):
        for extra in (["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
            out = run(a, b, *sel, *extra)
            assert out.returncode != 0 and out.returncode != 2 and "-m gmsd does not run with" in out.stderr, (sel, extra, out.returncode, out.stderr)
    assert not list(tmp_path.glob("m*.pfm"))
    # usage errors: exit code 2
    for bad in ("GMSD", "gmsm", "gmsd,psnr", "gms"):
        for form in (["-m", bad], ["-m" + bad], ["--metrics", bad]):
            out = run(a, b, *form)
            assert out.returncode == 2 and f"'{bad}'" in out.stderr, (form, out.returncode, out.stderr)
            assert "[" + VALUES + ", psnr-hvs, psnr-hvs-m] [and: ciede2000] [and: gmsd]" in out.stderr
    for opts in (["--gmsd-population"], ["--gmsd-map", "x"], ["--gmsd-map=x", "-m", "psnr"], ["--gmsd-population", "--siti"]):
        out = run(a, b, *opts)
        assert out.returncode == 2 and "belong to '-m gmsd'" in out.stderr, (opts, out.returncode, out.stderr)
    out = run(a, b, "-m", "gmsd", "--gmsd-map")
    assert out.returncode == 2 and "--gmsd-map <PREFIX>" in out.stderr
    out = run(a, "-m", "gmsd")  # the distorted argument is still required
    assert out.returncode == 2 and "<DISTORTED>" in out.stderr
