"""PSNR-HVS / PSNR-HVS-M without a GPU: the tables and the float64 restatement (tests/hvs_ref.py), hand values,
the kernel SOURCE run lane by lane on the CPU (tests/hvs_emul) against the restatement with the measured tolerance of
tests/hvs_util.py, seeded mistakes, the library's ABI and refusals, and the CLI's usage."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import hvs_ref as R
from tests import hvs_util as U
from tm_pkg import tm

H = tm.hvs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HLIB = H.LIB_PATH


# ---- tables and the restatement ------------------------------------------------------------------------------------------------
def test_tables_follow_the_quotient_rule_in_all_128_entries():
    q = R.Q
    assert q.shape == (8, 8) and q[0].tolist() == [16, 11, 10, 16, 24, 40, 51, 61] and q[7].tolist() == [72, 92, 95, 98, 112, 100, 103, 99]
    csf = np.array([[round(25.73509 / v, 6) for v in row] for row in q])
    mask = np.array([[round((10.0 / v) ** 2, 6) for v in row] for row in q])
    assert np.array_equal(R.CSF, csf) and np.array_equal(R.MASK, mask)
    assert csf[0].tolist() == [1.608443, 2.339554, 2.573509, 1.608443, 1.072295, 0.643377, 0.504610, 0.421887]
    assert mask[0].tolist() == [0.390625, 0.826446, 1.000000, 0.390625, 0.173611, 0.062500, 0.038447, 0.026874]
    for got in (U.kernel_tables(), H.tables()):  # the kernel source's literals and the library's accessors
        assert got[0].dtype == np.float32 and np.array_equal(got[0], csf.astype(np.float32)) and np.array_equal(got[1], mask.astype(np.float32))
    # the literals as the source spells them: six decimals each
    src = open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "tm_hvs_kernels.h")).read()
    for name, want in (("TMH_CSF_VALUES", csf), ("TMH_MASK_VALUES", mask)):
        body = src.split("#define " + name)[1].split("}")[0]
        lits = re.findall(r"(\d+\.\d+)f", body)
        assert len(lits) == 64 and all(len(x.split(".")[1]) == 6 for x in lits)
        assert [float(x) for x in lits] == want.reshape(-1).tolist()


def test_transform_is_orthonormal_and_the_kernels_factorisation_is_it():
    c = R.C8
    assert np.allclose(c @ c.T, np.eye(8), atol=1e-15)
    assert np.allclose(c[0], math.sqrt(1 / 8)) and np.isclose(c[1, 0], 0.5 * math.cos(math.pi / 16))
    rng = np.random.default_rng(1)
    for x in list(np.eye(8)) + [rng.integers(-255, 256, 8).astype(np.float64) for _ in range(8)]:
        want = c @ x
        want[0] = x.sum()  # the kernel's 8-point pass leaves sqrt(1 / 8) of the DC output to the end of the second pass
        assert np.allclose(U.kernel_dct8(x), want, rtol=0, atol=2e-5 * max(1.0, np.abs(x).max()))


# ---- hand values ---------------------------------------------------------------------------------------------------------------
def _emul1(a, b, layout, bits):
    h, w = a.shape
    (s2, s1, n), = U.emulate(w, h, layout, bits, [1], U.planes_of(layout, [(a, b)], bits))
    return s2, s1, n


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_flat_pictures(layout, bits):
    """only the DC term is non-zero and it is never masked: psnr_hvs = psnr_hvs_m = 20 log10(peak / (1.608443 d))"""
    peak = (1 << bits) - 1
    for w, h, base, d in ((8, 8, 0, 1), (24, 17, peak // 2, 3), (17, 8, peak - 7, 7)):
        a, b = np.full((h, w), base, np.int64), np.full((h, w), base + d, np.int64)
        want = 20 * math.log10(peak / (1.608443 * d))
        r = R.sums(a, b)
        assert abs(R.psnr(r.s_hvs, r.blocks, bits) - want) < 1e-9 and r.s_hvsm == pytest.approx(r.s_hvs, rel=1e-12)
        s2, s1, n = _emul1(a, b, layout, bits)
        assert n == (w // 8) * (h // 8) and s1 == s2  # the same f32 operations on the one non-zero term
        assert abs(H.psnr(s2, n, bits) - want) < 4e-4 and abs(R.psnr(s2, n, bits) - H.psnr(s2, n, bits)) < 1e-12


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_identical_pictures_give_exactly_zero_and_inf(layout, bits):
    a, _ = U.pair(33, 18, bits, "noise", 3)
    assert R.sums(a, a)[:2] == (0.0, 0.0)
    s2, s1, n = _emul1(a, a, layout, bits)
    assert (s2, s1, n) == (0.0, 0.0, 8) and H.psnr(s2, n, bits) == math.inf and R.psnr(s1, n, bits) == math.inf


def test_a_sub_threshold_difference_on_a_textured_block_is_masked_away():
    """A = a full-amplitude checkerboard (0 / 255), B = A with +1 at a dark sample and -1 at a bright one.  The difference
    sums to 0, so the DC term of T(A - B) is 0.  Every |T(A - B)[k][l]| <= sum |C[k][i]| |C[l][j]| |d[i][j]| <= 2 (1/2)(1/2) = 0.5.
    maskeff(A): the AC energy of A is sum (z - mean)^2 = 64 * 127.5^2, so m >= min(MASK) * 64 * 127.5^2 = 0.00683 * 1040400 > 7105; every
    quadrant has the per-sample variance of the block, so pop = (16 / 15) / (64 / 63) = 1.05; maskeff(A) >= sqrt(7105 * 1.05) / 32 > 2.69.
    MASK <= 1, so every threshold M / MASK >= 2.69 > 0.5: S1 is exactly 0 while S2 is not."""
    y, x = np.indices((8, 8))
    a = ((x + y) % 2) * 255
    b = a.copy()
    b[1, 1] += 1
    b[6, 3] -= 1
    assert b.min() == 0 and b.max() == 255 and (a - b).sum() == 0
    r = R.sums(a, b)
    assert r.s_hvsm < 1e-30 and r.s_hvs > 0.01  # float64's C (A - B) C^T leaves a DC term of the size of one rounding; the kernel's is exact
    for layout, bits in (("y8", 8), ("y16_low", 12)):
        s2, s1, _ = _emul1(a, b, layout, bits)
        assert s1 == 0.0 and U.rel_err(s2, r.s_hvs) <= U.REL_TOL
    assert R.maskeff(a[None].astype(np.float64), R.MASK)[0] > 2.69


def test_a_block_of_zero_variance_takes_the_pop_0_branch():
    """A flat: vari(A) = 0, so pop stays 0 and maskeff(A) = 0 (no 0 / 0); M is maskeff(B) alone"""
    a = np.full((8, 8), 100, np.int64)
    b = a.copy()
    b[2:5, 3:7] += np.arange(12).reshape(3, 4)
    assert R.maskeff(a[None].astype(np.float64), R.MASK)[0] == 0.0 and R.maskeff(b[None].astype(np.float64), R.MASK)[0] > 0
    r = R.sums(a, b)
    assert math.isfinite(r.s_hvs) and 0 < r.s_hvsm < r.s_hvs
    for x, y in ((a, b), (b, a)):
        s2, s1, _ = _emul1(x, y, "y8", 8)
        assert U.rel_err(s2, r.s_hvs) <= U.REL_TOL and U.rel_err(s1, r.s_hvsm) <= U.REL_TOL


def test_host_functions():
    assert H.psnr(0.0, 4, 8) == math.inf and math.isnan(H.psnr(1.0, 0, 8)) and math.isnan(H.psnr(1.0, 1, 7)) and math.isnan(H.psnr(1.0, 1, 17))
    assert H.psnr(255.0 ** 2 * 64 * 3, 3, 8) == 0.0
    assert abs(H.psnr(64.0 * 5, 5, 10) - 20 * math.log10(1023)) < 1e-12
    # a sequence: the summed S over the summed Num
    assert H.psnr(3.0 + 5.0, 4 + 4, 8) == R.psnr(8.0, 8, 8)


# ---- the kernel source against the restatement -----------------------------------------------------------------------------------
def test_emulation_against_restatement(capsys):
    """every shape, layout / depth and kind, several slots per compute on reused buffers, both load paths.  Prints the largest relative
    error of S2 and of S1: hvs_util.REL_TOL is that figure times 4 and may not exceed 1e-4."""
    worst = [0.0, 0.0]
    for w, h in U.shapes():
        for layout, bits in U.CASES:
            pairs = [U.pair(w, h, bits, k) for k in U.KINDS]
            for aligned in (False, True):
                frames = U.planes_of(layout, pairs, bits, pad=0 if aligned else 3, aligned=aligned)
                got = U.emulate(w, h, layout, bits, [3, len(pairs) - 3], frames, cap=4)
                for kind, (a, b), g in zip(U.KINDS, pairs, got):
                    want = R.sums(a, b)
                    assert g[2] == want.blocks == (w // 8) * (h // 8)
                    e = (U.rel_err(g[0], want.s_hvs), U.rel_err(g[1], want.s_hvsm))
                    assert max(e) <= U.REL_TOL, (w, h, layout, bits, kind, aligned, e)
                    worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    with capsys.disabled():
        print(f"\nPSNR-HVS emulation against restatement: largest relative error S2 {worst[0]:.3g}, S1 {worst[1]:.3g}; tolerance {U.REL_TOL:.3g}")
    assert max(worst) <= U.MEASURED_REL * 1.0001 and U.REL_TOL == 4 * U.MEASURED_REL <= 1e-4


def test_load_paths_slots_and_repeats_give_the_same_bits():
    w, h = U.shapes()[-1]
    for layout, bits in U.CASES:
        pairs = [U.pair(w, h, bits, k, seed=5) for k in ("noise", "quadrant", "near_peak")]
        tight = U.planes_of(layout, pairs, bits)
        one = [U.emulate(w, h, layout, bits, [1], [f])[0] for f in tight]
        assert U.emulate(w, h, layout, bits, [3], tight) == one
        assert U.emulate(w, h, layout, bits, [2, 1], tight, cap=5) == one  # a second compute owes nothing to the first
        assert U.emulate(w, h, layout, bits, [3], U.planes_of(layout, pairs, bits, pad=2, aligned=True)) == one
        assert U.emulate(w, h, layout, bits, [3], tight, vec=False) == one


def test_the_remainder_is_never_read():
    """garbage in the columns and rows beyond the last block changes nothing"""
    w, h = 23, 15
    a, b = U.pair(w, h, 8, "noise", 2)
    a2, b2 = a.copy(), b.copy()
    a2[:, 16:] = 255 - a2[:, 16:]
    b2[8:, :] = 7
    one = U.emulate(w, h, "y8", 8, [1], U.planes_of("y8", [(a, b)], 8))
    assert U.emulate(w, h, "y8", 8, [1], U.planes_of("y8", [(a2, b2)], 8)) == one
    assert one[0][2] == 2 and R.sums(a2, b2) == R.sums(a, b)


# ---- seeded mistakes -------------------------------------------------------------------------------------------------------------
def _moved(mistake):
    """does the mistake move S2 or S1 of some test picture beyond the tolerance?"""
    for (w, h), bits, kind in (((15, 9), 8, "noise"), ((24, 16), 8, "flat_noise"), ((24, 16), 10, "quadrant"), ((24, 16), 8, "noise")):
        a, b = U.pair(w, h, bits, kind, seed=9)
        right, wrong = R.sums(a, b), R.sums(a, b, mistake)
        if right.blocks != wrong.blocks or U.rel_err(wrong.s_hvs, right.s_hvs) > U.REL_TOL or U.rel_err(wrong.s_hvsm, right.s_hvsm) > U.REL_TOL:
            return True
    return False


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_seeded_mistakes_are_caught(mistake):
    assert _moved(mistake)


def test_no_mistake_moves_nothing():
    assert not _moved(None)


# ---- refusals and ABI ------------------------------------------------------------------------------------------------------------
def _supported(w, h, layout, bits):
    return 8 <= w <= 32768 and 8 <= h <= 32768 and {"y8": bits == 8, "y16_msb": 9 <= bits <= 16, "y16_low": 9 <= bits <= 16, "y10_packed": bits == 10}[layout]


GEOMS = ((8, 8), (7, 8), (8, 7), (0, 0), (32768, 8), (32769, 8), (8, 32769), (1920, 1080))


def test_create_refuses_before_touching_the_device():
    L = H.lib()
    h = C.c_void_p()
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 12, 16, 17):
            for w, hh in GEOMS + ((0xFFFFFFFF, 0xFFFFFFFF),):
                ok = _supported(w, hh, layout, bits)
                assert (U.geom(w, hh, layout, bits) is not None) == ok
                if not ok:
                    assert L.tm_hvs_create(C.byref(h), w, hh, U.LAYOUT[layout], bits, 1) == tm.ffi.TM_ERR_UNSUPPORTED, (layout, bits, w, hh)
    assert L.tm_hvs_create(C.byref(h), 16, 16, 4, 8, 1) == tm.ffi.TM_ERR_UNSUPPORTED
    assert L.tm_hvs_create(None, 16, 16, 0, 8, 1) == tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_hvs_create(C.byref(h), 16, 16, 0, 8, 0) == tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_hvs_create(C.byref(h), 16, 16, 0, 8, 65536) == tm.ffi.TM_ERR_INVALID_ARG
    assert h.value is None


def declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(2) for m in re.finditer(r" ([A-Za-z]) (\S+)", out) if m.group(1) in "TDBRW" and not m.group(2).startswith(("_init", "_fini", "__bss", "_edata", "_end")))


def test_header_is_plain_c99_and_the_library_exports_exactly_it(tmp_path):
    want = declared("turbo_metrics_hvs.h")
    assert len(want) == 10 and all(n.startswith("tm_hvs") for n in want)
    assert exported(HLIB) == want
    assert sorted(H.SYMBOLS) == want
    listed = re.findall(r"^\s*(tm_[a-z0-9_]+);", open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "hvs.map")).read(), flags=re.M)
    assert sorted(listed) == want
    assert H.LAYOUTS == tm.vif.LAYOUTS == U.LAYOUT
    src = tmp_path / "c.c"
    src.write_text('#include "turbo_metrics_hvs.h"\n#include "turbo_metrics_vif.h"\n#include <stdio.h>\n'
                   "int main(void) { tm_hvs *s = NULL; tm_hvs_frame f; (void)s; (void)f;\n"
                   "  if ((int)TM_HVS_Y8 != (int)TM_VIF_Y8 || (int)TM_HVS_Y16_MSB != (int)TM_VIF_Y16_MSB || (int)TM_HVS_Y16_LOW != (int)TM_VIF_Y16_LOW ||\n"
                   "      (int)TM_HVS_Y10_PACKED != (int)TM_VIF_Y10_PACKED || sizeof f != 24) return 3;\n"
                   "  printf(\"%.4f %.6f %.6f\\n\", tm_hvs_psnr(64.0, 1, 8), (double)tm_hvs_csf()[1], (double)tm_hvs_mask()[63]); return 0; }\n")
    exe = str(tmp_path / "c")
    lib_dir = os.path.dirname(HLIB)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                           "-L" + lib_dir, "-lturbometrics_hvs", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "48.1308 2.339554 0.010203", (out.returncode, out.stdout, out.stderr)


def test_the_other_libraries_export_nothing_of_it():
    for lib in (tm.ffi.SHIP_LIB_PATH, tm.ffi.LIB_PATH, tm.xpsnr.LIB_PATH, tm.motion.LIB_PATH, tm.vif.LIB_PATH, tm.adm.LIB_PATH, tm.scene.LIB_PATH,
                tm.cambi.LIB_PATH, tm.flip.LIB_PATH, tm.yuv.LIB_PATH):
        assert not [n for n in exported(lib) if "tm_hvs" in n], lib


class _FakeLib:
    """stands in for the library under an Hvs object: any call after the plane checks is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_binding_rejects_bad_planes_before_the_library():
    m = tm.Hvs.__new__(tm.Hvs)
    m._L, m._h, m._keep = _FakeLib(), None, {}
    m.w, m.h, m.layout, m.bits, m.batch = 16, 16, "y8", 8, 2
    y = np.zeros((16, 16), np.uint8)
    for bad in (y.astype(np.uint16), y.astype(np.float32), y[:15], y[:, :15], np.zeros((16, 32), np.uint8)[:, ::2], np.zeros(256, np.uint8), [[0] * 16] * 16,
                y.astype(np.int8)):
        with pytest.raises(ValueError):
            m.set_pair(0, y, bad)
        with pytest.raises(ValueError):
            m.set_pair(0, bad, y)
    with pytest.raises(ValueError):
        m.set_pair(2, y, y)
    assert tm.hvs.Hvs is tm.Hvs and tm.HvsFrame is H.HvsFrame


# ---- CLI -------------------------------------------------------------------------------------------------------------------------
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
VALUES = "possible values: psnr, ssim, msssim, ssimulacra2, xpsnr, vif, adm, cambi, flip, psnr-yuv, ssim-yuv"


def test_cli_names_the_values_and_refuses_what_it_cannot_do_before_touching_the_device(tmp_path):
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    for p in (a, b):
        with open(p, "wb") as f:
            f.write(b"YUV4MPEG2 W16 H16 F25:1 C420jpeg\nFRAME\n" + bytes(16 * 16 + 2 * 64))

    def run(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)
    out = run("--help")
    assert out.returncode == 0 and all(s in out.stdout for s in ("-m psnr-hvs ", "-m psnr-hvs-m ", "[and: psnr-hvs, psnr-hvs-m]"))
    lines = out.stdout.splitlines()
    at = [i for i, x in enumerate(lines) if x.endswith("vif, adm, cambi, flip, psnr-yuv, ssim-yuv]")]
    assert len(at) == 1 and "psnr-hvs, psnr-hvs-m" in lines[at[0] + 1]  # the pinned line stays, the new values are named below it
    for sel in (["-m", "psnr-hvs"], ["-m", "psnr-hvs-m"], ["-mpsnr-hvs", "-m", "psnr-hvs-m", "-m", "psnr"], ["--metrics", "psnr-hvs-m", "--motion"]):
        for extra in (["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
            out = run(a, b, *sel, *extra)
            assert out.returncode != 0 and "-m psnr-hvs / psnr-hvs-m do not run with" in out.stderr, (sel, extra, out.returncode, out.stderr)
    # usage errors: exit code 2
    for bad in ("psnr_hvs", "hvs", "psnr-hvs,psnr-hvs-m", "PSNR-HVS", "psnr-hvsm"):
        for form in (["-m", bad], ["-m" + bad], ["--metrics", bad]):
            out = run(a, b, *form)
            assert out.returncode == 2 and f"'{bad}'" in out.stderr, (form, out.returncode, out.stderr)
            assert "[" + VALUES + ", psnr-hvs, psnr-hvs-m]" in out.stderr
    out = run(a, "-m", "psnr-hvs")  # the distorted argument is still required
    assert out.returncode == 2 and "<DISTORTED>" in out.stderr
