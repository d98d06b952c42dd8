"""CPU tier of dE ITP: the printed values of BT.2100 / BT.2408 (tests/golden/itp_pins.json) on the library's
double functions, the float64 restatement and the device's f32 stages; the device's log2 / exp2 / pow against float64; the kernel source
run on the CPU (tests/itp_emul) against the restatement over every layout, depth, transfer, shape and picture kind, with the measured
tolerance and its condition; hand values; seeded mistakes; load paths; refusals; the ABI; the binding's plane checks; the CLI's usage."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import itp_ref as R
from tests import itp_util as U
from tm_pkg import tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = tm.itp
DLIB = D.LIB_PATH
TRANSFERS = ("pq", "hlg")

_WANT = {}


def want_of(w, h, bits, kind, transfer, seed):
    """(the pair, its restatement), computed once"""
    key = (w, h, bits, kind, transfer, seed)
    if key not in _WANT:
        pr = U.pair(w, h, bits, kind, seed=seed)
        _WANT[key] = (pr, R.picture(pr[0], pr[1], bits, transfer))
    return _WANT[key]


# ---- pins ------------------------------------------------------------------------------------------------------------------------
def test_printed_values_of_bt2100_and_bt2408():
    """the double functions, the restatement and the device's f32 stages within half a unit of the last printed digit"""
    P = U.pins()
    for light, signal in P["pq_inverse_eotf"]:
        for got in (D.pq_inv_eotf(light), float(R.pq_inv_eotf(light)), float(U.kernel_pq_inv([light])[0])):
            assert abs(got - signal) <= U.PIN_SIGNAL_TOL, (light, got)
        for got in (D.pq_eotf(D.pq_inv_eotf(light)), float(R.pq_eotf(R.pq_inv_eotf(light))), float(U.kernel_pq_eotf(U.kernel_pq_inv([light]))[0])):
            assert abs(got - light) <= 1e-3 * light, (light, got)  # the round trip; f32: the signal's half ulp times the curve's slope
    assert D.pq_eotf(1.0) == 10000.0 and D.pq_eotf(0.0) == 0.0 and U.kernel_pq_eotf([0.0, 1.0]).tolist() == [0.0, 10000.0]
    for signal, scene in P["hlg_scene"]:
        assert abs(float(R.hlg_scene(signal)) - scene) < 1e-15
    for signal, light in P["hlg_display_grey"]:
        for got in (D.hlg_display([signal] * 3), [float(t) for t in R.hlg_display([np.float64(signal)] * 3)], U.kernel_hlg_display([signal] * 3).tolist()):
            assert all(abs(g - light) <= U.PIN_LIGHT_TOL for g in got), (signal, got)
    assert D.hlg_display([0, 0, 0]) == (0.0, 0.0, 0.0) and U.kernel_hlg_display([0, 0, 0]).tolist() == [0.0, 0.0, 0.0]
    # the matrices: exact integers
    assert P["lms_rows"] == R.LMS.astype(int).tolist() and all(sum(r) == P["lms_row_sum"] == 4096 for r in P["lms_rows"])
    assert P["ctcp_rows"] == R.ICTCP[1:].astype(int).tolist() and all(sum(r) == P["ctcp_row_sum"] == 0 for r in P["ctcp_rows"])
    assert R.ICTCP[0].tolist() == [2048, 2048, 0]


def test_double_functions_are_the_restatement():
    rng = np.random.default_rng(5)
    for bits in (8, 10, 12, 16):
        for transfer in TRANSFERS:
            for _ in range(40):
                y, u, v = (int(t) for t in rng.integers(0, 1 << bits, 3))
                got, want = D.ictcp(y, u, v, bits, transfer), [float(t) for t in R.ictcp(y, u, v, bits, transfer)]
                assert np.allclose(got, want, rtol=0, atol=1e-12), (bits, transfer, y, u, v)
    a, b = D.ictcp(512, 512, 512, 10), D.ictcp(513, 512, 512, 10)
    assert abs(D.de(a, b) - float(R.de(a, b))) < 1e-12 and D.de(a, a) == 0.0 and D.de(a, b) == D.de(b, a)


# ---- the pow alone ----------------------------------------------------------------------------------------------------------------
def _arguments():
    rng = np.random.default_rng(1)
    return np.concatenate([np.linspace(0, 1, 100001), rng.random(100000), 10.0 ** rng.uniform(-30, 0, 50000), [0.0, 1.0]]).astype(np.float32)


def test_log2_exp2_and_pow_against_float64():
    """dense and random arguments in [0, 1] for each of the five exponents; the exact values at 0 and 1; the largest relative error is
    recorded in itp_util.MEASURED_POW_REL: half an ulp of f32, the function is correctly rounded but for rare ties"""
    x = _arguments()
    x64 = x.astype(np.float64)
    worst = 0.0
    for k, e in enumerate(U.POW_EXPONENTS):
        got, want = U.kernel_pow(x, k).astype(np.float64), np.power(x64, e)
        assert got[-2] == 0.0 and got[-1] == 1.0 and got[0] == 0.0
        nz = want >= 1.2e-38
        worst = max(worst, float((np.abs(got[nz] - want[nz]) / want[nz]).max()))
    print("pow: largest relative error", worst)
    assert worst <= U.MEASURED_POW_REL
    pos = x[x > 0]
    lg, want = U.kernel_log2(pos).astype(np.float64), np.log2(pos.astype(np.float64))
    assert lg[-1] == 0.0 and (np.abs(lg - want) <= 6.0e-8 * np.abs(want)).all()
    t = np.random.default_rng(2).uniform(-120, 0, 100000).astype(np.float32)
    assert float(np.abs(U.kernel_exp2(t).astype(np.float64) / np.exp2(t.astype(np.float64)) - 1).max()) <= 6.0e-8
    assert U.kernel_exp2([0.0, -1.0, -2.0]).tolist() == [1.0, 0.5, 0.25]


# ---- the emulated kernel ----------------------------------------------------------------------------------------------------------
def test_emulation_against_restatement():
    """every shape, layout, depth, transfer and picture kind (one batch of all kinds per case); no position is skipped.  Prints the
    measured figures; they must not exceed the recorded ones, and the recorded absolute one must meet the condition"""
    A = Rr = M = 0.0
    for w, h in U.shapes():
        for layout, bits in U.CASES:
            for transfer in TRANSFERS:
                items = [want_of(w, h, bits, k, transfer, i) for i, k in enumerate(U.KINDS)]
                got = U.emulate(w, h, layout, bits, [len(items)], U.frames_of(layout, [it[0] for it in items], w, h, bits), transfer=transfer)
                for (pr, want), (s, mx, mp), kind in zip(items, got, U.KINDS):
                    why = U.agrees(mp, want, U.ATOL, U.RTOL)
                    assert why is None, (w, h, layout, bits, transfer, kind, why)
                    a, r = U.errors(mp, want)
                    A, Rr, M = max(A, a), max(Rr, r), max(M, U.mean_rel(s, want))
                    assert U.mean_rel(s, want) <= U.MEAN_REL_TOL and abs(mx - want.de_max) <= U.ATOL + U.RTOL * want.de_max
                    assert mx == float(mp.max())
    print("measured atol %.3e rtol %.3e mean rel %.3e" % (A, Rr, M))
    assert A <= U.MEASURED_ATOL and Rr <= U.MEASURED_RTOL and M <= U.MEASURED_MEAN_REL
    assert U.MEASURED_ATOL <= U.ATOL_LIMIT  # the condition: 1 % of a just-noticeable difference


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_identical_pictures_give_exactly_zero(layout, bits):
    w, h = 17, 9
    for transfer in TRANSFERS:
        prs = [U.pair(w, h, bits, k, seed=3)[0] for k in ("noise", "primaries", "near_black")]
        got = U.emulate(w, h, layout, bits, [3], U.frames_of(layout, [(p, p) for p in prs], w, h, bits), transfer=transfer)
        for s, mx, mp in got:
            assert s == 0.0 and mx == 0.0 and not mp.any()


def test_one_luma_code_step_at_mid_grey_and_swapped_sides():
    """neutral 512 -> 513 at 10 bits, PQ: the restatement's value (about 0.82); the sides exchanged give the same bits"""
    w, h = 8, 6
    g = (np.full((h, w), 512), np.full((h // 2, w // 2), 512), np.full((h // 2, w // 2), 512))
    g1 = (g[0] + 1, g[1], g[2])
    want = R.picture(g, g1, 10, "pq")
    assert abs(want.de_mean - 0.82) < 0.005 and abs(want.de_mean - D.de(D.ictcp(512, 512, 512), D.ictcp(513, 512, 512))) < 1e-12
    fwd = U.emulate(w, h, "i420", 10, [1], U.frames_of("i420", [(g, g1)], w, h, 10))[0]
    assert abs(fwd[0] / (w * h) - want.de_mean) <= U.ATOL and abs(fwd[1] - want.de_max) <= U.ATOL
    for layout, bits, kind in (("p016", 10, "noise"), ("i420", 12, "primaries"), ("nv12", 8, "near_peak")):
        for transfer in TRANSFERS:
            a, b = U.pair(17, 9, bits, kind, seed=8)
            one = U.emulate(17, 9, layout, bits, [2], U.frames_of(layout, [(a, b), (b, a)], 17, 9, bits, dirty=False), transfer=transfer)
            assert one[0][:2] == one[1][:2] and np.array_equal(one[0][2].view(np.uint32), one[1][2].view(np.uint32))


def test_the_transfer_reaches_the_kernel():
    a, b = U.pair(17, 9, 10, "near_neutral", seed=2)
    fr = U.frames_of("i420", [(a, b)], 17, 9, 10)
    pq, hlg = (U.emulate(17, 9, "i420", 10, [1], fr, transfer=t)[0] for t in TRANSFERS)
    assert pq[0] != hlg[0]
    got = U.kernel_ictcp(700, 400, 600, 10, "hlg").astype(np.float64)
    assert np.allclose(got, R.ictcp(700, 400, 600, 10, "hlg"), rtol=0, atol=2e-6)


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_load_paths_pitches_slots_and_repeats_give_the_same_bits(layout, bits):
    """tight planes, padded rows, 16-byte aligned planes on the wide and on the sample-by-sample path, batches 1 / 3 on one object's
    reused buffers, with and without maps"""
    tw, th = U.tile()
    w, h = tw + 9, th + 3
    pairs = [U.pair(w, h, bits, k, seed=5) for k in ("noise", "near_neutral", "one_code")]
    tight = U.frames_of(layout, pairs, w, h, bits)
    one = U.emulate(w, h, layout, bits, [3], tight)

    def same(other):
        return all(a[:2] == b[:2] and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)) for a, b in zip(one, other))
    assert same(U.emulate(w, h, layout, bits, [1, 1, 1], tight, cap=3))
    assert same(U.emulate(w, h, layout, bits, [2, 1], tight, cap=3))
    assert same(U.emulate(w, h, layout, bits, [3], U.frames_of(layout, pairs, w, h, bits, pad=5)))
    assert same(U.emulate(w, h, layout, bits, [3], U.frames_of(layout, pairs, w, h, bits, aligned=True)))
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
MISTAKE_PICTURES = (((17, 9), 10, "noise", "pq"), ((17, 9), 10, "primaries", "pq"), ((17, 9), 8, "near_neutral", "hlg"), ((16, 8), 10, "one_code", "pq"))


def _moved(mistake):
    """does the mistake move some position of some small test picture beyond the tolerance?"""
    for (w, h), bits, kind, transfer in MISTAKE_PICTURES:
        pr, right = want_of(w, h, bits, kind, transfer, 9)
        wrong = R.picture(pr[0], pr[1], bits, transfer, mistake)
        if U.agrees(wrong.map, right, U.ATOL, U.RTOL) is not None:
            return True
    return False


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_seeded_mistakes_are_caught(mistake):
    assert _moved(mistake)


def test_no_mistake_moves_nothing():
    assert set(R.MISTAKES) == {"ct_not_halved", "m1_m2_exchanged", "no_clamp", "chroma_at_xy", "bt709_matrix", "no_720"} and not _moved(None)


# ---- refusals and ABI ------------------------------------------------------------------------------------------------------------
def _supported(w, h, layout, bits):
    return 2 <= w <= 32768 and 2 <= h <= 32768 and {"nv12": bits == 8, "p016": 9 <= bits <= 16, "i420": 8 <= bits <= 16, "i420p10": bits == 10}[layout]


GEOMS = ((2, 2), (1, 2), (2, 1), (0, 0), (32768, 2), (32769, 2), (2, 32769), (3840, 2160), (0xFFFFFFFF, 0xFFFFFFFF))


def test_create_refuses_before_touching_the_device():
    L = D.lib()
    h = C.c_void_p()
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 12, 16, 17):
            for w, hh in GEOMS:
                ok = _supported(w, hh, layout, bits)
                assert (U.geom(w, hh, layout, bits) is not None) == ok
                if not ok:
                    assert L.tm_itp_create(C.byref(h), w, hh, U.LAYOUT[layout], bits, 0, 0, 0, 1) == tm.ffi.TM_ERR_UNSUPPORTED, (layout, bits, w, hh)
    U_, I_ = tm.ffi.TM_ERR_UNSUPPORTED, tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_itp_create(C.byref(h), 16, 16, 4, 8, 0, 0, 0, 1) == U_
    assert L.tm_itp_create(C.byref(h), 16, 16, 0, 8, 0, 1, 0, 1) == U_  # full range
    assert L.tm_itp_create(None, 16, 16, 0, 8, 0, 0, 0, 1) == I_
    assert L.tm_itp_create(C.byref(h), 16, 16, 0, 8, 0, 0, 0, 0) == I_
    assert L.tm_itp_create(C.byref(h), 16, 16, 0, 8, 0, 0, 0, 65536) == I_
    for t in (-1, 2):
        assert L.tm_itp_create(C.byref(h), 16, 16, 0, 8, t, 0, 0, 1) == I_
    assert h.value is None
    out = (C.c_double * 3)()
    assert L.tm_itp_ictcp(64, 512, 512, 7, 0, out) == U_ and L.tm_itp_ictcp(64, 512, 512, 10, 2, out) == I_ and L.tm_itp_ictcp(64, 512, 512, 10, 0, None) == I_
    assert L.tm_itp_hlg_display(None, out) == I_ and np.isnan(L.tm_itp_de(None, out))
    with pytest.raises(ValueError):
        tm.Itp(16, 16, "nv12", 8, transfer="sdr")


def declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(2) for m in re.finditer(r" ([A-Za-z]) (\S+)", out) if m.group(1) in "TDBRW" and not m.group(2).startswith(("_init", "_fini", "__bss", "_edata", "_end")))


def test_header_is_plain_c99_and_the_library_exports_exactly_it(tmp_path):
    want = declared("turbo_metrics_itp.h")
    assert len(want) == 13 and all(n.startswith("tm_itp") for n in want)
    assert exported(DLIB) == want
    assert sorted(D.SYMBOLS) == want
    listed = re.findall(r"^\s*(tm_[a-z0-9_]+);", open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "itp.map")).read(), flags=re.M)
    assert sorted(listed) == want
    src = tmp_path / "c.c"
    src.write_text('#include "turbo_metrics_itp.h"\n#include "turbo_metrics_yuv.h"\n#include <stdio.h>\n'
                   "int main(void) { tm_itp *s = NULL; tm_itp_frame f; double a[3], b[3]; (void)s; (void)f;\n"
                   "  if ((int)TM_ITP_NV12 != (int)TM_YUV_NV12 || (int)TM_ITP_P016 != (int)TM_YUV_P016 || (int)TM_ITP_I420 != (int)TM_YUV_I420 ||\n"
                   "      (int)TM_ITP_I420P10_PACKED != (int)TM_YUV_I420P10_PACKED || sizeof f != 32 || TM_ITP_PQ != 0 || TM_ITP_HLG != 1) return 3;\n"
                   "  if (tm_itp_ictcp(512, 512, 512, 10, TM_ITP_PQ, a) || tm_itp_ictcp(513, 512, 512, 10, TM_ITP_PQ, b)) return 4;\n"
                   "  printf(\"%.2f %.4f\\n\", tm_itp_de(a, b), tm_itp_pq_inv_eotf(203.0)); return 0; }\n")
    exe = str(tmp_path / "c")
    lib_dir = os.path.dirname(DLIB)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                           "-L" + lib_dir, "-lturbometrics_itp", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "0.82 0.5807", (out.returncode, out.stdout, out.stderr)


def test_the_other_libraries_export_nothing_of_it():
    libs = (tm.ffi.SHIP_LIB_PATH, tm.ffi.LIB_PATH, tm.xpsnr.LIB_PATH, tm.motion.LIB_PATH, tm.vif.LIB_PATH, tm.adm.LIB_PATH, tm.scene.LIB_PATH,
            tm.cambi.LIB_PATH, tm.flip.LIB_PATH, tm.yuv.LIB_PATH, tm.hvs.LIB_PATH, tm.ciede.LIB_PATH, tm.siti.LIB_PATH, tm.gmsd.LIB_PATH, tm.haarpsi.LIB_PATH)
    assert len(set(libs)) == 15
    for lib in libs:
        assert not [n for n in exported(lib) if "tm_itp" in n], lib
    assert not [n for n in exported(DLIB) if "ciede" in n]  # the kernels it takes from CIEDE2000's header are not entry points


class _FakeLib:
    """stands in for the library under an Itp object: any call after the plane checks is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_binding_rejects_bad_planes_before_the_library():
    m = tm.Itp.__new__(tm.Itp)
    m._L, m._h, m._keep = _FakeLib(), None, {}
    m.w, m.h, m.layout, m.bits, m.batch = 16, 16, "i420", 10, 2
    y, c = np.zeros((16, 16), np.uint16), np.zeros((8, 8), np.uint16)
    for bad in (y.astype(np.uint8), y.astype(np.float32), y[:15], y[:, :15], np.zeros((16, 32), np.uint16)[:, ::2], np.zeros(256, np.uint16), [[0] * 16] * 16):
        with pytest.raises(ValueError):
            m.set_frame(0, 0, (bad, c, c))
    for bad in (c[:7], c[:, :7], c.astype(np.uint8), np.zeros((8, 16), np.uint16)[:, ::2]):
        with pytest.raises(ValueError):
            m.set_frame(0, 1, (y, bad, c))
        with pytest.raises(ValueError):
            m.set_frame(0, 1, (y, c, bad))
    with pytest.raises(ValueError):
        m.set_frame(0, 0, (y, c))
    m.layout = "p016"
    with pytest.raises(ValueError):
        m.set_frame(0, 0, (y, c, c))
    with pytest.raises(ValueError):
        m.set_frame(0, 0, (y, c))  # the interleaved plane is 16 elements wide
    assert tm.itp.Itp is tm.Itp and tm.ItpFrame is D.ItpFrame


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
    assert out.returncode == 0 and all(s in out.stdout for s in ("-m deitp ", "--itp-transfer <pq|hlg>", "--itp-map <PREFIX>", "[and: deitp]"))
    assert "--matrix-coefficients is not consulted" in out.stdout
    lines = out.stdout.splitlines()
    at = [i for i, x in enumerate(lines) if x.strip() == "[and: haarpsi]"]
    assert len(at) == 1 and lines[at[0] + 1].strip() == "[and: deitp]"
    for sel in (["-m", "deitp"], ["-mdeitp", "-m", "psnr"], ["--metrics", "deitp", "--motion"], ["-m", "deitp", "--itp-transfer", "hlg"]):
        for extra in (["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
            out = run(a, b, *sel, *extra)
            assert out.returncode != 0 and "-m deitp does not run with" in out.stderr, (sel, extra, out.returncode, out.stderr)
    # usage errors: exit code 2
    for bad in ("itp", "de-itp", "DEITP", "deitp,psnr"):
        for form in (["-m", bad], ["-m" + bad], ["--metrics", bad]):
            out = run(a, b, *form)
            assert out.returncode == 2 and f"'{bad}'" in out.stderr, (form, out.returncode, out.stderr)
            assert VALUES in out.stderr and "deitp" in out.stderr.split(VALUES)[1]
    for opt in (["--itp-transfer", "hlg"], ["--itp-map", str(tmp_path / "m_")]):  # the options belong to -m deitp
        out = run(a, b, "-m", "psnr", *opt)
        assert out.returncode == 2 and "deitp" in out.stderr, (opt, out.returncode, out.stderr)
    for bad in ("sdr", "PQ", ""):
        out = run(a, b, "-m", "deitp", "--itp-transfer", bad)
        assert out.returncode == 2 and "--itp-transfer" in out.stderr, (bad, out.stderr)
    out = run(a, "-m", "deitp")  # the distorted argument is still required
    assert out.returncode == 2 and "<DISTORTED>" in out.stderr
