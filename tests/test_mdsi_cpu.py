"""MDSI without a GPU: the kernel SOURCE run lane by lane on the CPU (tests/mdsi_emul) against the float64
restatement in the paper's form (tests/mdsi_ref.py), the measured tolerance, the automatic factor, hand values, seeded mistakes, the
refusals and the ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mdsi_ref as R
from tests import mdsi_util as U
from tm_pkg import tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = tm.mdsi
DLIB = D.LIB_PATH

_WANT = {}


def want_of(w, h, bits, kind, f, matrix="bt709", seed=0):
    """(the pair, its restatement), computed once"""
    key = (w, h, bits, kind, f, matrix, seed)
    if key not in _WANT:
        pr = U.pair(w, h, bits, kind, seed=seed, scale=f or R.factor(w, h))
        _WANT[key] = (pr, R.mdsi(pr[0], pr[1], bits, matrix, f))
    return _WANT[key]


def sweep():
    """(f, w, h, layout, bits, kind, vec): every forced factor x every shape x every layout / depth case, two kinds and one load path
    each, rotated so that every kind meets every case and every factor on both paths"""
    for fi, f in enumerate(U.FACTORS):
        for si, (w, h) in enumerate(U.shapes(f)):
            for ci, (layout, bits) in enumerate(U.CASES):
                for kk in range(2):
                    yield f, w, h, layout, bits, U.KINDS[(ci + si + 3 * kk) % len(U.KINDS)], (None if (ci + kk + fi) % 2 == 0 else False)


def test_the_sweep_covers_what_it_says():
    seen = list(sweep())
    assert {(s[3], s[4]) for s in seen} == set(U.CASES) and {s[0] for s in seen} == set(U.FACTORS)
    for kind in U.KINDS:
        assert {(s[3], s[4], s[6]) for s in seen if s[5] == kind} == {(l, b, v) for l, b in U.CASES for v in (None, False)}, kind
        assert {s[0] for s in seen if s[5] == kind} == set(U.FACTORS)
    assert max(s[1] for s in seen) <= 300 and max(s[2] for s in seen) <= 200
    tw, th = U.tile()
    for f in (1, 2, 3, 4):  # one below, at and one above a tile edge, each way
        dec = {(-(-w // f), -(-h // f)) for w, h in U.shapes(f)}
        assert {d[0] for d in dec} >= {tw - 1, tw, tw + 1} and {d[1] for d in dec} >= {th - 1, th, th + 1}, (f, dec)


def test_emulation_against_restatement():
    worst_mad, worst_mdsi = (0.0, None), (0.0, None)
    negative_factors = set()
    for f, w, h, layout, bits, kind, vec in sweep():
        pr, want = want_of(w, h, bits, kind, f)
        got = U.emulate_pair(w, h, layout, bits, pr, factor=f, vec=vec)
        assert got.n == want.n and got.negatives == want.negatives, (f, w, h, layout, bits, kind)
        em = abs(got.mad - want.mad)
        if em > worst_mad[0]:
            worst_mad = (em, (f, w, h, layout, bits, kind, vec))
        if want.mdsi >= U.MDSI_FLOOR:
            ed = abs(got.mdsi - want.mdsi)
            if ed > worst_mdsi[0]:
                worst_mdsi = (ed, (f, w, h, layout, bits, kind, vec, want.mdsi))
        if kind == "identical":
            assert got.dev == 0.0 and got.mdsi == 0.0 and (got.map == 1.0).all() and got.sum_re == want.n and got.sum_im == 0.0
        if kind == "negative" and want.negatives:
            negative_factors.add(f)
            assert got.sum_im > 0
    print(f"\nlargest |MAD - ref| {worst_mad[0]:.3e} at {worst_mad[1]}; largest |mdsi - ref| over mdsi >= {U.MDSI_FLOOR}: {worst_mdsi[0]:.3e} at "
          f"{worst_mdsi[1]}; per-position expression: f{8 * U.real_bytes()}")
    # the restatement itself finds GCS < 0 in the "negative" kind at every factor: the complex branch is exercised
    assert negative_factors == set(U.FACTORS)
    # the condition that decides f32 against f64 per position
    assert worst_mdsi[0] <= U.MDSI_LIMIT and U.MEASURED_MDSI <= U.MDSI_LIMIT
    assert worst_mad[0] <= U.MEASURED_MAD and worst_mdsi[0] <= U.MEASURED_MDSI  # the figures in mdsi_util are the measured ones
    assert U.MAD_TOL == 4 * U.MEASURED_MAD and U.MDSI_TOL == 4 * U.MEASURED_MDSI


@pytest.mark.parametrize("m,f", [(383, 1), (384, 2), (639, 2), (640, 3), (895, 3), (896, 4), (1, 1), (255, 1), (1080, 4), (2160, 8), (32768, 128)])
def test_automatic_factor(m, f):
    assert R.factor(m, m + 100) == f and R.factor(m + 7, m) == f and D.factor(m, m + 100) == f and D.factor(m + 7, m) == f
    if m >= 4:
        g = U.geom(m, m - 1, "i420", 8)
        assert g["f"] == R.factor(m, m - 1) and (g["wd"], g["hd"]) == (-(-m // g["f"]), -(-(m - 1) // g["f"]))
        assert U.geom(m, m, "i420", 8)["f"] == f


def _real_picture():
    return want_of(640, 641, 8, "chroma_only", 0)


def test_a_real_picture_at_640_x_641_takes_factor_3():
    pr, want = _real_picture()
    assert want.factor == 3 and R.factor(640, 641, "half_even") == 2
    got = U.emulate_pair(640, 641, "nv12", 8, pr)
    assert got.map.shape == (214, 214) and got.n == want.n
    assert abs(got.mad - want.mad) <= U.MAD_TOL and abs(got.mdsi - want.mdsi) <= U.MDSI_TOL, (got.mdsi, want.mdsi)


def test_by_height_picks_the_matrix():
    assert U.geom(1280, 720, "nv12", 8, "by_height")["matrix"] == 0 and U.geom(1280, 719, "nv12", 8, "by_height")["matrix"] == 1
    pr, w709 = want_of(33, 19, 8, "noise", 2, "bt709")
    _, w601 = want_of(33, 19, 8, "noise", 2, "bt601")
    assert abs(w709.mad - w601.mad) > 10 * U.MAD_TOL  # the two matrices are told apart
    for m, want in (("bt601", w601), ("by_height", w601), ("bt709", w709)):
        got = U.emulate_pair(33, 19, "i420", 8, pr, factor=2, matrix=m)
        assert abs(got.mad - want.mad) <= U.MAD_TOL, m


# ---- hand values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,bits", [("nv12", 8), ("i420", 8), ("p016", 10), ("i420p10", 10), ("i420", 16), ("p016", 16)])
def test_identical_pictures_give_exactly_zero(layout, bits):
    for f, (w, h) in ((1, (37, 21)), (3, (50, 35)), (4, (67, 41))):
        pr, _ = want_of(w, h, bits, "identical", f)
        for vec in (None, False):
            got = U.emulate_pair(w, h, layout, bits, pr, factor=f, vec=vec)
            assert (got.map == 1.0).all() and got.dev == 0.0 and got.mdsi == 0.0 and got.negatives == 0 and got.sum_re == got.n and got.sum_im == 0.0


def test_flat_against_flat_at_5_x_5_by_hand():
    """5 x 5, f = 2: the windows are [2 i, 2 i + 1], so the decimated plane is 3 x 3 and column 5 and row 5, which do not exist, enter
    the last windows as zeros with the divisor still 4.  A flat picture of plane value a therefore decimates to a W with
        W = [[1, 1, 1/2], [1, 1, 1/2], [1/2, 1/2, 1/4]].
    Prewitt with zeros beyond the 3 x 3 plane: the vertical three-sums of W's columns are (2, 5/2, 3/2) for columns 0 and 1 and
    (1, 5/4, 3/4) for column 2, so 3 gx = right minus left =
        [[2, -1, -2], [5/2, -5/4, -5/2], [3/2, -3/4, -3/2]]
    and, W being symmetric, 3 gy is its transpose.  With k = sqrt(gx^2 + gy^2) of W: g_r = a_L k, g_d = b_L k, g_f = (a_L + b_L) k / 2;
    H and M are a_H W, a_M W.  Everything else is the definition's quotients at nine positions."""
    s = 1
    ref, dis = (90 * s, 100 * s, 170 * s), (140 * s + 1, 150 * s, 120 * s)
    pr = U.pair(5, 5, 8, "flat_flat")
    assert all((p == v).all() for p, v in zip(pr[0], ref)) and all((p == v).all() for p, v in zip(pr[1], dis))
    W = np.array([[1, 1, .5], [1, 1, .5], [.5, .5, .25]])
    gx3 = np.array([[2, -1, -2], [2.5, -1.25, -2.5], [1.5, -.75, -1.5]])
    k = np.sqrt(gx3 ** 2 + gx3.T ** 2) / 3
    a, b = D.lhm(*ref, "bt709", 8), D.lhm(*dis, "bt709", 8)
    gr, gd, gf = a[0] * k, b[0] * k, (a[0] + b[0]) / 2 * k
    q = lambda x, y, c: (2 * x * y + c) / (x * x + y * y + c)
    gs = q(gr, gd, 140.0) + q(gd, gf, 55.0) - q(gr, gf, 55.0)
    cs = (2 * (a[1] * b[1] + a[2] * b[2]) * W * W + 550.0) / ((a[1] ** 2 + b[1] ** 2 + a[2] ** 2 + b[2] ** 2) * W * W + 550.0)
    gcs = 0.6 * gs + 0.4 * cs
    z = gcs.astype(complex) ** 0.25
    mad = float(np.abs(z - z.mean()).mean())
    assert 0.01 < mad ** 0.25 < 1
    for layout in ("nv12", "i420"):
        got = U.emulate_pair(5, 5, layout, 8, pr, factor=2)
        assert np.abs(got.map - gcs).max() < 1e-6
        assert abs(got.mad - mad) <= U.MAD_TOL and abs(got.mdsi - mad ** 0.25) <= U.MDSI_TOL, (got.mdsi, mad ** 0.25)
    want = R.mdsi(pr[0], pr[1], 8, "bt709", 2)
    assert abs(want.mad - mad) < 1e-12


# ---- seeded mistakes ---------------------------------------------------------------------------------------------------------------
def _mistake_case(mistake):
    """(w, h, kind, f): a picture on which the mistake matters"""
    if mistake == "half_even":
        return 640, 641, "chroma_only", 0
    return 25, 19, "negative" if mistake == "mu_real" else "noise", 3


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_seeded_mistakes_are_caught(mistake):
    w, h, kind, f = _mistake_case(mistake)
    pr, want = want_of(w, h, 8, kind, f)
    got = U.emulate_pair(w, h, "i420", 8, pr, factor=f)
    wrong = R.mdsi(pr[0], pr[1], 8, "bt709", f, mistake=mistake)
    print(f"\n{mistake}: mdsi {want.mdsi:.6f}, with the mistake {wrong.mdsi:.6f}, emulated {got.mdsi:.6f}")
    assert abs(got.mad - want.mad) <= U.MAD_TOL and abs(got.mdsi - want.mdsi) <= U.MDSI_TOL
    if wrong.gcs.shape == got.map.shape:
        assert abs(got.mad - wrong.mad) > U.MAD_TOL and abs(got.mdsi - wrong.mdsi) > U.MDSI_TOL
    else:
        assert mistake == "half_even" and wrong.factor == 2
        g = U.geom(w, h, "i420", 8)  # the kernel's own geometry, which the library and the emulation share: halves go up
        assert g["f"] == 3 == want.factor and got.map.shape == (g["hd"], g["wd"]) == (214, 214) and D.factor(w, h) == 3


def test_nothing_beside_the_rows_is_read():
    """padded rows filled with garbage, odd sizes, both paths: the bits of the tight planes"""
    for layout, bits in (("nv12", 8), ("p016", 10), ("i420", 12), ("i420p10", 10)):
        pr, _ = want_of(25, 19, bits, "noise", 2)
        base = U.emulate_pair(25, 19, layout, bits, pr, factor=2, aligned=False, vec=False)
        for pad, aligned, vec in ((0, True, None), (7, True, None), (5, False, None), (16, True, False)):
            got = U.emulate_pair(25, 19, layout, bits, pr, factor=2, pad=pad, aligned=aligned, vec=vec)
            assert (got.map == base.map).all() and (got.sum_re, got.sum_im, got.dev, got.negatives) == (base.sum_re, base.sum_im, base.dev, base.negatives)


def test_slots_and_repeats_give_the_same_bits():
    w, h, f = 70, 37, 2
    prs = [want_of(w, h, 8, kind, f)[0] for kind in ("noise", "identical", "negative", "chroma_only")]
    fr = U.frames_of("nv12", prs, w, h, 8, aligned=True)
    one = [U.emulate(w, h, "nv12", 8, [1], [x], factor=f)[0] for x in fr]
    many = U.emulate(w, h, "nv12", 8, [4, 1, 3], fr + fr[:1] + fr[1:], factor=f, cap=4)
    for a, b in zip(many, one + one[:1] + one[1:]):
        assert (a.map == b.map).all() and (a.sum_re, a.sum_im, a.dev, a.negatives) == (b.sum_re, b.sum_im, b.dev, b.negatives)


# ---- the host functions, the refusals and the ABI --------------------------------------------------------------------------------
def test_host_functions_are_the_restatement():
    for bits in (8, 10, 16):
        s = 1 << (bits - 8)
        for m in ("bt709", "bt601"):
            for yuv in ((16 * s, 128 * s, 128 * s), (235 * s, 128 * s, 128 * s), (81 * s, 90 * s, 240 * s), (0, 0, (1 << bits) - 1)):
                want = R.lhm(*(np.float64(v) for v in yuv), bits, m)
                assert np.allclose(D.lhm(*yuv, m, bits), want, rtol=0, atol=1e-10)
    assert np.allclose(D.lhm(235, 128, 128), (0.9999 * 255, -0.01 * 255, -0.09 * 255), atol=1e-9)  # white: the coefficient sums
    assert D.score(0.0, 9) == 0.0 and D.score(9 * 0.0016, 9) == pytest.approx(0.2) and np.isnan(D.score(1.0, 0))
    assert R.score(9 * 0.0016, 9) == pytest.approx(0.2)


def test_create_refuses_before_touching_the_device():
    L = D.lib()
    h = C.c_void_p()
    U_, I_ = tm.ffi.TM_ERR_UNSUPPORTED, tm.ffi.TM_ERR_INVALID_ARG
    create = lambda w, hh, layout, bits, matrix=0, factor=0, flags=0, batch=1, out=h: L.tm_mdsi_create(
        C.byref(out) if out is not None else None, w, hh, layout, bits, matrix, factor, flags, batch)
    for w, hh, layout, bits in ((1, 8, 0, 8), (8, 1, 0, 8), (32769, 8, 0, 8), (8, 32769, 0, 8), (16, 16, 0, 10), (16, 16, 1, 8), (16, 16, 1, 17),
                                (16, 16, 2, 7), (16, 16, 3, 8), (16, 16, 4, 8), (0, 0, 0, 8)):
        assert create(w, hh, layout, bits) == U_, (w, hh, layout, bits)
        assert U.geom(w, hh, layout, bits) == -1
    # fewer than four decimated positions
    assert create(3, 2, 0, 8, factor=2) == U_ and create(128, 300, 0, 8, factor=128) == U_ and create(2, 2, 0, 8, factor=2) == U_
    assert U.geom(2, 2, "nv12", 8)["n"] == 4 and U.geom(3, 2, "nv12", 8, factor=2) == -1
    assert create(16, 16, 0, 8, out=None) == I_ and create(16, 16, 0, 8, batch=0) == I_ and create(16, 16, 0, 8, batch=65536) == I_
    assert create(16, 16, 0, 8, flags=2) == I_ and create(16, 16, 0, 8, matrix=3) == I_ and create(16, 16, 0, 8, matrix=-1) == I_
    assert create(16, 16, 0, 8, factor=129) == I_ and U.geom(16, 16, "nv12", 8, factor=129) == -2
    assert h.value is None
    out = (C.c_double * 3)()
    assert L.tm_mdsi_lhm(16, 128, 128, 0, 7, out) == U_ and L.tm_mdsi_lhm(16, 128, 128, 2, 8, out) == I_ and L.tm_mdsi_lhm(16, 128, 128, 0, 8, None) == I_
    with pytest.raises(ValueError):
        tm.Mdsi(16, 16, "nv12", 8, matrix="bt2020")
    with pytest.raises(ValueError):
        tm.Mdsi(16, 16, "yuy2", 8)
    assert L.tm_mdsi_get_factor(None) == 0


def declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(2) for m in re.finditer(r" ([A-Za-z]) (\S+)", out) if m.group(1) in "TDBRW" and not m.group(2).startswith(("_init", "_fini", "__bss", "_edata", "_end")))


def test_header_is_plain_c99_and_the_library_exports_exactly_it(tmp_path):
    want = declared("turbo_metrics_mdsi.h")
    assert len(want) == 12 and all(n.startswith("tm_mdsi") for n in want)
    assert exported(DLIB) == want
    assert sorted(D.SYMBOLS) == want
    listed = re.findall(r"^\s*(tm_[a-z0-9_]+);", open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "mdsi.map")).read(), flags=re.M)
    assert sorted(listed) == want
    src = tmp_path / "c.c"
    src.write_text('#include "turbo_metrics_mdsi.h"\n#include "turbo_metrics_ciede.h"\n#include <stdio.h>\n'
                   "int main(void) { tm_mdsi *s = NULL; tm_mdsi_frame f; double a[3]; (void)s; (void)f;\n"
                   "  if ((int)TM_MDSI_NV12 != (int)TM_CIEDE_NV12 || (int)TM_MDSI_P016 != (int)TM_CIEDE_P016 || (int)TM_MDSI_I420 != (int)TM_CIEDE_I420 ||\n"
                   "      (int)TM_MDSI_I420P10_PACKED != (int)TM_CIEDE_I420P10_PACKED || (int)TM_MDSI_BT709 != (int)TM_CIEDE_BT709 ||\n"
                   "      (int)TM_MDSI_BT601 != (int)TM_CIEDE_BT601 || sizeof f != 48 || TM_MDSI_MAPS != 1) return 3;\n"
                   "  if (tm_mdsi_lhm(235, 128, 128, TM_MDSI_BT709, 8, a)) return 4;\n"
                   "  printf(\"%u %.3f %.4f\\n\", (unsigned)tm_mdsi_factor(640, 641), a[0], tm_mdsi_score(0.0144, 9)); return 0; }\n")
    exe = str(tmp_path / "c")
    lib_dir = os.path.dirname(DLIB)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                           "-L" + lib_dir, "-lturbometrics_mdsi", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "3 254.974 0.2000", (out.returncode, out.stdout, out.stderr)


def test_the_other_libraries_export_nothing_of_it():
    libs = (tm.ffi.SHIP_LIB_PATH, tm.ffi.LIB_PATH, tm.xpsnr.LIB_PATH, tm.motion.LIB_PATH, tm.vif.LIB_PATH, tm.adm.LIB_PATH, tm.scene.LIB_PATH,
            tm.cambi.LIB_PATH, tm.flip.LIB_PATH, tm.yuv.LIB_PATH, tm.hvs.LIB_PATH, tm.ciede.LIB_PATH, tm.siti.LIB_PATH, tm.gmsd.LIB_PATH,
            tm.haarpsi.LIB_PATH, tm.itp.LIB_PATH)
    assert len(set(libs)) == 16
    for lib in libs:
        assert not [n for n in exported(lib) if "tm_mdsi" in n], lib
    assert not [n for n in exported(DLIB) if "ciede" in n]  # what it takes from CIEDE2000's header are not entry points


def test_the_kernel_header_keeps_to_plain_stores_and_the_shared_loaders():
    src = open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "tm_mdsi_kernels.h")).read()
    code = re.sub(r"//.*", "", src)
    assert "atomic" not in code and "asm" not in code
    assert "tmx::load4_raw" in code and "tmx::sample1" in code and '#include "tm_ciede_kernels.h"' in code
    host = open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "tm_mdsi.hip")).read()
    assert '#include "tm_feature_host.h"' in host and "TmFeatureHost c;" in host
    for call in ("hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree(", "hipStreamCreateWithFlags(", "hipStreamDestroy(", "hipGetDevice(", "hipMemset"):
        assert call not in host, call


def test_cli_names_the_value_and_refuses_what_it_cannot_do_before_touching_the_device(tmp_path):
    cli = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
    out = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and all(s in out.stdout for s in ("-m mdsi ", "--mdsi-factor <N>", "--mdsi-map <PREFIX>", "[and: mdsi]"))
    assert "the sequence value is the\n" in out.stdout and "mean of the per-pair values" in out.stdout  # MDSI does not pool across pictures
    lines = out.stdout.splitlines()
    at = [i for i, x in enumerate(lines) if x.strip() == "[and: deitp]"]
    assert len(at) == 1 and lines[at[0] + 1].strip() == "[and: mdsi]"  # after every existing value
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    for p in (a, b):
        with open(p, "wb") as f:
            f.write(b"YUV4MPEG2 W8 H8 F25:1 Ip A1:1 C420jpeg\nFRAME\n" + bytes(96))
    for args, what in ((("-m", "psnr", "--mdsi-factor", "2"), "belong to '-m mdsi'"), (("-m", "psnr", "--mdsi-map", "x"), "belong to '-m mdsi'"),
                       (("-m", "mdsi", "--mdsi-factor", "0"), "--mdsi-factor"), (("-m", "mdsi", "--mdsi-factor", "129"), "--mdsi-factor"),
                       (("-m", "mdsi", "--mdsi-factor", "x"), "--mdsi-factor"), (("-m", "mdsi", "--mdsi-map"), "--mdsi-map"),
                       (("-m", "mdsi", "--devices", "2"), "-m mdsi does not run with --devices"), (("-m", "mdsx"), "[and: mdsi]")):
        out = subprocess.run([cli, a, b, *args], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and what in out.stderr, (args, out.returncode, out.stderr)
