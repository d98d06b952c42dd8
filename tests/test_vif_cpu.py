"""No-GPU tier of VMAF's VIF (include/turbo_metrics_vif.h, libturbometrics_vif.so): the filter tables, the hand-derived answers of
DESIGN.md section 10 as literals against the numpy restatement (tests/vif_ref.py) and against the kernel SOURCE executed lane by lane
on the CPU (tests/vif_emul); emulated kernel == restatement, the three integer planes of all four scales bit-exact and the sums
within 1e-9, on all four layouts, with dirty bytes; create-time refusals; the ABI (C99 header, exports); tm_vif_scores; the binding's
checks; the CLI's option parsing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import motion_ref
from tests import vif_ref as R
from tests import vif_util as U
from tm_pkg import tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VLIB = os.path.join(ROOT, "turbo-metrics_amd", "libturbometrics_vif.so")
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
# Derived, not measured: branches are taken on integers and the order of the operations is fixed, so the sums differ only by log2
# (a few ulp of 2^-53 per term) and by the order of adding at most 2^23 non-negative terms (<= n 2^-53, about 1e-9, at worst).
RTOL = 1e-9
SEEN = {"rel": 0.0}  # the largest relative difference between the emulated kernel's sums and the restatement's (printed at the end)


def declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(2) for m in re.finditer(r" ([A-Za-z]) (\S+)", out) if m.group(1) in "TDBRW" and not m.group(2).startswith(("_init", "_fini", "__bss", "_edata", "_end")))


def emul(w, h, layout, bits, ref, dis, pad=0, dirty=None):
    return U.emulate(w, h, layout, bits, U.luma_plane(layout, ref, bits, pad=pad, dirty=dirty),
                     U.luma_plane(layout, dis, bits, pad=pad, dirty=None if dirty is None else dirty + 1))


def check_against_restatement(got, want, what):
    for s in range(4):
        for name, a, b in zip(("s1", "s2", "s12"), got[s]["planes"], want[s]["planes"]):
            assert a.shape == b.shape and np.array_equal(a, b), (what, s, name, int(np.abs(a.astype(np.int64) - b).max()))
        for k in ("num", "den"):
            rel = abs(got[s][k] - want[s][k]) / max(abs(want[s][k]), 1e-300) if want[s][k] != got[s][k] else 0.0
            SEEN["rel"] = max(SEEN["rel"], rel)
            print(f"{what} scale {s} {k}: kernel {got[s][k]!r} restatement {want[s][k]!r} rel {rel:.3e}")
            assert rel <= RTOL, (what, s, k, got[s][k], want[s][k])


# ---- the filters -------------------------------------------------------------------------------------------------------------
def test_filter_tables():
    for tab in (R.F, U.filters()):
        assert [len(f) for f in tab] == [17, 9, 5, 3]
        for f in tab:
            assert sum(f) == 65536 and tuple(f) == tuple(reversed(f))
        assert tuple(tab[2]) == tuple(motion_ref.F)
    assert U.filters() == R.F
    assert R.F[0][8] == 7784 and R.F[0][7] == 7455 and R.F[1][3] == 12590 and R.F[1][4] == 14692 and R.F[3] == (10904, 43728, 10904)


def test_the_mirror_is_symmetric_and_not_motions():
    L = U.emul_lib()
    for n in (4, 5, 32):
        assert [R.mirror(i, n) for i in (-2, -1, 0, n - 1, n, n + 1)] == [2, 1, 0, n - 1, n - 2, n - 3]
        assert all(L.ve_mirror(i, n) == R.mirror(i, n) for i in range(-3, n + 3) if -n < i < 2 * n - 1)
    assert motion_ref.mirror(32, 32) == 31 != R.mirror(32, 32)


@pytest.mark.parametrize("w,h,want", [(32, 32, [(32, 32), (16, 16), (8, 8), (4, 4)]), (33, 47, [(33, 47), (16, 23), (8, 11), (4, 5)]),
                                      (1920, 1080, [(1920, 1080), (960, 540), (480, 270), (240, 135)]), (101, 75, [(101, 75), (50, 37), (25, 18), (12, 9)])])
def test_scale_sizes(w, h, want):
    assert R.sizes(w, h) == want
    ws, hs = (C.c_int * 4)(), (C.c_int * 4)()
    assert U.emul_lib().ve_sizes(w, h, 0, 8, ws, hs) == 0
    assert list(zip(ws, hs)) == want


# ---- by hand, no tolerance ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,bits", U.CASES)
def test_flat_pictures_are_exactly_one(layout, bits):
    w, h = 53, 37  # odd, and not a multiple of 8 or of the tile
    M = (1 << bits) - 1
    for lr, ld in ((1, 1), (M // 2, M // 2), (M, M), (0, M), (M // 3, M // 2 + 1)):
        ref, dis = np.full((h, w), lr, np.int64), np.full((h, w), ld, np.int64)
        want = R.vif(ref, dis, bits)
        got = emul(w, h, layout, bits, ref, dis, pad=3, dirty=7)
        for s, (ws, hs) in enumerate(R.sizes(w, h)):
            for res in (want, got):
                assert all((p == 0).all() and p.shape == (hs, ws) for p in res[s]["planes"]), (s, lr, ld)
                assert res[s]["num"] == res[s]["den"] == float(ws * hs), (s, lr, ld, res[s]["num"], res[s]["den"])
        assert R.scores(want) == R.scores(got) == [1.0] * 5


def test_single_bright_sample_by_hand():
    """ref: one sample of 255 at row 20, column 19 of a 48 x 48 field of zeros, D = 8, scale 0; dis: zeros.  On paper (F0[8] = 7784 is
    the centre tap, F0[7] = 7455 its neighbour; 8-bit input: the vertical shift is 8 with rounding 128, q = 0):
      vertical, column 19:  m1v[20] = (7784 * 255 + 128) >> 8 = 1985048 >> 8 = 7754      xxv[20] = 7784 * 255^2 = 506154600
                            m1v[21] = (7455 * 255 + 128) >> 8 = 1901153 >> 8 = 7426      xxv[21] = 7455 * 255^2 = 484761375
      horizontal, row 20:   column 19: m1 = 7784 * 7754 = 60357136, xx = (7784 * 506154600 + 32768) >> 16 = 60118216,
                                       (m1^2 + 2^31) >> 32 = 848198, s1 = 60118216 - 848198 = 59270018
                            column 20: m1 = 7455 * 7754 = 57806070, xx = (7455 * 506154600 + 32768) >> 16 = 57577248,
                                       (m1^2 + 2^31) >> 32 = 778013, s1 = 56799235
      row 21, column 19:    m1 = 7784 * 7426 = 57803984, xx = (7784 * 484761375 + 32768) >> 16 = 57577248, s1 = 56799291
    and 17 x 17 pixels around the sample are the only ones that are not 0; s2 = s12 = 0 everywhere."""
    w = h = 48
    ref, dis = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    ref[20, 19] = 255
    (s1, s2, s12), mid = R.moments(ref, dis, 0, 8)
    assert mid["m1v"][20, 19] == 7754 and mid["m1v"][21, 19] == 7426 and mid["m1v"][19, 19] == 7426
    assert mid["xxv"][20, 19] == 506154600 and mid["xxv"][21, 19] == 484761375
    assert mid["m1"][20, 19] == 60357136 and mid["xx"][20, 19] == 60118216 and mid["m1"][20, 20] == 57806070 and mid["xx"][20, 20] == 57577248
    got = emul(w, h, "y8", 8, ref, dis)[0]["planes"]
    for p1, p2, p12 in ((s1, s2, s12), got):
        assert p1[20, 19] == 59270018 and p1[20, 20] == 56799235 == p1[20, 18] and p1[21, 19] == 56799291 == p1[19, 19]
        assert (p2 == 0).all() and (p12 == 0).all()
        outside = np.ones((h, w), bool)
        outside[12:29, 11:28] = False
        assert (p1[outside] == 0).all() and (p1[12:29, 11:28] > 0).all()
    assert np.array_equal(got[0], s1)


def test_corner_sample_by_hand_needs_the_symmetric_mirror():
    """The same sample in the bottom-right corner (47, 47).  With the symmetric mirror rows 48, 49, ... read rows 46, 45, ...: row 47
    is read ONCE by the pixels of row 47 (centre tap) and once by those of row 46 (F0[9] = 7455), so the corner pixel has the values
    of the centre pixel above and its upper neighbour those of the neighbour above.  Motion's mirror would repeat row 47
    (m1v[47] = ((7784 + 7455) * 255 + 128) >> 8 = 15179)."""
    w = h = 48
    ref, dis = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    ref[47, 47] = 255
    (s1, _, _), mid = R.moments(ref, dis, 0, 8)
    assert mid["m1v"][47, 47] == 7754 and mid["m1v"][46, 47] == 7426 and mid["xxv"][47, 47] == 506154600
    got = emul(w, h, "y8", 8, ref, dis)[0]["planes"][0]
    for p in (s1, got):
        assert p[47, 47] == 59270018 and p[47, 46] == 56799235 and p[46, 47] == 56799291
    assert np.array_equal(got, s1)


def test_decimation_by_hand():
    """A picture that is 255 on one row only (row 10, every column), D = 8.  Scale 1 uses F1 (9 taps, centre 14692, then 12590,
    7925, 3663, 1244): t[r] = (F1[4 - (r - 10)] * 255 + 128) >> 8 for |r - 10| <= 4, the horizontal pass of a row-constant t gives
    (65536 t + 32768) >> 16 = t, and x1[r'] = t[2 r'], so rows 3 .. 7 of x1 are
      (1244 * 255 + 128) >> 8 = 1239, (7925 * 255 + 128) >> 8 = 7894, (14692 * 255 + 128) >> 8 = 14635, 7894, 1239
    on the 16-bit scale, and 0 elsewhere.  F0 there instead of F1 would give 7754 at the centre."""
    w, h = 40, 36
    ref = np.zeros((h, w), np.int64)
    ref[10, :] = 255
    x1 = R.decimate(ref, 1, 8)
    assert x1.shape == (18, 20)
    assert [int(v) for v in x1[:, 0]] == [0, 0, 0, 1239, 7894, 14635, 7894, 1239] + [0] * 10 and (x1 == x1[:, :1]).all()
    # the moments of scale 1 see those values: a flat row pattern has s1 > 0 only around rows 3 .. 7
    got, want = emul(w, h, "y8", 8, ref, ref), R.vif(ref, ref, 8)
    check_against_restatement(got, want, "one bright row")
    assert (want[1]["planes"][0][5] > 0).all()


# ---- emulated kernel vs restatement ------------------------------------------------------------------------------------------
SIZES = ((32, 32), (33, 47), (75, 35), (100, 40))  # the smallest; odd; a width that is not a multiple of the tile; 3 x 3 tiles


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("layout,bits", U.CASES)
def test_emulated_kernel_matches_the_restatement(layout, bits, w, h):
    kind = U.CONTENTS[(U.CASES.index((layout, bits)) + SIZES.index((w, h))) % len(U.CONTENTS)]
    ref, dis = U.pair(w, h, bits, kind)
    check_against_restatement(emul(w, h, layout, bits, ref, dis, pad=5, dirty=11), R.vif(ref, dis, bits), f"{layout} {bits} {w}x{h} {kind}")


@pytest.mark.parametrize("kind", U.CONTENTS)
@pytest.mark.parametrize("layout,bits", [("y8", 8), ("y16_msb", 16), ("y10_packed", 10)])
def test_every_content_on_several_tiles(layout, bits, kind):
    w, h = 100, 40
    ref, dis = U.pair(w, h, bits, kind, seed=3)
    want = R.vif(ref, dis, bits)
    got = emul(w, h, layout, bits, ref, dis)
    check_against_restatement(got, want, f"{layout} {bits} {kind}")
    sc = R.scores(got)
    if kind == "identical":
        # Not exactly 1: g = C / (A + 1e-10).  And where a pixel's variance is below the noise variance (0 < a < 131072) the
        # definition's first branch gives num = 1 - B 4/65025 against den = 1 even for identical pictures: the smoothed 8-bit noise
        # of scale 3 has such pixels (vif_scale3 = 0.99999937).  That deficit is computed here from the integer planes; what is
        # left of |vif_scale_s - 1| is held to 1e-9, and where no pixel takes that branch this is |vif_scale_s - 1| <= 1e-9 itself.
        for s in range(4):
            a = want[s]["planes"][0].astype(np.int64)
            deficit = float((np.where((a < 131072) & (a > 0), a, 0) / 65536.0 * (4.0 / 65025.0)).sum())
            for res in (want, got):
                assert abs((res[s]["num"] + deficit) / res[s]["den"] - 1.0) <= 1e-9, (s, deficit, res[s])
            if deficit == 0.0:
                assert abs(sc[s] - 1.0) <= 1e-9, (s, sc)
        if bits != 8:
            assert all(abs(v - 1.0) <= 1e-9 for v in sc), sc  # full-range noise of more than 8 bits keeps every variance above 2
    if kind == "negative":
        assert all(int(p["planes"][2].max()) <= 0 for p in want)
    if kind == "flat_ref":
        assert (want[0]["planes"][0] == 0).all() and int(want[0]["planes"][1].min()) > 131072 and want[0]["den"] == float(w * h)


def test_largest_difference_seen():
    """prints what DESIGN.md section 10 records (run after the comparisons above: pytest keeps file order)"""
    print(f"largest relative difference of num / den, emulated kernel vs restatement: {SEEN['rel']:.3e}")
    assert SEEN["rel"] <= RTOL


@pytest.mark.parametrize("layout,bits", [("y16_low", 10), ("y16_msb", 12), ("y8", 8), ("y10_packed", 10)])
def test_dirty_bytes_do_not_change_a_bit(layout, bits):
    """high bits above D in y16_low, low bits below D in y16_msb, and the padding beyond W of a pitched row"""
    w, h = 61, 34
    ref, dis = U.pair(w, h, bits, "blurred", seed=5)
    clean = emul(w, h, layout, bits, ref, dis)
    for pad, dirty in ((9, 1), (1, 99)):
        got = emul(w, h, layout, bits, ref, dis, pad=pad, dirty=dirty)
        for s in range(4):
            assert got[s]["num"] == clean[s]["num"] and got[s]["den"] == clean[s]["den"]
            assert all(np.array_equal(a, b) for a, b in zip(got[s]["planes"], clean[s]["planes"]))
    if layout in ("y16_low", "y16_msb"):
        a, b = U.luma_plane(layout, ref, bits, dirty=1), U.luma_plane(layout, ref, bits)
        assert not np.array_equal(a, b)  # the dirty planes do differ in the bits the kernel must ignore


# ---- refusals, ABI, host function, binding, CLI -------------------------------------------------------------------------------
def test_refusals_match_the_restatement():
    z = np.zeros((64, 64), np.uint16)
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 12, 16, 17):
            for w, h in ((32, 32), (31, 32), (32, 31), (64, 40)):
                ok = R.supported(w, h, layout, bits)
                ws, hs = (C.c_int * 4)(), (C.c_int * 4)()
                assert (U.emul_lib().ve_sizes(w, h, U.LAYOUT[layout], bits, ws, hs) == 0) == ok, (layout, bits, w, h)
    assert U.emulate(31, 40, "y8", 8, z, z) is None


def test_create_refuses_before_touching_the_device():
    L = tm.vif.lib()
    h = C.c_void_p()
    for w, hh, lay, bits in ((31, 32, 0, 8), (32, 31, 0, 8), (64, 64, 0, 10), (64, 64, 1, 8), (64, 64, 1, 17), (64, 64, 3, 12), (64, 64, 4, 8), (64, 64, 2, 7)):
        assert L.tm_vif_create(C.byref(h), w, hh, lay, bits, 1) == tm.ffi.TM_ERR_UNSUPPORTED, (w, hh, lay, bits)
        assert h.value is None
    assert L.tm_vif_create(None, 64, 64, 0, 8, 1) == tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_vif_create(C.byref(h), 64, 64, 0, 8, 0) == tm.ffi.TM_ERR_INVALID_ARG
    assert h.value is None


def test_header_is_plain_c99_and_the_library_exports_exactly_it(tmp_path):
    want = declared("turbo_metrics_vif.h")
    assert len(want) == 8 and all(n.startswith("tm_vif") for n in want)
    assert exported(VLIB) == want
    assert sorted(tm.vif.SYMBOLS) == want
    src = tmp_path / "c.c"
    src.write_text('#include "turbo_metrics_vif.h"\n#include <stdio.h>\n'
                   "int main(void) { tm_vif *v = NULL; tm_vif_frame f; double o[5]; int s; (void)v;\n"
                   "  for (s = 0; s < 4; ++s) { f.num[s] = 1.0 + s; f.den[s] = 4.0; }\n"
                   "  tm_vif_scores(&f, o); printf(\"%.4f %.4f %.4f %.4f %.4f\\n\", o[0], o[1], o[2], o[3], o[4]); return 0; }\n")
    exe = str(tmp_path / "c")
    lib_dir = os.path.dirname(VLIB)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                           "-L" + lib_dir, "-lturbometrics_vif", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "0.2500 0.5000 0.7500 1.0000 0.6250", (out.returncode, out.stdout, out.stderr)


def test_the_other_libraries_are_unchanged_in_what_they_export():
    for lib in (tm.ffi.SHIP_LIB_PATH, tm.ffi.LIB_PATH, tm.xpsnr.LIB_PATH, tm.motion.LIB_PATH):
        assert not [n for n in exported(lib) if "vif" in n], lib
    assert not [n for n in tm.ffi.SYMBOLS if "vif" in n]
    assert exported(tm.motion.LIB_PATH) == declared("turbo_metrics_motion.h")


def test_scores_match_the_formula():
    rng = np.random.default_rng(4)
    for _ in range(100):
        den = rng.uniform(1.0, 1e7, 4)
        num = den * rng.uniform(0.0, 1.2, 4)
        per = [dict(num=float(n), den=float(d)) for n, d in zip(num, den)]
        got = tm.vif.scores(num, den)
        assert got == R.scores(per)
        assert got[:4] == [float(n) / float(d) for n, d in zip(num, den)]
        assert got[4] == (((0.0 + num[0]) + num[1]) + num[2] + num[3]) / (((0.0 + den[0]) + den[1]) + den[2] + den[3])
    assert tm.vif.scores([9.0, 4.0, 2.0, 1.0], [9.0, 4.0, 2.0, 1.0]) == [1.0] * 5


class _FakeLib:
    """stands in for the library under a Vif object: any call after the plane checks is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_binding_rejects_bad_planes_before_the_library():
    def obj(w, h, layout, bits):
        v = tm.Vif.__new__(tm.Vif)
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
    assert tm.Vif is tm.vif.Vif and tm.VifFrame is tm.vif.VifFrame


def test_cli_names_vif_and_refuses_what_it_cannot_do_before_touching_the_device(tmp_path):
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    for p in (a, b):
        with open(p, "wb") as f:
            f.write(b"YUV4MPEG2 W32 H32 F25:1 C420jpeg\nFRAME\n" + bytes(32 * 32 + 2 * 256))
    for extra in (["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
        for sel in ([], ["-m", "psnr"]):
            out = subprocess.run([CLI, a, b, "-m", "vif", *sel, *extra], capture_output=True, text=True, timeout=60)
            assert out.returncode != 0 and "-m vif does not run with" in out.stderr, (extra, out.returncode, out.stderr)
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "vif" in out.stdout
    out = subprocess.run([CLI, a, "-m", "vif"], capture_output=True, text=True, timeout=60)  # the distorted argument is still required
    assert out.returncode == 2 and "<DISTORTED>" in out.stderr
