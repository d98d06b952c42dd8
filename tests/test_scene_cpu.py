"""No-GPU tier of scene-cut detection (include/turbo_metrics_scene.h, libturbometrics_scene.so): the hand-derived answers of DESIGN.md
section 12 as literals against the library's host functions, the numpy restatement (tests/scene_ref.py) and the kernel SOURCE executed
lane by lane on the CPU (tests/scene_emul); emulated kernel == restatement, all 256 bins, on all four layouts, dirty bytes, tiny and
odd sizes, odd pitches, batches and repeated computes; create-time refusals; the ABI (C99 header, exports); the binding's checks; the
CLI's option parsing."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import scene_ref as R
from tests import scene_util as U
from tm_pkg import tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLIB = os.path.join(ROOT, "turbo-metrics_amd", "libturbometrics_scene.so")
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
S = tm.scene


def one_bin(b, n):
    h = np.zeros(256, np.uint32)
    h[b] = n
    return h


def emul_hists(w, h, layout, bits, pics, batches=None, pad=0, dirty=True, vec=None, aligned=False, cap=None):
    planes = [U.luma_plane(layout, Y, bits, pad=pad, dirty=(i + 1 if dirty else None)) for i, Y in enumerate(pics)]
    if aligned:
        planes = [U.aligned_copy(p) for p in planes]
    return U.emulate(w, h, layout, bits, batches or [len(pics)], planes, cap=cap, vec=vec)


def same(got, pics, bits):
    """every bin of every picture: nothing is left out of the comparison"""
    assert len(got) == len(pics)
    for g, Y in zip(got, pics):
        want = R.hist(Y, bits)
        assert g.dtype == np.uint32 and g.shape == (256,) and want.shape == (256,)
        assert int(g.astype(np.uint64).sum()) == Y.size
        assert (g == want).all(), np.flatnonzero(g != want)[:8]
    return True


# ---- the host functions, by hand -------------------------------------------------------------------------------------------
W, H = 48, 20
WH = W * H


def test_distance_score_and_verdict_by_hand():
    flat10, flat200 = one_bin(10, WH), one_bin(200, WH)
    for bins in R.BINS:
        assert S.distance(flat10, flat10, bins) == 0 == R.distance(flat10, flat10, bins)
        assert S.distance(flat10, flat200, bins) == 2 * WH == R.distance(flat10, flat200, bins)
    assert S.score(0, W, H) == 0.0 and S.score(2 * WH, W, H) == 1.0
    half = one_bin(10, WH // 2) + one_bin(200, WH // 2)
    assert S.distance(half, flat10) == WH == R.distance(half, flat10)
    s = S.score(WH, W, H)
    assert s == 0.5 == R.score(WH, W, H)
    assert S.is_cut(s, 0.5) and not S.is_cut(s, math.nextafter(0.5, 1.0))  # the >=
    assert not S.is_cut(math.nextafter(0.5, 0.0), 0.5)
    assert S.is_cut(0.5) and not S.is_cut(0.49)  # the default threshold


def test_the_merge_by_hand():
    a, b = one_bin(100, WH), one_bin(101, WH)  # both in merged bin 25 of 64
    assert S.distance(a, b, 256) == 2 * WH and S.distance(a, b, 64) == 0 and S.distance(a, b, 128) == 0
    # 103 | 104 straddle merged bins 25 | 26 of 64 (runs of 4) and 12 | 13 of 32 (runs of 8: 103 // 8 = 12, 104 // 8 = 13); the first
    # merge that puts them together is 16 (runs of 16: both in 6)
    a, b = one_bin(103, WH), one_bin(104, WH)
    assert S.distance(a, b, 64) == 2 * WH and S.distance(a, b, 32) == 2 * WH and S.distance(a, b, 256) == 2 * WH
    assert S.distance(a, b, 16) == 0 and S.distance(a, b, 8) == 0
    a, b = one_bin(100, WH), one_bin(103, WH)  # both in 25 of 64; apart at 128 (50 | 51)
    assert S.distance(a, b, 64) == 0 and S.distance(a, b, 32) == 0 and S.distance(a, b, 128) == 2 * WH
    a, b = one_bin(103, WH), one_bin(104, WH)
    # a merge by bin % bins would put 0 and 64 together, and 0 and 1 apart
    assert S.distance(one_bin(0, WH), one_bin(64, WH), 64) == 2 * WH and S.distance(one_bin(0, WH), one_bin(1, WH), 64) == 0
    assert S.distance(a, b) == S.distance(a, b, 64)  # the default
    for bins in (0, 7, 512, -64, 1, 4, 255):
        with pytest.raises(ValueError):
            S.distance(a, b, bins)
        out = C.c_uint64(77)
        p = a.ctypes.data_as(C.POINTER(C.c_uint32))
        assert S.lib().tm_scene_distance(p, p, bins, C.byref(out)) == tm.ffi.TM_ERR_INVALID_ARG and out.value == 77


def test_distance_adds_in_64_bits():
    full = np.full(256, 0xFFFFFFFF, np.uint32)
    zero = np.zeros(256, np.uint32)
    for bins in R.BINS:
        assert S.distance(full, zero, bins) == 256 * 0xFFFFFFFF == R.distance(full, zero, bins)
    assert S.score(1 << 32, 1 << 16, 1 << 15) == 1.0  # w h = 2^31: the product is taken in double


def test_host_functions_match_the_restatement_on_random_histograms():
    rng = np.random.default_rng(12)
    for _ in range(50):
        a, b = (rng.integers(0, 1 << 20, 256, dtype=np.uint64).astype(np.uint32) for _ in range(2))
        for bins in R.BINS:
            d = S.distance(a, b, bins)
            assert d == R.distance(a, b, bins)
            assert S.score(d, 1920, 1080) == R.score(d, 1920, 1080)
        assert S.stats(a) == R.stats(a)


def test_stats_by_hand():
    h = one_bin(10, 3) + one_bin(200, 1)
    assert S.stats(h) == (10, 200, (10 * 3 + 200) / 4) == (10, 200, 57.5)
    assert S.stats(one_bin(255, 1 << 31)) == (255, 255, 255.0)
    assert S.stats(one_bin(0, 5)) == (0, 0, 0.0)
    with pytest.raises(ValueError):
        S.stats(np.zeros(256, np.uint32))
    with pytest.raises(ValueError):
        S.stats(np.zeros(255, np.uint32))


def test_cuts_on_a_hand_built_sequence():
    a, b, c = one_bin(10, WH), one_bin(120, WH), one_bin(10, WH // 2) + one_bin(120, WH // 2)
    hists = [a, a, b, b, c, b, a]
    scores, flags = S.cuts(hists, W, H)
    assert scores == [0.0, 0.0, 1.0, 0.0, 0.5, 0.5, 1.0] and flags == [False, False, True, False, True, True, True]
    assert (scores, flags) == R.cuts(hists, W, H)
    assert S.cuts(hists, W, H, threshold=0.75)[1] == [False, False, True, False, False, False, True]
    assert S.cuts([b], W, H) == ([0.0], [False]) and S.cuts([], W, H) == ([], [])
    assert S.cuts([a, b], W, H, threshold=1.0)[1] == [False, True]
    # bins 10 and 11 share a merged bin at 64 and not at 256
    n = [one_bin(10, WH), one_bin(11, WH)]
    assert S.cuts(n, W, H)[0] == [0.0, 0.0] and S.cuts(n, W, H, bins=256) == ([0.0, 1.0], [False, True])


# ---- histograms, by hand -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,bits", U.CASES)
def test_flat_pictures_by_hand(layout, bits):
    w, h = 37, 5
    vals = [0, (1 << bits) - 1, 0x5A5A % (1 << bits), 1 << (bits - 8)]
    pics = [np.full((h, w), v, np.int64) for v in vals]
    got = emul_hists(w, h, layout, bits, pics)
    for v, g in zip(vals, got):
        assert (g == one_bin(v >> (bits - 8), w * h)).all(), v
        assert (R.hist(np.full((h, w), v), bits) == g).all()


@pytest.mark.parametrize("layout,bits", [("y8", 8), ("y16_msb", 10), ("y16_low", 10), ("y10_packed", 10)])
def test_ramp_by_hand(layout, bits):
    w, h = 1 << bits, 3  # sample = x mod 2^D on a width that is a multiple of 2^D: w h / 256 in every bin
    Y = np.tile(np.arange(w, dtype=np.int64) % (1 << bits), (h, 1))
    for g in emul_hists(w, h, layout, bits, [Y]) + emul_hists(w, h, layout, bits, [Y], aligned=True):
        assert (g == np.full(256, w * h // 256, np.uint32)).all()
    assert (R.hist(Y, bits) == w * h // 256).all()


def test_ramp_of_257_columns_by_hand():
    w, h = 257, 6
    Y = np.tile(np.arange(w, dtype=np.int64) % 256, (h, 1))
    want = np.full(256, h, np.uint32)
    want[0] = 2 * h
    for kw in ({}, {"aligned": True}, {"vec": False}):
        assert (emul_hists(w, h, "y8", 8, [Y], **kw)[0] == want).all()
    assert (R.hist(Y, 8) == want).all()


@pytest.mark.parametrize("layout,bits", U.CASES)
@pytest.mark.parametrize("w", [1, 2, 3, 5, 7])
def test_lanes_beyond_the_width_are_not_counted(layout, bits, w):
    h = 3
    M = (1 << bits) - 1
    Y = (np.indices((h, w)).sum(axis=0) % 3 + 1) * (M // 4)  # bins 63, 127, 191: nothing in bin 0
    assert (Y >> (bits - 8)).min() > 0
    for kw in ({"dirty": False}, {"dirty": True, "pad": 3}, {"aligned": True}):
        g = emul_hists(w, h, layout, bits, [Y], **kw)[0]
        assert g[0] == 0 and int(g.sum()) == w * h, kw
        assert (g == R.hist(Y, bits)).all()


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_a_full_scale_sample_in_each_corner(layout, bits):
    w, h = 70, 9
    M = (1 << bits) - 1
    base = 77 << (bits - 8)
    Y = np.full((h, w), base, np.int64)
    Y[0, 0] = Y[0, -1] = Y[-1, 0] = Y[-1, -1] = M
    want = one_bin(77, w * h - 4) + one_bin(255, 4)
    for kw in ({}, {"aligned": True}, {"pad": 1}):
        assert (emul_hists(w, h, layout, bits, [Y], **kw)[0] == want).all()
    assert (R.hist(Y, bits) == want).all()


# ---- emulated kernel == restatement --------------------------------------------------------------------------------------------
SIZES = [(1, 1), (3, 1), (1, 5), (5, 3), (63, 2), (64, 64), (65, 33), (255, 7), (257, 9), (1021, 3), (33, 517)]


def test_the_sizes_cover_more_than_one_band_and_more_than_one_pass_of_the_lanes():
    assert U.bands(33, 517, "y8", 8) > 1 and U.bands(64, 64, "y8", 8) == 1 and U.bands(1, 1, "y8", 8) == 1
    assert U.bands(1920, 1080, "y8", 8) > 8
    assert 1021 > 4 * 256 - 4  # the widest size needs every lane of the workgroup, and 257 / 1021 end in a partial group


@pytest.mark.parametrize("layout,bits", U.CASES)
@pytest.mark.parametrize("w,h", SIZES)
def test_emulated_kernel_matches_the_restatement(layout, bits, w, h):
    """the four contents as the four slots of one compute, dirty bits everywhere, on: whatever pitch the plane has (the library's
    alignment rule decides), an odd pitch, 16-byte aligned memory (the wide loads), and the sample-by-sample path forced"""
    pics = [U.picture(w, h, bits, k, seed=w + h) for k in U.KINDS]
    for kw in ({"pad": 0}, {"pad": 5 if layout != "y10_packed" else 1}, {"aligned": True}, {"vec": False, "pad": 3}):
        assert same(emul_hists(w, h, layout, bits, pics, **kw), pics, bits), kw


def test_emulated_kernel_at_1080p():
    w, h = 1920, 1080
    pics = [U.picture(w, h, 8, "smooth", seed=3)]
    assert same(emul_hists(w, h, "y8", 8, pics, aligned=True), pics, 8)


@pytest.mark.parametrize("layout,bits", [("y8", 8), ("y10_packed", 10), ("y16_msb", 12)])
def test_batches_come_back_in_slot_order(layout, bits):
    w, h = 65, 33
    for n in (1, 3, 8):
        pics = [U.picture(w, h, bits, U.KINDS[i % 4], seed=100 + i) for i in range(n)]
        assert len({R.hist(p, bits).tobytes() for p in pics}) == n  # distinct pictures, distinct answers
        assert same(emul_hists(w, h, layout, bits, pics, aligned=True), pics, bits)


@pytest.mark.parametrize("layout,bits", [("y8", 8), ("y16_low", 10)])
def test_a_second_compute_owes_nothing_to_the_first(layout, bits):
    w, h = 33, 300  # more than one band
    assert U.bands(w, h, layout, bits) > 1
    pics = [U.picture(w, h, bits, k, seed=s) for s, k in enumerate(("flat", "noise", "extreme", "smooth", "noise", "flat", "flat"))]
    # three computes into the same slots of one object: 3, 3 and 1 pictures (the last one leaves slots 1 and 2 alone)
    assert same(emul_hists(w, h, layout, bits, pics, batches=[3, 3, 1], cap=3), pics, bits)
    # and the same picture twice gives the same answer twice
    twice = emul_hists(w, h, layout, bits, [pics[1], pics[1]], batches=[1, 1], dirty=False)
    assert (twice[0] == twice[1]).all()


def test_refusals_match_the_restatement():
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 12, 16, 17):
            for w, h in ((0, 8), (8, 0), (1, 1), (8, 8), (1 << 16, 1 << 15), ((1 << 16) + 1, 1 << 15), (1 << 31, 1), ((1 << 31) + 1, 1)):
                assert (U.bands(w, h, layout, bits) > 0) == R.supported(w, h, layout, bits), (layout, bits, w, h)
    assert U.bands(8, 8, 7, 8) == 0 and U.bands(8, 8, -1, 8) == 0


# ---- the library without a device --------------------------------------------------------------------------------------------------
def test_create_refuses_before_touching_the_device():
    L = S.lib()
    h = C.c_void_p()
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 16, 17):
            for w, hh in ((0, 8), (8, 0), (0, 0), ((1 << 16) + 1, 1 << 15), (0xFFFFFFFF, 0xFFFFFFFF), (1 << 31, 2)):
                assert L.tm_scene_create(C.byref(h), w, hh, U.LAYOUT[layout], bits, 1) == tm.ffi.TM_ERR_UNSUPPORTED
            if not R.supported(8, 8, layout, bits):
                assert L.tm_scene_create(C.byref(h), 8, 8, U.LAYOUT[layout], bits, 1) == tm.ffi.TM_ERR_UNSUPPORTED
    assert L.tm_scene_create(C.byref(h), 8, 8, 7, 8, 1) == tm.ffi.TM_ERR_UNSUPPORTED
    assert L.tm_scene_create(None, 8, 8, 0, 8, 1) == tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_scene_create(C.byref(h), 8, 8, 0, 8, 0) == tm.ffi.TM_ERR_INVALID_ARG
    assert h.value is None


def declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(2) for m in re.finditer(r" ([A-Za-z]) (\S+)", out) if m.group(1) in "TDBRW" and not m.group(2).startswith(("_init", "_fini", "__bss", "_edata", "_end")))


def test_header_is_plain_c99_and_the_library_exports_exactly_it(tmp_path):
    want = declared("turbo_metrics_scene.h")
    assert len(want) == 11 and all(n.startswith("tm_scene") for n in want)
    assert exported(SLIB) == want
    assert sorted(S.SYMBOLS) == want
    listed = re.findall(r"^\s*(tm_[a-z0-9_]+);", open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "scene.map")).read(), flags=re.M)
    assert sorted(listed) == want
    assert [S.LAYOUTS[k] for k in ("y8", "y16_msb", "y16_low", "y10_packed")] == [0, 1, 2, 3] and S.LAYOUTS == tm.motion.LAYOUTS
    src = tmp_path / "c.c"
    src.write_text('#include "turbo_metrics_scene.h"\n#include "turbo_metrics_motion.h"\n#include <stdio.h>\n'
                   "int main(void) { tm_scene *s = NULL; static tm_scene_frame a, b; uint64_t d = 9; uint32_t lo, hi; double mean; (void)s;\n"
                   "  a.hist[100] = 6; b.hist[104] = 6;\n"
                   "  if ((int)TM_SCENE_Y8 != (int)TM_MOTION_Y8 || (int)TM_SCENE_Y16_MSB != (int)TM_MOTION_Y16_MSB ||\n"
                   "      (int)TM_SCENE_Y16_LOW != (int)TM_MOTION_Y16_LOW || (int)TM_SCENE_Y10_PACKED != (int)TM_MOTION_Y10_PACKED || sizeof a != 1024) return 3;\n"
                   "  if (tm_scene_distance(a.hist, b.hist, 7, &d) != TM_ERR_INVALID_ARG || d != 9) return 4;\n"
                   "  if (tm_scene_distance(a.hist, b.hist, TM_SCENE_DEFAULT_BINS, &d) || tm_scene_stats(b.hist, &lo, &hi, &mean)) return 5;\n"
                   "  printf(\"%llu %.2f %d %d %u %u %.1f\\n\", (unsigned long long)d, tm_scene_score(d, 3, 2), tm_scene_is_cut(0.5, TM_SCENE_DEFAULT_THRESHOLD),\n"
                   "         tm_scene_is_cut(0.25, 0.5), (unsigned)lo, (unsigned)hi, mean); return 0; }\n")
    exe = str(tmp_path / "c")
    lib_dir = os.path.dirname(SLIB)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                           "-L" + lib_dir, "-lturbometrics_scene", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "12 1.00 1 0 104 104 104.0", (out.returncode, out.stdout, out.stderr)


def test_the_other_libraries_are_unchanged_in_what_they_export():
    for lib in (tm.ffi.SHIP_LIB_PATH, tm.ffi.LIB_PATH, tm.xpsnr.LIB_PATH, tm.motion.LIB_PATH, tm.vif.LIB_PATH, tm.adm.LIB_PATH):
        assert not [n for n in exported(lib) if "scene" in n], lib
    assert not [n for n in tm.ffi.SYMBOLS if "scene" in n]
    assert exported(tm.motion.LIB_PATH) == declared("turbo_metrics_motion.h")


# ---- binding and CLI ---------------------------------------------------------------------------------------------------------------
class _FakeLib:
    """stands in for the library under a Scene object: any call after the plane checks is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_binding_rejects_bad_planes_before_the_library():
    def obj(w, h, layout, bits):
        m = tm.Scene.__new__(tm.Scene)
        m._L, m._h, m._keep = _FakeLib(), None, {}
        m.w, m.h, m.layout, m.bits, m.batch = w, h, layout, bits, 2
        return m
    m = obj(16, 8, "y8", 8)
    for bad in (np.zeros((8, 16), np.uint16), np.zeros((8, 16), np.int8), np.zeros((8, 16), np.float32), np.zeros((7, 16), np.uint8),
                np.zeros((8, 15), np.uint8), np.zeros((8, 32), np.uint8)[:, ::2], np.zeros(128, np.uint8), [[0] * 16] * 8):
        with pytest.raises(ValueError):
            m.set_frame(0, bad)
    with pytest.raises(ValueError):
        m.set_frame(2, np.zeros((8, 16), np.uint8))
    m = obj(16, 8, "y16_low", 10)
    for bad in (np.zeros((8, 16), np.uint8), np.zeros((8, 16), np.int64), np.zeros((8, 12), np.uint16)):
        with pytest.raises(ValueError):
            m.set_frame(0, bad)
    m = obj(400, 8, "y10_packed", 10)
    assert m.plane_shape() == ((8, 256), 4)
    for bad in (np.zeros((8, 400), np.uint16), np.zeros((8, 255), np.uint32)):
        with pytest.raises(ValueError):
            m.set_frame(0, bad)
    import torch
    m = obj(16, 8, "y16_msb", 10)
    for bad in (torch.zeros((8, 16), dtype=torch.uint8), torch.zeros((8, 16), dtype=torch.float16), torch.zeros((16, 8), dtype=torch.int16).t()):
        with pytest.raises(ValueError):
            m.set_frame(0, bad)
    with pytest.raises(ValueError):
        S.distance(np.zeros(255, np.uint32), np.zeros(256, np.uint32))
    assert tm.scene.Scene is tm.Scene and tm.SceneFrame is S.SceneFrame


def test_cli_names_scenes_and_refuses_what_it_cannot_do_before_touching_the_device(tmp_path):
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    for p in (a, b):
        with open(p, "wb") as f:
            f.write(b"YUV4MPEG2 W16 H16 F25:1 C420jpeg\nFRAME\n" + bytes(16 * 16 + 2 * 64))

    def run(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)
    for extra in (["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
        for sel in ([], ["-m", "psnr"], ["--motion"]):
            out = run(a, b, "--scenes", *sel, *extra)
            assert out.returncode != 0 and "--scenes does not run with" in out.stderr, (extra, out.returncode, out.stderr)
    out = run("--help")
    assert all(s in out.stdout for s in ("--scenes", "--scene-threshold <X>", "--scene-bins <N>", "--motion"))
    # the two values belong to --scenes
    for extra in (["--scene-threshold", "0.4"], ["--scene-bins", "32"], ["--scene-bins=32", "--scene-threshold=0.4"]):
        out = run(a, b, "-m", "psnr", *extra)
        assert out.returncode == 2 and "--scenes" in out.stderr, (extra, out.returncode, out.stderr)
    # the threshold lies in (0, 1], the bins are one of six values
    for v in ("0", "-0.5", "1.0000001", "2", "nan", "inf", "abc", "", "0.5x"):
        out = run(a, b, "--scenes", "--scene-threshold=" + v)
        assert out.returncode == 2 and "--scene-threshold" in out.stderr, (v, out.returncode, out.stderr)
    for v in ("0", "7", "512", "-64", "abc", "64.0", "1", "4"):
        out = run(a, b, "--scenes", "--scene-bins=" + v)
        assert out.returncode == 2 and "--scene-bins" in out.stderr, (v, out.returncode, out.stderr)
    for flag in ("--scene-threshold", "--scene-bins"):
        out = run(a, b, "--scenes", flag)
        assert out.returncode == 2 and flag in out.stderr
    out = run(a, "--scenes")  # the distorted argument is still required
    assert out.returncode == 2 and "<DISTORTED>" in out.stderr
    out = run(a, b, "-m", "scenes")  # a flag, not a value of -m
    assert out.returncode == 2 and "possible values: psnr, ssim, msssim, ssimulacra2" in out.stderr
