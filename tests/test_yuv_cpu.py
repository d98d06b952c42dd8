"""CPU tier of plane-wise YUV PSNR and SSIM: hand values of the definition, the kernel source run on the CPU
(tests/yuv_util.py) against the numpy restatement (tests/yuv_ref.py), state and order, refusals, the ABI, the binding, and seeded
mistakes in the restatement.

The criterion everywhere: `sse` equal, every map value bit-identical, each plane's `ssim_sum` within n 2^-53 sum |v| of the exactly
rounded sum (n: the plane's windows).  The bound is derived (yuv_ref.sum_bound), not measured."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import yuv_ref as R
from tests import yuv_util as U
from tm_pkg import tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y = tm.yuv
YLIB = Y.LIB_PATH
f32 = np.float32
T = U.tile()
E = 4 * (T + 1)  # samples at which a plane has exactly one tile of windows: T + 1 blocks
# the issue's sizes, then the tile edge -1 / 0 / +1 block in both directions: of the luma (E) and of the chroma planes (2 E)
SIZES = ((16, 16), (17, 17), (18, 16), (24, 16), (67, 35), (130, 70),
         (E - 4, E + 4), (E, E), (E + 4, E - 4), (2 * E - 8, 2 * E + 8), (2 * E, 2 * E), (2 * E + 8, 2 * E - 7))


def flat3(w, h, vals):
    shapes = ((h, w), ((h + 1) // 2, (w + 1) // 2), ((h + 1) // 2, (w + 1) // 2))
    return tuple(np.full(sh, v, np.int64) for sh, v in zip(shapes, vals))


def emul(w, h, layout, bits, pairs, batches=None, cap=None, **kw):
    vec = kw.pop("vec", None)
    return U.emulate(w, h, layout, bits, batches or [len(pairs)], U.frames_of(layout, pairs, w, h, bits, **kw), cap=cap, vec=vec)


def both(w, h, layout, bits, pairs, **kw):
    """the emulation's results after checking them against the restatement's"""
    got = emul(w, h, layout, bits, pairs, **kw)
    for i, (g, (a, b)) in enumerate(zip(got, pairs)):
        why = U.agrees(g, R.frame(a, b, bits))
        assert why is None, (i, why)
    return got


# ---- hand values ---------------------------------------------------------------------------------------------------------------
def test_constants():
    want = {8: (416, 235963), 10: (6698, 3797644), 12: (107322, 60851438), 16: (27486952, 15585101693)}
    for bits, (c1, c2) in want.items():
        mx = (1 << bits) - 1
        # the header's expression, and the same value from exact rational arithmetic: floor(x + 1/2)
        assert (c1, c2) == ((mx * mx * 64 * 2 + 10000) // 20000, (9 * mx * mx * 64 * 63 * 2 + 10000) // 20000)
        assert R.constants(bits) == (c1, c2) == U.constants(bits)


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_identical_pictures(layout, bits):
    w, h = 70, 37
    ref, _ = U.pair(w, h, bits, "noise", 3)
    g = both(w, h, layout, bits, [(ref, ref)])[0]
    assert g.sse == (0, 0, 0)
    for p in range(3):
        assert (g.maps[p].view(np.uint32) == f32(1.0).view(np.uint32)).all()
        assert g.ssim_sum[p] == g.maps[p].size
    assert R.psnr(0, w * h, bits) == math.inf == Y.psnr(0, w * h, bits)
    assert R.psnr(0, w * h, bits, 6 * bits + 12) == 6 * bits + 12 == Y.psnr(0, w * h, bits, Y.psnr_cap(bits))
    assert Y.ssim_db(1.0) == math.inf == R.ssim_db(1.0)


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_flat_pictures(layout, bits):
    w, h = 37, 70
    M = (1 << bits) - 1
    c1, c2 = R.constants(bits)
    for c, d in ((M // 3, M // 2), (1, 0), (M, M - 1), (0, M)):
        g = both(w, h, layout, bits, [(flat3(w, h, (c, c, d)), flat3(w, h, (d, c, c)))])[0]
        ns = (w * h, 19 * 35, 19 * 35)
        assert g.sse == (ns[0] * (c - d) ** 2, 0, ns[2] * (c - d) ** 2)
        # vars = covar = 0: the second factors are both (float)c2 and cancel exactly; what is left is one f32 quotient
        want = f32(2 * 64 * c * 64 * d + c1) * f32(c2) / (f32((64 * c) ** 2 + (64 * d) ** 2 + c1) * f32(c2))
        for p in (0, 2):
            assert (g.maps[p].view(np.uint32) == want.view(np.uint32)).all(), (c, d, p)
        assert (g.maps[1] == f32(1.0)).all()
    # 0 against max: c1 / (max^2 4096 + c1), to f32 rounding of the factors
    zero = f32(c1) * f32(c2) / (f32(M * M * 4096 + c1) * f32(c2))
    assert g.maps[0][0, 0] == zero and abs(float(zero) - c1 / (M * M * 4096 + c1)) <= 4 * 2.0 ** -24 * float(zero)


def test_checkerboard_against_its_inverse_is_negative():
    w, h = 32, 24
    yy, xx = np.indices((h, w))
    a = np.where((xx + yy) % 2 == 1, 255, 0).astype(np.int64)
    ref = (a, a[:h // 2, :w // 2], a[:h // 2, :w // 2])
    dis = tuple(255 - p for p in ref)
    g = both(w, h, "nv12", 8, [(ref, dis)])[0]
    assert (g.maps[0] < 0).all() and g.ssim_sum[0] < 0 and (g.maps[1] < 0).all()
    # s1 = s2 = 32 * 255, ss = 64 * 255^2, s12 = 0
    s = 32 * 255
    want = f32(2 * s * s + 416) * f32(2 * (0 - s * s) + 235963) / (f32(2 * s * s + 416) * f32(64 * 64 * 255 * 255 - 2 * s * s + 235963))
    assert g.maps[0][0, 0] == want


def test_single_samples_at_the_corners_and_beyond_the_last_block():
    w, h = 4 * 19 + 3, 4 * 18 + 2  # luma: 3 columns and 2 rows beyond the last block; chroma 40 x 37: 0 columns, 1 row
    ref, _ = U.pair(w, h, 8, "smooth", 5)
    ref = tuple(np.clip(p, 0, 200) for p in ref)
    base = both(w, h, "nv12", 8, [(ref, ref)])[0]
    spots = [(0, 0), (4 * 18 - 1, 4 * 19 - 1), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h - 1, 40), (30, w - 1), (h - 2, w - 3), (4 * 18, 0)]
    for k, (y, x) in enumerate(spots):
        dis = tuple(p.copy() for p in ref)
        dis[0][y, x] += 3 + k
        cx = x // 2
        dis[2][dis[2].shape[0] - 1, cx] += 2  # the chroma row beyond the last block
        g = both(w, h, "nv12", 8, [(ref, dis)])[0]
        assert g.sse == ((3 + k) ** 2, 0, 4), (y, x)
        inside = y < 4 * 18 and x < 4 * 19
        assert np.array_equal(g.maps[0], base.maps[0]) != inside, (y, x)  # beyond the blocks: SSIM untouched
        assert np.array_equal(g.maps[2], base.maps[2]) and g.ssim_sum[2] == base.ssim_sum[2]


def test_host_functions():
    L = Y.lib()
    for sse, n, bits, cap in ((1, 1, 8, 0), (12345, 1920 * 1080, 8, 0), (7, 640 * 480, 10, 72), (10 ** 12, 3840 * 2160, 16, 0), (1, 10 ** 7, 12, 84)):
        assert Y.psnr(sse, n, bits, cap) == R.psnr(sse, n, bits, cap)
    assert Y.psnr(255 * 255, 1, 8) == 0.0 and Y.psnr(1, 100, 8, 60.0) == 60.0
    for bits in (0, 7, 17, 64, 200):  # a depth the definition does not have: NaN, no shift by the depth
        assert math.isnan(Y.psnr(1, 1, bits)) and math.isnan(Y.psnr(0, 1, bits, 60.0)) and math.isnan(R.psnr(1, 1, bits))
    for s in (0.0, 0.5, 0.987654321, 1 - 2.0 ** -53, -0.25):
        assert Y.ssim_db(s) == R.ssim_db(s)
    for w, h in ((16, 16), (17, 35), (1920, 1080)):
        ns = (w * h, ((w + 1) // 2) * ((h + 1) // 2), ((w + 1) // 2) * ((h + 1) // 2))
        assert Y.ssim_all((0.9, 0.5, 0.25), w, h) == R.ssim_all((0.9, 0.5, 0.25), ns)
        assert Y.map_size(w, h, 0) == ((w >> 2) - 1, (h >> 2) - 1) and Y.map_size(w, h, 2) == ((((w + 1) // 2) >> 2) - 1, (((h + 1) // 2) >> 2) - 1)
    mw, mh = C.c_uint32(), C.c_uint32()
    assert L.tm_yuv_map_size(15, 16, 0, C.byref(mw), C.byref(mh)) == tm.ffi.TM_ERR_UNSUPPORTED
    assert L.tm_yuv_map_size(16, 16, 3, C.byref(mw), C.byref(mh)) == tm.ffi.TM_ERR_INVALID_ARG
    # the frame's average is plane-size weighted: the PSNR of the summed SSE over the summed samples
    assert R.psnr_avg((100, 10, 20), (64, 16, 16), 8) == Y.psnr(130, 96, 8)


# ---- emulation against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,bits", U.CASES)
@pytest.mark.parametrize("w,h", SIZES)
def test_emulated_kernel_matches_the_restatement(layout, bits, w, h):
    """the four contents as the four slots of one compute, dirty bits everywhere, on: whatever pitch the planes have (the library's
    alignment rule decides), 16-byte aligned memory (the wide loads), and the sample-by-sample path forced on padded rows"""
    pairs = [U.pair(w, h, bits, k, seed=w + h) for k in U.KINDS]
    a = both(w, h, layout, bits, pairs)
    b = both(w, h, layout, bits, pairs, aligned=True)
    c = both(w, h, layout, bits, pairs, vec=False, pad=3 if layout != "i420p10" else 1)
    for x, y, z in zip(a, b, c):
        assert x.ssim_sum == y.ssim_sum == z.ssim_sum  # the same order on every path


def test_emulated_kernel_at_1080p():
    w, h = 1920, 1080
    pairs = [U.pair(w, h, 8, "smooth", seed=3)]
    g = both(w, h, "nv12", 8, pairs, aligned=True)[0]
    assert 0 < g.ssim_sum[0] < g.maps[0].size and g.maps[0].shape == (269, 479)


# ---- state and order --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,bits", [("nv12", 8), ("i420p10", 10), ("p016", 12)])
def test_batches_come_back_in_slot_order(layout, bits):
    w, h = 2 * E + 8, 35
    for n in (1, 3, 8):
        pairs = [U.pair(w, h, bits, U.KINDS[i % 3], seed=100 + i) for i in range(n)]
        got = both(w, h, layout, bits, pairs, aligned=True)
        assert len({g.sse for g in got}) == n  # distinct pairs, distinct answers


@pytest.mark.parametrize("layout,bits", [("nv12", 8), ("i420", 10)])
def test_a_second_compute_owes_nothing_to_the_first(layout, bits):
    w, h = 2 * E + 9, E + 5  # several tiles in the luma
    assert U.geom(w, h, layout, bits)[2] > 2
    pairs = [U.pair(w, h, bits, k, seed=s) for s, k in enumerate(("flat", "noise", "extreme", "smooth", "noise", "flat", "flat"))]
    # three computes into the same slots of one object: 3, 3 and 1 pairs (the last one leaves slots 1 and 2 alone)
    both(w, h, layout, bits, pairs, batches=[3, 3, 1], cap=3)
    twice = emul(w, h, layout, bits, [pairs[1], pairs[1]], batches=[1, 1], dirty=False)
    assert twice[0].sse == twice[1].sse and twice[0].ssim_sum == twice[1].ssim_sum
    assert all(np.array_equal(a, b) for a, b in zip(twice[0].maps, twice[1].maps))


def test_slot_5_of_8_behaves_like_slot_0_of_1():
    w, h = 130, 70
    pairs = [U.pair(w, h, 8, U.KINDS[i % 4], seed=20 + i) for i in range(8)]
    eight = both(w, h, "nv12", 8, pairs)
    one = both(w, h, "nv12", 8, [pairs[5]])[0]
    assert eight[5].sse == one.sse and eight[5].ssim_sum == one.ssim_sum and all(np.array_equal(a, b) for a, b in zip(eight[5].maps, one.maps))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
GEOMS = ((0, 16), (16, 0), (15, 16), (16, 15), (16, 16), (17, 31), (32768, 16), (32769, 16), (16, 32769), (1 << 31, 16))


def test_refusals_match_the_restatement():
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 12, 16, 17):
            for w, h in GEOMS:
                assert (U.geom(w, h, layout, bits) is not None) == R.supported(w, h, layout, bits), (layout, bits, w, h)
    assert U.geom(16, 16, 4, 8) is None and U.geom(16, 16, -1, 8) is None


def test_create_refuses_before_touching_the_device():
    L = Y.lib()
    h = C.c_void_p()
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 12, 16, 17):
            for w, hh in GEOMS + ((0xFFFFFFFF, 0xFFFFFFFF),):
                if not R.supported(w, hh, layout, bits):
                    assert L.tm_yuv_create(C.byref(h), w, hh, U.LAYOUT[layout], bits, 1) == tm.ffi.TM_ERR_UNSUPPORTED, (layout, bits, w, hh)
    assert L.tm_yuv_create(C.byref(h), 16, 16, 7, 8, 1) == tm.ffi.TM_ERR_UNSUPPORTED
    assert L.tm_yuv_create(None, 16, 16, 0, 8, 1) == tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_yuv_create(C.byref(h), 16, 16, 0, 8, 0) == tm.ffi.TM_ERR_INVALID_ARG
    assert h.value is None


# ---- ABI --------------------------------------------------------------------------------------------------------------------------
def declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(2) for m in re.finditer(r" ([A-Za-z]) (\S+)", out) if m.group(1) in "TDBRW" and not m.group(2).startswith(("_init", "_fini", "__bss", "_edata", "_end")))


def test_header_is_plain_c99_and_the_library_exports_exactly_it(tmp_path):
    want = declared("turbo_metrics_yuv.h")
    assert len(want) == 12 and all(n.startswith("tm_yuv") for n in want)
    assert exported(YLIB) == want
    assert sorted(Y.SYMBOLS) == want
    listed = re.findall(r"^\s*(tm_[a-z0-9_]+);", open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "yuv.map")).read(), flags=re.M)
    assert sorted(listed) == want
    assert Y.LAYOUTS == tm.xpsnr.LAYOUTS
    src = tmp_path / "c.c"
    src.write_text('#include "turbo_metrics_yuv.h"\n#include "turbo_metrics_xpsnr.h"\n#include <stdio.h>\n'
                   "int main(void) { tm_yuv *s = NULL; tm_yuv_frame f; uint32_t mw, mh; double q[3] = {1.0, 0.5, 0.5}; (void)s; (void)f;\n"
                   "  if ((int)TM_YUV_NV12 != (int)TM_XPSNR_NV12 || (int)TM_YUV_P016 != (int)TM_XPSNR_P016 || (int)TM_YUV_I420 != (int)TM_XPSNR_I420 ||\n"
                   "      (int)TM_YUV_I420P10_PACKED != (int)TM_XPSNR_I420P10_PACKED || sizeof f != 72) return 3;\n"
                   "  if (tm_yuv_map_size(1920, 1080, 0, &mw, &mh)) return 4;\n"
                   "  printf(\"%u %u %.4f %.4f %.4f %.4f\\n\", (unsigned)mw, (unsigned)mh, tm_yuv_psnr(65025, 1, 8, 0), tm_yuv_psnr(1, 1, 8, 60), tm_yuv_ssim_db(0.9),\n"
                   "         tm_yuv_ssim_all(q, 16, 16)); return 0; }\n")
    exe = str(tmp_path / "c")
    lib_dir = os.path.dirname(YLIB)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                           "-L" + lib_dir, "-lturbometrics_yuv", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "479 269 0.0000 48.1308 10.0000 0.8333", (out.returncode, out.stdout, out.stderr)


def test_the_other_libraries_are_unchanged_in_what_they_export():
    for lib in (tm.ffi.SHIP_LIB_PATH, tm.ffi.LIB_PATH, tm.xpsnr.LIB_PATH, tm.motion.LIB_PATH, tm.vif.LIB_PATH, tm.adm.LIB_PATH, tm.scene.LIB_PATH,
                tm.cambi.LIB_PATH, tm.flip.LIB_PATH):
        assert not [n for n in exported(lib) if "tm_yuv" in n], lib
    assert exported(tm.xpsnr.LIB_PATH) == declared("turbo_metrics_xpsnr.h")


# ---- binding ----------------------------------------------------------------------------------------------------------------------
class _FakeLib:
    """stands in for the library under a Yuv object: any call after the plane checks is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_binding_rejects_bad_planes_before_the_library():
    def obj(w, h, layout, bits):
        m = tm.Yuv.__new__(tm.Yuv)
        m._L, m._h, m._keep = _FakeLib(), None, {}
        m.w, m.h, m.layout, m.bits, m.batch = w, h, layout, bits, 2
        return m
    m = obj(16, 16, "nv12", 8)
    y, uv = np.zeros((16, 16), np.uint8), np.zeros((8, 16), np.uint8)
    for bad in ((y,), (y, uv, uv), (y.astype(np.uint16), uv), (y, uv.astype(np.float32)), (y[:15], uv), (y, uv[:, :15]), (y, np.zeros((8, 32), np.uint8)[:, ::2]),
                (np.zeros(256, np.uint8), uv), ([[0] * 16] * 16, uv), (y.astype(np.int8), uv)):
        with pytest.raises(ValueError):
            m.set_frame(0, 0, bad)
    m = obj(17, 17, "i420", 10)
    y, c = np.zeros((17, 17), np.uint16), np.zeros((9, 9), np.uint16)
    for bad in ((y, c), (y, c, c.astype(np.uint8)), (y, c, np.zeros((9, 8), np.uint16)), (y, c, np.zeros((8, 9), np.uint16)), (y.astype(np.int64), c, c)):
        with pytest.raises(ValueError):
            m.set_frame(0, 1, bad)
    m = obj(400, 16, "i420p10", 10)
    assert m._plane_shapes() == ([(16, 256), (8, 128), (8, 128)], 4)
    with pytest.raises(ValueError):
        m.set_frame(0, 0, (np.zeros((16, 400), np.uint16), np.zeros((8, 128), np.uint32), np.zeros((8, 128), np.uint32)))
    import torch
    m = obj(16, 16, "p016", 10)
    for bad in ((torch.zeros((16, 16), dtype=torch.uint8), torch.zeros((8, 16), dtype=torch.int16)),
                (torch.zeros((16, 16), dtype=torch.int16), torch.zeros((16, 8), dtype=torch.int16).t())):
        with pytest.raises(ValueError):
            m.set_frame(0, 0, bad)
    with pytest.raises(ValueError):
        m.ssim_map(0, 3)
    assert tm.yuv.Yuv is tm.Yuv and tm.YuvFrame is Y.YuvFrame


# ---- seeded mistakes --------------------------------------------------------------------------------------------------------------
def _moved(mistake):
    """does the mistake move some test picture beyond the criterion?"""
    for (w, h), bits, kind in (((67, 35), 8, "smooth"), ((67, 35), 8, "noise"), ((130, 70), 10, "smooth")):
        a, b = U.pair(w, h, bits, kind, seed=9)
        right = R.frame(a, b, bits)
        cw, ch = R.chroma_size(w, h, mistake)
        a2, b2 = ((p[0], p[1][:ch, :cw], p[2][:ch, :cw]) for p in (a, b))
        wrong = R.frame(a2, b2, bits, mistake)
        for r, x in zip(right, wrong):
            if r.sse != x.sse or r.map.shape != x.map.shape or not np.array_equal(r.map.view(np.uint32), x.map.view(np.uint32)):
                return True
            if not abs(r.ssim_sum - x.ssim_sum) <= R.sum_bound(r):
                return True
    return False


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_seeded_mistakes_are_caught(mistake):
    assert _moved(mistake)


def test_no_mistake_moves_nothing():
    assert not _moved(None)


# ---- CLI --------------------------------------------------------------------------------------------------------------------------
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
    assert out.returncode == 0 and all(s in out.stdout for s in ("-m psnr-yuv", "-m ssim-yuv", "--psnr-yuv-cap", "--ssim-yuv-map <PREFIX>", "vif, adm, cambi, flip, psnr-yuv, ssim-yuv]"))
    for sel in (["-m", "psnr-yuv"], ["-m", "ssim-yuv"], ["-mpsnr-yuv", "-m", "ssim-yuv", "-m", "psnr"], ["--metrics", "ssim-yuv", "--motion"]):
        for extra in (["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
            out = run(a, b, *sel, *extra)
            assert out.returncode != 0 and "-m psnr-yuv / ssim-yuv do not run with" in out.stderr, (sel, extra, out.returncode, out.stderr)
    # usage errors: exit code 2
    for bad in ("psnr_yuv", "yuv", "psnr-yuv,ssim-yuv", "PSNR-YUV"):
        for form in (["-m", bad], ["-m" + bad], ["--metrics", bad]):
            out = run(a, b, *form)
            assert out.returncode == 2 and VALUES in out.stderr and f"'{bad}'" in out.stderr, (form, out.returncode, out.stderr)
    for args, word in ((["-m", "psnr", "--psnr-yuv-cap"], "-m psnr-yuv"), (["-m", "ssim-yuv", "--psnr-yuv-cap"], "-m psnr-yuv"),
                       (["-m", "psnr-yuv", "--ssim-yuv-map", "x"], "-m ssim-yuv"), (["--ssim-yuv-map=x", "-m", "xpsnr"], "-m ssim-yuv"),
                       (["-m", "ssim-yuv", "--ssim-yuv-map"], "--ssim-yuv-map <PREFIX>"), (["-m", "ssim-yuv", "--ssim-yuv-map="], "--ssim-yuv-map <PREFIX>")):
        out = run(a, b, *args)
        assert out.returncode == 2 and word in out.stderr, (args, out.returncode, out.stderr)
    out = run(a, "-m", "psnr-yuv")  # the distorted argument is still required
    assert out.returncode == 2 and "<DISTORTED>" in out.stderr
