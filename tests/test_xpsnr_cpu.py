"""No-GPU tier of XPSNR (include/turbo_metrics_xpsnr.h, libturbometrics_xpsnr.so): the paper checks of the definition against the CPU
restatement (tests/xpsnr_ref.py), the library's host functions against the restatement, create-time rejections before any device
call, the ABI (C99 header, exports), and the kernel SOURCE executed lane by lane on the CPU (tests/xpsnr_emul) bit-exact against the
restatement."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import xpsnr_ref as R
from tests import xpsnr_util as U
from tm_pkg import tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XLIB = os.path.join(ROOT, "turbo-metrics_amd", "libturbometrics_xpsnr.so")


def declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(2) for m in re.finditer(r" ([A-Za-z]) (\S+)", out) if m.group(1) in "TDBRW" and not m.group(2).startswith(("_init", "_fini", "__bss", "_edata", "_end")))


def flat(w, h, v, bits=8):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return (np.full((h, w), v, np.int64), np.full((ch, cw), v, np.int64), np.full((ch, cw), v, np.int64))


def test_paper_checks_1080p():
    """1920x1080, 8-bit, ref all 128, dis all 130, 25 fps (first order).  b = 64, bval = 1, avg_act = sqrt(16 * 2^7 / sqrt(0.25)) = 64.

    Frame 1 (history all zero): a flat picture has no spatial activity (the active windows keep every tap inside the picture), and
    ta = 2 * sum |128 - 0| over a block, so ms = ta / area = 2 * 128 = 256 > 2^(8-6) = 4; ms^2 = 65536, w = 1 / 256 for every block.
    wsse = sum sse * w = (1920 * 1080 * 2^2) / 256 = 32400, times avg_act 64 = 2 073 600.  XPSNR_y = 10 log10(1920 * 1080 * 255^2 /
    2073600) = 10 log10(65025) = 48.131 dB; PSNR = 10 log10(255^2 / 4) = 42.110 dB, so XPSNR = PSNR + 6.02 dB (the weight 1/256 against
    avg_act 64 is a factor 1/4 on the SSE).

    Frame 2 (the same pictures again): m1 = the reference, ta = 0, ms = 0 is clamped to 4, w = 1/4, wsse = sse / 4 * 64 = 16 sse
    = 16 * 8 294 400 = 132 710 400: XPSNR = PSNR - 10 log10(16) = PSNR - 12.04 dB."""
    w, h = 1920, 1080
    assert R.block_size(w, h) == 64 and R.avg_act(w, h, 8) == 64.0 and R.bval_of(w, h) == 1
    seq = R.Sequence(w, h, 8, (25, 1))
    ref, dis = flat(w, h, 128), flat(w, h, 130)
    (w1, s1), (w2, s2) = seq.push(ref, dis), seq.push(ref, dis)
    sse = w * h * 4
    psnr = 10 * math.log10(255 ** 2 / 4)
    assert w1[0] == 2073600 and abs(s1[0] - 10 * math.log10(65025)) < 1e-12 and abs(s1[0] - 48.131) < 5e-4
    assert abs(s1[0] - psnr - 10 * math.log10(4)) < 1e-9
    assert w2[0] == 16 * sse == 132710400
    assert abs(s2[0] - (psnr - 10 * math.log10(16))) < 1e-9
    # the library's dB functions on the same numbers
    assert tm.xpsnr.from_wsse(w1[0], w, h, 8) == s1[0] and tm.xpsnr.from_wsse(w2[0], w, h, 8) == s2[0]


def test_block_size_and_db_functions_match_the_restatement():
    sizes = [(8, 8), (40, 40), (44, 46), (45, 45), (64, 48), (97, 61), (176, 144), (640, 480), (641, 480), (1279, 719), (1280, 720),
             (1920, 1080), (2048, 1152), (2050, 1152), (2400, 1000), (3840, 2160), (4096, 2160), (7680, 4320), (1, 5000000)]
    for w, h in sizes:
        assert tm.xpsnr.block_size(w, h) == R.block_size(w, h), (w, h)
    assert [R.block_size(*s) for s in ((1920, 1080), (3840, 2160), (640, 480), (40, 40))] == [64, 128, 24, 0]
    rng = np.random.default_rng(5)
    for bits in range(8, 17):
        for pw, ph in ((1920, 1080), (960, 540), (20, 20), (640, 480), (3840, 2160)):
            for wsse in [0, 1, 2, 3, 1000] + [int(v) for v in rng.integers(1, 2 ** 62, 20)]:
                assert tm.xpsnr.from_wsse(wsse, pw, ph, bits) == R.from_wsse(wsse, pw, ph, bits), (wsse, pw, ph, bits)
            for n in (1, 2, 9, 1000):
                for s in (0.0, 0.5 * n, float(n), n * 1234.5678, float(rng.random() * 1e9)):
                    x = float(rng.random() * 100 * n)
                    got, want = tm.xpsnr.sequence(s, x, n, pw, ph, bits), R.sequence(s, x, n, pw, ph, bits)
                    assert got == want, (s, x, n, pw, ph, bits)
    assert math.isinf(tm.xpsnr.from_wsse(0, 64, 64, 8))


def test_create_rejects_bad_arguments_before_touching_the_device():
    """every refusal happens in host arithmetic, before the first HIP call (this tier has no device: a HIP call would fail with
    TM_ERR_HIP instead)"""
    L = tm.xpsnr.lib()
    h = C.c_void_p()
    NV12, P016, I420, P10 = 0, 1, 2, 3
    inv, uns = tm.ffi.TM_ERR_INVALID_ARG, tm.ffi.TM_ERR_UNSUPPORTED
    assert L.tm_xpsnr_create(None, 64, 64, NV12, 8, 25, 1, 1) == inv
    assert L.tm_xpsnr_create(C.byref(h), 0, 64, NV12, 8, 25, 1, 1) == inv
    assert L.tm_xpsnr_create(C.byref(h), 64, 64, NV12, 8, 0, 1, 1) == inv
    assert L.tm_xpsnr_create(C.byref(h), 64, 64, NV12, 8, 25, 0, 1) == inv
    assert L.tm_xpsnr_create(C.byref(h), 64, 64, NV12, 8, 25, 1, 0) == inv
    assert L.tm_xpsnr_create(C.byref(h), 7, 64, I420, 8, 25, 1, 1) == uns       # W below 8
    assert L.tm_xpsnr_create(C.byref(h), 64, 7, I420, 8, 25, 1, 1) == uns       # H below 8
    assert L.tm_xpsnr_create(C.byref(h), 64, 64, I420, 7, 25, 1, 1) == uns      # depth below 8
    assert L.tm_xpsnr_create(C.byref(h), 64, 64, I420, 17, 25, 1, 1) == uns     # depth above 16
    assert L.tm_xpsnr_create(C.byref(h), 64, 64, NV12, 10, 25, 1, 1) == uns     # NV12 is 8-bit
    assert L.tm_xpsnr_create(C.byref(h), 64, 64, P016, 8, 25, 1, 1) == uns      # P016 is 9..16-bit
    assert L.tm_xpsnr_create(C.byref(h), 64, 64, P10, 12, 25, 1, 1) == uns      # the packed kind is 10-bit
    assert L.tm_xpsnr_create(C.byref(h), 64, 64, 4, 8, 25, 1, 1) == uns         # no such layout
    assert L.tm_xpsnr_create(C.byref(h), 3841, 2160, I420, 8, 25, 1, 1) == uns  # odd W with bval = 2
    assert L.tm_xpsnr_create(C.byref(h), 2400, 1001, I420, 8, 25, 1, 1) == uns  # odd H with bval = 2
    assert L.tm_xpsnr_create(C.byref(h), 2 * 7680, 2 * 4320, I420, 8, 25, 1, 1) == uns  # block size above 256
    assert h.value is None
    # odd sizes stay legal where the high-pass is not downsampled
    assert R.bval_of(1279, 719) == 1 and R.bval_of(2049, 1151) == 1


def test_header_is_plain_c99_and_the_library_exports_exactly_it(tmp_path):
    want = declared("turbo_metrics_xpsnr.h")
    assert len(want) == 11 and all(n.startswith("tm_xpsnr_") for n in want)
    assert exported(XLIB) == want
    src = tmp_path / "c.c"
    src.write_text('#include "turbo_metrics_xpsnr.h"\n#include <stdio.h>\n'
                   "int main(void) { tm_xpsnr *x = NULL; tm_xpsnr_frame f; f.wsse[0] = 0; (void)x;\n"
                   "  printf(\"%u %.4f\\n\", tm_xpsnr_block_size(1920, 1080), tm_xpsnr_from_wsse(2073600, 1920, 1080, 8)); return (int)f.wsse[0]; }\n")
    exe = str(tmp_path / "c")
    lib_dir = os.path.dirname(XLIB)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                           "-L" + lib_dir, "-lturbometrics_xpsnr", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "64 48.1308", (out.returncode, out.stdout, out.stderr)


def test_the_engine_libraries_carry_no_xpsnr_symbol():
    for lib in (tm.ffi.SHIP_LIB_PATH, tm.ffi.LIB_PATH):
        assert not [n for n in exported(lib) if "xpsnr" in n], lib
    assert not [n for n in tm.ffi.SYMBOLS if "xpsnr" in n]
    assert sorted(tm.xpsnr.SYMBOLS) == declared("turbo_metrics_xpsnr.h")


def test_the_rust_binding_in_integration_md_is_the_xpsnr_header():
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = txt[txt.index("pub fn tm_xpsnr_create") - 40:]
    block = block[:block.index("\n}\n")]
    assert sorted(set(re.findall(r"pub fn (tm_xpsnr_[a-z0-9_]+)\(", block))) == declared("turbo_metrics_xpsnr.h")


def _emulated_against_restatement(w, h, layout, bits, fps, batches, pad=0, kind="synth", dirty=False):
    n = sum(batches)
    seq = R.Sequence(w, h, bits, fps)
    frames, want = [], []
    for i in range(n):
        ref, dis = U.pictures(w, h, i, bits, kind)
        want.append(seq.push(ref, dis)[0])
        frames.append(tuple(U.layout_planes(layout, p, w, h, bits, pad, dirty=U.dirt_seed(i, side) if dirty else None)
                            for side, p in enumerate((ref, dis))))
    got = U.emulate(w, h, layout, bits, fps, batches, frames)
    assert got == want, (w, h, layout, bits, fps, batches, kind, dirty, got, want)
    return want


@pytest.mark.parametrize("w,h,layout,bits,fps,batches,pad", [
    (64, 48, "nv12", 8, (25, 1), [2, 1, 2], 0),          # b = 4: the smallest blocks, minimum smoothing, first order
    (64, 48, "nv12", 8, (60, 1), [1, 3, 1], 4),          # second order across launches of 1 (m2 from the history's m1)
    (176, 144, "i420", 10, (50, 1), [3, 2], 0),          # 16-bit words with the value in the low bits, second order
    (97, 61, "i420", 8, (25, 1), [2, 2], 3),             # odd sizes (bval = 1), unaligned rows: the per-sample loads
    (130, 66, "i420p10", 10, (60, 1), [3], 0),           # the packed 10-bit kind
    (200, 120, "p016", 10, (30000, 1001), [1, 1, 1], 0), # P016; 29.97 fps is first order
    (40, 40, "nv12", 8, (25, 1), [2, 1], 0),             # b < 4: plain SSE
    (150, 90, "p016", 12, (25, 1), [2], 8),              # P016 at 12 bits
    (1280, 720, "i420p10", 10, (25, 1), [1], 0),         # chroma blocks of 22 columns: groups of 4 not at a block edge, across runs
    (854, 480, "i420p10", 10, (60, 1), [1, 1], 0),       # chroma blocks of 14 columns
    (1280, 720, "nv12", 8, (25, 1), [1], 0),             # the same chroma grid through the interleaved loads
    (2048, 1152, "nv12", 8, (25, 1), [1], 0),            # exactly 2048 x 1152: still bval = 1
    (2050, 1152, "i420", 10, (25, 1), [1], 2),           # two columns more: bval = 2, w % 4 == 2
    (45, 45, "nv12", 8, (31, 1), [1, 1], 0),             # the temporal order at its boundary: 31 fps is first order
    (45, 45, "nv12", 8, (32, 1), [1, 1], 0),             # 32 fps is second order
    (45, 45, "i420", 10, (63, 2), [2], 0),               # 31.5 fps: the integer rate 31, first order
    (45, 45, "i420", 10, (64, 2), [2], 0),               # 32.0 fps, second order
    (45, 45, "p016", 10, (60000, 1001), [1, 1], 0),      # 59.94 fps, second order
    (65, 49, "i420", 8, (25, 1), [2], 0),                # b = 4: the last block column and row cropped to 1 sample (empty window)
    (66, 50, "nv12", 8, (60, 1), [2], 0),                # cropped to 2 samples
])
def test_emulated_kernels_match_the_restatement(w, h, layout, bits, fps, batches, pad):
    _emulated_against_restatement(w, h, layout, bits, fps, batches, pad)


def test_emulated_kernels_downsampled_highpass():
    """bval = 2 (w h > 2048 x 1152) on a 2400 x 1000 strip: the `highds` taps, 2x2-cell temporal activity, 2-sample halos; first and
    second order"""
    _emulated_against_restatement(2400, 1000, "nv12", 8, (25, 1), [2, 1])
    _emulated_against_restatement(2400, 1000, "i420", 10, (50, 1), [1, 2], pad=2)


def test_emulated_kernels_640x480_smoothing():
    w = _emulated_against_restatement(640, 480, "i420", 8, (25, 1), [2])
    assert all(v[0] > 0 for v in w)


def test_cli_refuses_what_xpsnr_cannot_do_before_touching_the_device(tmp_path):
    """`-m xpsnr` is stateful across one sequence on one device: --every > 1, --devices, --ranks and the one-pair loops are refused at
    parse time, with a message that names xpsnr and a non-zero exit"""
    cli = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    for p in (a, b):
        with open(p, "wb") as f:
            f.write(b"YUV4MPEG2 W16 H16 F25:1 C420jpeg\nFRAME\n" + bytes(16 * 16 + 2 * 64))
    for extra in (["--every", "2"], ["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
        out = subprocess.run([cli, a, b, "-m", "xpsnr", *extra], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "xpsnr" in out.stderr, (extra, out.returncode, out.stderr)
    out = subprocess.run([cli, a, b, "-m", "xpsnr", "--xpsnr-fps", "0"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--xpsnr-fps" in out.stderr
    out = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert "ssimulacra2, xpsnr]" in out.stdout and "--xpsnr-fps" in out.stdout


# ---- known answers derived by hand, the second restatement, dirty bytes, geometry edges, the binding's checks -------------------
from tests import xpsnr_twin as T  # noqa: E402


def _both(w, h, bits, fps, pics):
    """the restatement and the twin over one sequence: they must agree frame for frame and on the sequence scores"""
    a, b = R.Sequence(w, h, bits, fps), T.Sequence(w, h, bits, fps)
    out = []
    for ref, dis in pics:
        x, y = a.push(ref, dis), b.push(ref, dis)
        assert x == y, (w, h, bits, fps, x, y)
        out.append(x)
    assert a.sequence_scores() == b.sequence_scores()
    return out, a.sequence_scores()


def _emulate_pics(w, h, layout, bits, fps, batches, pics, pad=0, dirty=False):
    return U.emulate(w, h, layout, bits, fps, batches, [
        tuple(U.layout_planes(layout, p, w, h, bits, pad, dirty=U.dirt_seed(i, side) if dirty else None) for side, p in enumerate(pair))
        for i, pair in enumerate(pics)])


@pytest.mark.parametrize("bits", [8, 10])
def test_known_answer_checkerboard_bval1(bits):
    """480 x 270 (r = 1/64): b = 4 (int)(32 / 8 + 0.5) = 16, bval = 1, avg_act = sqrt(16 * 2^(2D-9) * 8) = 2^(D-1); 30 x 17 blocks, the
    last row 14 high; chroma 240 x 135 in blocks of 8 x 8.  Reference: the 0 / M checkerboard (M = 2^D - 1 where x + y is odd) in
    every plane, the same every frame; distorted: M - reference, so every sample's error is M and sse = M^2 per sample.

    High-pass at a sample of value M: 12 M - 2 (4 direct neighbours, all 0) - (4 diagonal ones, all M) = 8 M; at a 0: -2 * 4 M = -8 M.
    So |f| = 8 M wherever the window lets it be evaluated, and sa / window area = 8 M in every block.  Frame 1 (history 0):
    ta = 2 sum |o| = 2 M (area / 2) (every block has even sides), ta / area = M, ms = 9 M > 2^(D-6), w = 1 / (9 M) in every block
    (equal weights: the minimum smoothing of this 129 600-sample picture changes nothing).  Frame 2 (m1 = the same picture): ta = 0,
    ms = 8 M, w = 1 / (8 M).  wsse = W H M^2 w avg_act:
      Y  frame 1: 129600 M 2^(D-1) / 9 = 14400 M 2^(D-1); frame 2: 129600 M 2^(D-1) / 8 = 16200 M 2^(D-1)
      Cb, Cr (32 400 samples): 3600 M 2^(D-1) and 4050 M 2^(D-1).
    D = 8: 470 016 000 / 117 504 000, then 528 768 000 / 132 192 000."""
    w, h, M, aa = 480, 270, (1 << bits) - 1, 1 << (bits - 1)
    assert R.block_size(w, h) == 16 and R.bval_of(w, h) == 1 and R.avg_act(w, h, bits) == aa
    pics = [U.pictures(w, h, n, bits, "checker") for n in range(2)]
    want = [(14400 * M * aa, 3600 * M * aa, 3600 * M * aa), (16200 * M * aa, 4050 * M * aa, 4050 * M * aa)]
    if bits == 8:
        assert want == [(470016000, 117504000, 117504000), (528768000, 132192000, 132192000)]
    got, _ = _both(w, h, bits, (25, 1), pics)
    assert [g[0] for g in got] == want
    layout = "nv12" if bits == 8 else "i420p10"
    assert _emulate_pics(w, h, layout, bits, (25, 1), [2], pics, dirty=True) == want


@pytest.mark.parametrize("kind", ["checker", "stripes"])
def test_known_answer_downsampled_highpass(kind):
    """2560 x 1440 (r = 4/9 > 2048 x 1152 / (3840 x 2160)): bval = 2, b = 4 (int)(32 * 2/3 + 0.5) = 84, the last block column 40 wide and
    the last row 12 high (all even), avg_act = sqrt(16 * 2^(2D-9) * 3/2); chroma blocks of 42 x 42.  D = 8, M = 255; distorted = M -
    reference (sse = M^2 per sample).  The `highds` filter at the cell (x, y), x and y even, weighs the 4 cell samples by 12, 8
    samples beside it by -3, 4 corners by -2 and 16 outer samples by -1.

    checker (M where x + y is odd): the cell sums to 2 M (+24 M); of each group of 4 beside it two are M (-6 M, -6 M), two corners are
    M (-4 M), and eight outer samples are M (-8 M): f = 0, so sa = 0.  Frame 1: the 2x2-cell sums of o - 0 are 2 M, ta = 2 * 2 M *
    (area / 4) = M area, ms = M, w = 1/M.  Frame 2: ta = 0, ms is clamped to 2^(8-6) = 4, w = 1/4.

    stripes (M where x % 4 < 2; cells at x % 4 == 0 are all M, at x % 4 == 2 all 0): at x % 4 == 0, +48 M, the samples above and
    below the cell -12 M, the outer ones above and below -4 M, everything at columns x - 2 .. x - 1 and x + 2 .. x + 3 is 0: f = 32 M.
    At x % 4 == 2: the columns beside the cell are M: -12 M, corners -8 M, outer 4 + 4 + 2 + 2 samples -12 M: f = -32 M.  So
    |f| = 32 M per cell, one cell per 4 samples: sa / window area = 8 M (a window starts at x = 2 and spans whole cells).  Cells
    alternate 4 M and 0, so ta / area = M as before.  Frame 1: ms = 9 M; frame 2: ms = 8 M.

    wsse = W H M^2 w avg_act, in float as the definition computes it: checker W H M avg_act and W H M^2 avg_act / 4, stripes
    W H M avg_act / 9 and W H M avg_act / 8 (Cb, Cr: the same with Wc Hc = W H / 4)."""
    w, h, bits, M = 2560, 1440, 8, 255
    aa = R.avg_act(w, h, bits)
    assert R.block_size(w, h) == 84 and R.bval_of(w, h) == 2 and aa == math.sqrt(16 * 2 ** 7 * 1.5)
    pics = [U.pictures(w, h, n, bits, kind) for n in range(2)]
    ws = [1 / M, 1 / 4] if kind == "checker" else [1 / (9 * M), 1 / (8 * M)]
    want = [tuple(int(n * M * M * wt * aa + 0.5) for n in (w * h, w * h // 4, w * h // 4)) for wt in ws]
    got, _ = _both(w, h, bits, (25, 1), pics)
    assert [g[0] for g in got] == want, ([g[0] for g in got], want)
    # the spatial activity itself: 0 for the checkerboard, 32 M per cell of the window for the stripes
    Y = pics[0][0][0]
    sa = R.sa_hp2(np.pad(Y, 2), 2, 2, w - 2, h - 2)
    assert sa == (0 if kind == "checker" else 32 * M * ((w - 4) // 2) * ((h - 4) // 2))
    if kind == "stripes":
        assert _emulate_pics(w, h, "nv12", bits, (25, 1), [1, 1], pics) == want


@pytest.mark.parametrize("second", [False, True])
def test_known_answer_temporal_activity(second):
    """Flat frames 0, K, 2K (K = 2^(D-4) = 16 at D = 8), distorted = reference + 1 (sse = 1 per sample), 480 x 270 (avg_act 128).  A flat
    picture has sa = 0.  Frame 1: o = 0, m1 = m2 = 0: ta = 0, ms is clamped to 2^(D-6) = 4, w = 1/4.  Frame 2: o - m1 = K and
    o - 2 m1 + m2 = K: ta / area = 2 K = 32, w = 1/32.  Frame 3: first order o - m1 = K again (w = 1/32); second order
    o - 2 m1 + m2 = 2K - 2K + 0 = 0 (w = 1/4).  wsse = W H w 128: 4 147 200 at w = 1/4, 518 400 at w = 1/32 (chroma: a quarter)."""
    w, h, bits = 480, 270, 8
    fps = (60, 1) if second else (25, 1)
    pics = [U.pictures(w, h, n, bits, "flat") for n in range(3)]
    assert [int(ref[0][0, 0]) for ref, _ in pics] == [0, 16, 32]
    a, b = (4147200, 1036800, 1036800), (518400, 129600, 129600)
    want = [a, b, a if second else b]
    got, _ = _both(w, h, bits, fps, pics)
    assert [g[0] for g in got] == want
    assert _emulate_pics(w, h, "i420", bits, fps, [1, 2], pics) == want


def test_known_answer_identical_pairs():
    """reference == distorted: sse = 0 in every block, wsse = 0 whatever the weights, every frame score +inf; the sequence sum
    S = sum sqrt(0) = 0 < n, so the sequence score is the mean of the frame scores: +inf"""
    w, h, bits = 176, 144, 10
    pics = [U.pictures(w, h, n, bits, "identical") for n in range(3)]
    got, seqs = _both(w, h, bits, (60, 1), pics)
    assert all(g[0] == (0, 0, 0) and all(math.isinf(v) and v > 0 for v in g[1]) for g in got)
    assert all(math.isinf(v) and v > 0 for v in seqs)
    assert tm.xpsnr.sequence(0.0, math.inf, 3, w, h, bits) == math.inf and tm.xpsnr.from_wsse(0, w, h, bits) == math.inf
    assert _emulate_pics(w, h, "i420", bits, (60, 1), [3], pics, pad=1, dirty=True) == [(0, 0, 0)] * 3


TWIN_SIZES = [(8, 8), (40, 40), (45, 45), (64, 48), (65, 49), (66, 50), (97, 61), (176, 144), (640, 480), (641, 480), (1280, 720),
              (2048, 1152), (2050, 1152), (2402, 1000)]


@pytest.mark.parametrize("w,h", TWIN_SIZES)
def test_twin_equals_the_restatement(w, h):
    """tests/xpsnr_twin.py (vectorised, written from DESIGN.md section 8) and tests/xpsnr_ref.py (the block loop) agree bit for bit on
    every content kind, first and second order, at depths 8, 10 and 16 (7680 x 4320, b = 256, is held against the twin on the GPU)"""
    big = w * h > 200000  # fewer depths and frames there: the block loop takes a second per frame
    combos = [(8, (25, 1)), (10, (60, 1)), (16, (25, 1))]
    for i, kind in enumerate(U.KINDS):
        for bits, fps in (combos if not big else [combos[1 + i % 2]]):
            _both(w, h, bits, fps, [U.pictures(w, h, n, bits, kind) for n in range(3 if not big else 2)])


@pytest.mark.parametrize("w,h,layout,bits,pad,kind,batches", [
    (96, 64, "nv12", 8, 0, "random", [2]),        # every group of 4 by the wide loads (16-byte pitches)
    (97, 61, "nv12", 8, 3, "steps", [1, 1]),      # the per-sample loads, padding on every row
    (96, 64, "p016", 12, 0, "random", [2]),       # low bits of P016 words: the wide loads must shift them out
    (98, 62, "p016", 10, 1, "stripes", [2]),      # ... and the per-sample ones
    (96, 64, "i420", 10, 0, "random", [2]),       # bits above D of I420 words: the wide loads must mask them off
    (97, 61, "i420", 12, 3, "steps", [1, 1]),     # ... and the per-sample ones
    (130, 66, "i420p10", 10, 0, "random", [2]),   # packed bits 30-31 and the absent samples of the last run
    (130, 66, "i420p10", 10, 1, "flat", [1, 1]),  # ... through the per-sample loads
    (200, 120, "i420", 16, 0, "checker", [2]),    # D = 16: shift 0, mask 0xFFFF, min_act 1024, the largest sums
    (200, 120, "p016", 16, 2, "random", [2]),
    (2402, 1000, "p016", 10, 0, "random", [1]),   # bval 2, a last block 22 wide, a last band of 16 rows
])
def test_emulated_kernels_ignore_dirty_bytes(w, h, layout, bits, pad, kind, batches):
    """every byte the layout says to ignore carries seeded garbage that differs between reference and distorted and from frame to
    frame (tests/xpsnr_util.layout_planes dirty=); the sums must be those of the sample values alone"""
    _emulated_against_restatement(w, h, layout, bits, (60, 1), batches, pad, kind=kind, dirty=True)


def test_emulated_kernels_130_slots_and_splits():
    """k_xpsnr_finish runs ceil(n / 64) workgroups: 130 slots need a third, and slots 64 .. 129 are only ever reached through
    blockIdx.x.  40 x 40 (b < 4: one block per picture, plain SSE) keeps the emulated block kernel at 130 workgroups."""
    w, h, bits = 40, 40, 8
    pics = [U.pictures(w, h, n, bits, "random") for n in range(130)]
    want, _ = _both(w, h, bits, (25, 1), pics)
    want = [g[0] for g in want]
    assert len(set(want)) > 100
    for batches in ([130], [65, 65], [128, 2]):
        assert _emulate_pics(w, h, "nv12", bits, (25, 1), batches, pics) == want, batches


def test_emulated_geometry_refusals_match_the_restatement():
    """a seeded sweep of sizes from 8 x 8 to a few hundred thousand samples, plus strips: the emulated library refuses a size
    (xe_sequence -1) exactly where the restatement's 4:2:0 grid assertion fires; some accepted sizes run 2 frames bit-exact"""
    rng = np.random.default_rng(2024)
    sizes = [(int(rng.integers(8, 700)), int(rng.integers(8, 500))) for _ in range(26)] + [(8, 600), (1000, 8), (4000, 9), (9, 3000)]
    accepted = 0
    for w, h in sizes:
        ref, dis = U.pictures(w, h, 0, 8, "random")
        try:
            R.Sequence(w, h, 8).push(ref, dis)
            ok = True
        except AssertionError:
            ok = False
        emu = U.emulate(w, h, "i420", 8, (25, 1), [], [])
        assert (emu is not None) == ok, (w, h, ok)
        if ok and accepted < 4 and w * h <= 200000:
            accepted += 1
            _emulated_against_restatement(w, h, "i420", 8, (60, 1), [1, 1], pad=w % 3, kind="random", dirty=True)
    assert accepted == 4


# ---- the binding's checks before any library call ----------------------------------------------------------------------------
class _FakeLib:
    def __init__(self):
        self.calls = []

    def tm_xpsnr_set_frame(self, *a):
        self.calls.append(a)
        return 0


def _fake(w, h, layout, bits):
    x = tm.Xpsnr.__new__(tm.Xpsnr)
    x._L, x._h, x.w, x.h, x.bits, x.batch, x.layout, x._keep = _FakeLib(), C.c_void_p(1), w, h, bits, 1, layout, {}
    return x


def test_binding_rejects_bad_planes_before_the_library():
    import torch
    w, h = 97, 61
    cw, ch = 49, 31
    good = {"nv12": [np.zeros((h, w), np.uint8), np.zeros((ch, 2 * cw), np.uint8)],
            "p016": [np.zeros((h, w), np.uint16), np.zeros((ch, 2 * cw), np.uint16)],
            "i420": [np.zeros((h, w), np.uint16), np.zeros((ch, cw), np.uint16), np.zeros((ch, cw), np.uint16)],
            "i420p10": [np.zeros((h, 128), np.uint32), np.zeros((ch, 128), np.uint32), np.zeros((ch, 128), np.uint32)]}
    bits = {"nv12": 8, "p016": 10, "i420": 12, "i420p10": 10}
    bad = []
    for layout, planes in good.items():
        bad += [(layout, planes[:-1]), (layout, planes + [planes[-1]])]                    # the plane count
        bad.append((layout, [planes[0].astype(np.int64)] + planes[1:]))                    # int64 read as bytes / words
        bad.append((layout, [planes[0].astype(np.float32 if planes[0].itemsize == 4 else np.float16)] + planes[1:]))
        bad.append((layout, [planes[0][:-1]] + planes[1:]))                                # a row short
        bad.append((layout, planes[:1] + [planes[1][:, :-1]] + planes[2:]))                # a column short
        bad.append((layout, [np.repeat(planes[0], 2, axis=1)[:, ::2]] + planes[1:]))       # column stride 2
        bad.append((layout, [torch.from_numpy(planes[0].view(np.int16 if planes[0].itemsize == 2 else planes[0].dtype))[:, :-1]]
                    + [torch.from_numpy(p.view(np.int16 if p.itemsize == 2 else p.dtype)) for p in planes[1:]]))
        t = torch.zeros((planes[0].shape[1], planes[0].shape[0]), dtype=torch.int32 if planes[0].itemsize == 4 else
                        (torch.int16 if planes[0].itemsize == 2 else torch.uint8)).t()
        bad.append((layout, [t] + [torch.from_numpy(p.view(np.int16 if p.itemsize == 2 else (np.int32 if p.itemsize == 4 else p.dtype)))
                                   for p in planes[1:]]))                                  # a transposed tensor: column stride h
    bad.append(("nv12", [np.zeros((h, w), np.int8), good["nv12"][1]]))                     # signed bytes
    bad.append(("i420", [torch.zeros((h, w), dtype=torch.int16)] + [torch.zeros((ch, cw + 1), dtype=torch.int16)[:, :cw],
                                                                    torch.zeros((ch, cw), dtype=torch.int16)]))  # Cb / Cr pitches
    for layout, planes in bad:
        x = _fake(w, h, layout, bits[layout])
        with pytest.raises(ValueError):
            x.set_frame(0, 0, planes)
        assert x._L.calls == [], layout
    # good hand-overs reach the library with the planes' own pointers and pitches
    for layout, planes in good.items():
        x = _fake(w, h, layout, bits[layout])
        padded = [np.zeros((p.shape[0], p.shape[1] + 5), p.dtype) for p in planes]  # contiguous: handed over in place
        x.set_frame(1, 0, padded)
        (a,) = x._L.calls
        assert a[1:3] == (1, 0)
        assert a[3] == padded[0].ctypes.data and a[4] == padded[1].ctypes.data and a[6] == padded[0].strides[0]
        assert a[7] == padded[1].strides[0] and a[8] == tm.ffi.TM_MEM_HOST
        assert a[5] == (padded[2].ctypes.data if len(planes) == 3 else None)
        # tensor views of padded rows: the row pitch is the padded one, the pointers the views' own
        tens = [torch.from_numpy(p.view({2: np.int16, 4: np.int32}.get(p.itemsize, p.dtype)))[:, :q.shape[1]] for p, q in zip(padded, planes)]
        x.set_frame(0, 1, tens)
        b = x._L.calls[1]
        assert b[1:3] == (0, 1) and b[3] == tens[0].data_ptr() and b[4] == tens[1].data_ptr()
        assert b[6] == padded[0].strides[0] and b[7] == padded[1].strides[0] and b[8] == tm.ffi.TM_MEM_HOST
    # host Cb / Cr planes of different pitches are copied to one
    x = _fake(w, h, "i420", 12)
    cb, cr = np.full((ch, cw + 3), 7, np.uint16)[:, :cw], np.full((ch, cw), 9, np.uint16)
    x.set_frame(0, 0, [np.zeros((h, w), np.uint16), cb, cr])
    (a,) = x._L.calls
    assert a[7] == cw * 2
    kept = x._keep[(0, 0)]
    assert kept[1].ctypes.data == a[4] and kept[2].ctypes.data == a[5] and (kept[1] == 7).all() and (kept[2] == 9).all()
