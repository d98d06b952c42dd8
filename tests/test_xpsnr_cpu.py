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


def _emulated_against_restatement(w, h, layout, bits, fps, batches, pad=0):
    n = sum(batches)
    seq = R.Sequence(w, h, bits, fps)
    frames, want = [], []
    for i in range(n):
        ref, dis = U.pictures(w, h, i, bits)
        want.append(seq.push(ref, dis)[0])
        frames.append((U.layout_planes(layout, ref, w, h, bits, pad), U.layout_planes(layout, dis, w, h, bits, pad)))
    got = U.emulate(w, h, layout, bits, fps, batches, frames)
    assert got == want, (w, h, layout, bits, fps, batches, got, want)
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
