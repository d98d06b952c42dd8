"""No-GPU tier of VMAF integer motion (include/turbo_metrics_motion.h, libturbometrics_motion.so): the hand-derived answers of DESIGN.md
section 9 as literals against the numpy restatement (tests/motion_ref.py) and against the kernel SOURCE executed lane by lane on the
CPU (tests/motion_emul); emulated kernel == restatement, sad exact, on all four layouts, dirty bytes, tiny and odd sizes, batch splits
and reset; create-time refusals; the ABI (C99 header, exports); the host functions; the binding's checks; the CLI's option parsing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import motion_ref as R
from tests import motion_util as U
from tm_pkg import tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MLIB = os.path.join(ROOT, "turbo-metrics_amd", "libturbometrics_motion.so")
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")


def declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(2) for m in re.finditer(r" ([A-Za-z]) (\S+)", out) if m.group(1) in "TDBRW" and not m.group(2).startswith(("_init", "_fini", "__bss", "_edata", "_end")))


def layout_for(bits, kind="msb"):
    return "y8" if bits == 8 else ("y16_msb" if kind == "msb" else "y16_low")


def emul_seq(w, h, layout, bits, seq, batches, pad=0, dirty=False, want_blur=False):
    planes = [U.luma_plane(layout, Y, bits, pad=pad, dirty=(i if dirty else None)) for i, Y in enumerate(seq)]
    return U.emulate(w, h, layout, bits, batches, planes, want_blur=want_blur)


# ---- the hand-derived answers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10, 16])
def test_known_answer_flat_pictures(bits):
    w, h = 37, 23
    a, b = np.full((h, w), 5 << (bits - 8), np.int64), np.full((h, w), 9 << (bits - 8), np.int64)
    assert (R.blur(a, bits) == 5 * 256).all() and (R.blur(b, bits) == 9 * 256).all()
    assert R.sequence([a, b], bits) == [(0, 0.0), (871424, 4.0)]
    for lay in {layout_for(bits), layout_for(bits, "low")}:
        sads, blurred = emul_seq(w, h, lay, bits, [a, b], [2], want_blur=True)
        assert sads == [0, 871424] and (blurred == 9 * 256).all()


def test_known_answer_single_sample():
    p = np.zeros((40, 41), np.int64)
    p[20, 19] = 255
    patch = np.array([[194, 869, 1432, 869, 194], [869, 3893, 6418, 3893, 869], [1432, 6418, 10582, 6418, 1432],
                      [869, 3893, 6418, 3893, 869], [194, 869, 1432, 869, 194]])
    want = np.zeros_like(p)
    want[18:23, 17:22] = patch
    assert patch.sum() == 65282
    assert (R.blur(p, 8) == want).all()
    sads, blurred = emul_seq(41, 40, "y8", 8, [np.zeros_like(p), p], [1, 1], want_blur=True)
    assert (blurred == want).all() and sads == [0, 65282]


def test_known_answer_alternating_columns_and_the_asymmetric_mirror():
    w, h = 64, 48
    s = np.where(np.indices((h, w))[1] % 2 == 1, 255, 0).astype(np.int64)
    b = R.blur(s, 8)
    assert (b[:, 2:-2:2] == 31883).all() and (b[:, 3:-2:2] == 33397).all()
    assert (b[:, :2] == [31883, 33397]).all() and (b[:, -2:] == [35440, 45781]).all()
    assert (b[:, 0] != b[:, -1]).all()  # left edge reflects without repeating the edge sample, right edge repeats it
    assert not (b[:, :-2] == 35440).any() and not (b[:, :-2] == 45781).any()
    assert R.sequence([s, 255 - s], 8) == [(0, 0.0), (6036000, 7.6751708984375)]
    sads, blurred = emul_seq(w, h, "y8", 8, [s, 255 - s, s], [3], want_blur=True)
    assert sads == [0, 6036000, 6036000] and (blurred == b).all()


def test_known_answer_full_scale_16_bit_does_not_overflow():
    p = np.full((9, 11), 65535, np.int64)
    assert (R.blur(p, 16) == 65535).all()
    for lay in ("y16_msb", "y16_low"):
        sads, blurred = emul_seq(11, 9, lay, 16, [0 * p, p], [2], want_blur=True)
        assert (blurred == 65535).all() and sads == [0, 65535 * 99]


# ---- emulated kernel == restatement ----------------------------------------------------------------------------------------
SIZES = [(3, 3), (3, 64), (64, 3), (5, 7), (121, 17), (130, 37), (250, 20), (243, 35)]  # widths not multiples of 4; not multiples of the 120 x 16 tile


@pytest.mark.parametrize("layout,bits", U.CASES)
@pytest.mark.parametrize("w,h", SIZES)
def test_emulated_kernel_matches_the_restatement_with_dirty_bytes(layout, bits, w, h):
    kind = ("random", "extreme", "smooth")[(w + h + bits) % 3]
    seq = U.sequence(w, h, 4, bits, kind)
    want = [f[0] for f in R.sequence(seq, bits)]
    for pad, dirty in ((0, False), (5, True)):
        sads, blurred = emul_seq(w, h, layout, bits, seq, [1, 3], pad=pad, dirty=dirty, want_blur=True)
        assert sads == want, (layout, bits, w, h, pad)
        assert (blurred == R.blur(seq[-1], bits)).all()


@pytest.mark.parametrize("layout,bits", [("y8", 8), ("y10_packed", 10), ("y16_low", 12)])
def test_batch_splits_and_reset_do_not_change_a_bit(layout, bits):
    w, h = 133, 21
    seq = U.sequence(w, h, 7, bits)
    want = [f[0] for f in R.sequence(seq, bits)]
    assert emul_seq(w, h, layout, bits, seq, [7], dirty=True) == want
    assert emul_seq(w, h, layout, bits, seq, [3, 1, 3], dirty=True) == want
    assert emul_seq(w, h, layout, bits, seq, [1] * 7, dirty=True) == want
    # a reset starts a new sequence: pictures 4 .. 6 as a sequence of their own
    again = [f[0] for f in R.sequence(seq[4:], bits)]
    assert again[0] == 0 and emul_seq(w, h, layout, bits, seq, [2, 2, -2, 1]) == want[:4] + again


def test_more_slots_than_one_batch():
    w, h, bits = 20, 9, 8
    seq = U.sequence(w, h, 23, bits)
    want = [f[0] for f in R.sequence(seq, bits)]
    assert emul_seq(w, h, "y8", bits, seq, [8, 8, 7]) == want
    assert emul_seq(w, h, "y8", bits, seq, [23]) == want


def test_refusals_match_the_restatement():
    seq = {}
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 12, 16, 17):
            for w, h in ((2, 8), (8, 2), (3, 3), (8, 8)):
                ok = R.supported(w, h, layout, bits)
                if ok and (w, h, bits) not in seq:
                    seq[(w, h, bits)] = U.sequence(w, h, 1, bits)
                if ok:
                    got = emul_seq(w, h, layout, bits, seq[(w, h, bits)], [1])
                else:  # the geometry is refused before a plane is looked at
                    got = U.emulate(w, h, layout, bits, [1], [np.zeros((8, 64), np.uint32)])
                assert (got is not None) == ok, (layout, bits, w, h)


def test_create_refuses_before_touching_the_device():
    L = tm.motion.lib()
    h = C.c_void_p()
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 16, 17):
            for w, hh in ((2, 8), (8, 2), (0, 0)):
                assert L.tm_motion_create(C.byref(h), w, hh, U.LAYOUT[layout], bits, 1) == tm.ffi.TM_ERR_UNSUPPORTED
            if not R.supported(8, 8, layout, bits):
                assert L.tm_motion_create(C.byref(h), 8, 8, U.LAYOUT[layout], bits, 1) == tm.ffi.TM_ERR_UNSUPPORTED
    assert L.tm_motion_create(C.byref(h), 8, 8, 7, 8, 1) == tm.ffi.TM_ERR_UNSUPPORTED
    assert L.tm_motion_create(None, 8, 8, 0, 8, 1) == tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_motion_create(C.byref(h), 8, 8, 0, 8, 0) == tm.ffi.TM_ERR_INVALID_ARG
    assert h.value is None


# ---- ABI, host functions, binding, CLI ---------------------------------------------------------------------------------------
def test_header_is_plain_c99_and_the_library_exports_exactly_it(tmp_path):
    want = declared("turbo_metrics_motion.h")
    assert len(want) == 10 and all(n.startswith("tm_motion") for n in want)
    assert exported(MLIB) == want
    assert sorted(tm.motion.SYMBOLS) == want
    src = tmp_path / "c.c"
    src.write_text('#include "turbo_metrics_motion.h"\n#include <stdio.h>\n'
                   "int main(void) { tm_motion *m = NULL; tm_motion_frame f; f.sad = 0; (void)m;\n"
                   "  printf(\"%.13f %.1f\\n\", tm_motion_from_sad(123456789123u, 1920, 1080), tm_motion2(3.0, 2.0)); return (int)f.sad; }\n")
    exe = str(tmp_path / "c")
    lib_dir = os.path.dirname(MLIB)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                           "-L" + lib_dir, "-lturbometrics_motion", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "232.5680389404297 2.0", (out.returncode, out.stdout, out.stderr)


def test_the_other_libraries_are_unchanged_in_what_they_export():
    for lib in (tm.ffi.SHIP_LIB_PATH, tm.ffi.LIB_PATH, tm.xpsnr.LIB_PATH):
        assert not [n for n in exported(lib) if "motion" in n], lib
    assert not [n for n in tm.ffi.SYMBOLS if "motion" in n]
    assert exported(tm.xpsnr.LIB_PATH) == declared("turbo_metrics_xpsnr.h")


def test_host_functions_match_the_restatement():
    assert tm.motion.from_sad(123456789123, 1920, 1080) == 232.5680389404297 == R.from_sad(123456789123, 1920, 1080)
    assert tm.motion.from_sad(123456789123, 1920, 1080) != 123456789123 / 256.0 / (1920 * 1080)  # the float casts change digits
    rng = np.random.default_rng(9)
    for _ in range(200):
        sad, w, h = int(rng.integers(0, 1 << 44)), int(rng.integers(3, 8000)), int(rng.integers(3, 5000))
        assert tm.motion.from_sad(sad, w, h) == R.from_sad(sad, w, h)
    assert tm.motion.from_sad(871424, 37, 23) == 4.0 and tm.motion.from_sad(0, 3, 3) == 0.0
    m = [0.0, 3.5, 1.25, 1.25, 9.0, 2.0]
    assert tm.motion.motion2(m) == R.motion2(m) == [0.0, 1.25, 1.25, 1.25, 2.0, 2.0]
    assert tm.motion.motion2([]) == [] and tm.motion.motion2([0.0]) == [0.0]


class _FakeLib:
    """stands in for the library under a Motion object: any call after the plane checks is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_binding_rejects_bad_planes_before_the_library():
    def obj(w, h, layout, bits):
        m = tm.Motion.__new__(tm.Motion)
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


def test_cli_names_motion_and_refuses_what_it_cannot_do_before_touching_the_device(tmp_path):
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    for p in (a, b):
        with open(p, "wb") as f:
            f.write(b"YUV4MPEG2 W16 H16 F25:1 C420jpeg\nFRAME\n" + bytes(16 * 16 + 2 * 64))
    for extra in (["--every", "2"], ["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
        for sel in ([], ["-m", "psnr"]):
            out = subprocess.run([CLI, a, b, "--motion", *sel, *extra], capture_output=True, text=True, timeout=60)
            assert out.returncode != 0 and "--motion does not run with" in out.stderr, (extra, out.returncode, out.stderr)
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "--motion" in out.stdout and "ssimulacra2, xpsnr]" in out.stdout
    out = subprocess.run([CLI, a, "--motion"], capture_output=True, text=True, timeout=60)  # the distorted argument is still required
    assert out.returncode == 2 and "<DISTORTED>" in out.stderr
    out = subprocess.run([CLI, a, b, "-m", "motion"], capture_output=True, text=True, timeout=60)  # a flag, not a value of -m
    assert out.returncode == 2 and "possible values: psnr, ssim, msssim, ssimulacra2" in out.stderr
