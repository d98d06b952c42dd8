"""No-GPU tier of P.910 SI / TI (include/turbo_metrics_siti.h, libturbometrics_siti.so): the hand-derived answers of DESIGN.md section 19
as literals against the integer restatement (tests/siti_ref.py) and against the kernel SOURCE executed lane by lane on the CPU
(tests/siti_emul); emulated kernel == restatement, every sum exact, on all four layouts, edge sizes, dirty bits, garbage padding,
unaligned bases, batch splits and reset; the integer SI against an independent float64 statement within a derived bound; seeded
mistakes in the restatement, each caught; create-time refusals; the ABI (C99 header, exports); the host functions; the binding's
checks; the CLI's option parsing; the parent's CLI output without --siti, byte for byte."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import siti_ref as R
from tests import siti_util as U
from tm_pkg import tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLIB = os.path.join(ROOT, "turbo-metrics_amd", "libturbometrics_siti.so")
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")


def declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(2) for m in re.finditer(r" ([A-Za-z]) (\S+)", out) if m.group(1) in "TDBRW" and not m.group(2).startswith(("_init", "_fini", "__bss", "_edata", "_end")))


def emul_seq(w, h, layout, bits, seq, batches, pad=0, dirty=False, misalign=False, want_last=False):
    planes = [U.luma_plane(layout, Y, bits, pad=pad, dirty=(i if dirty else None)) for i, Y in enumerate(seq)]
    if misalign:
        planes = [U.misaligned(p) for p in planes]
    return U.emulate(w, h, layout, bits, batches, planes, want_last=want_last)


def both(seq, bits, layout=None, batches=None):
    """the restatement's sums, after checking that the emulated kernel gives the same"""
    h, w = seq[0].shape
    want = R.sums(seq, bits)
    lay = layout or ("y8" if bits == 8 else "y16_low")
    assert emul_seq(w, h, lay, bits, seq, batches or [len(seq)]) == want
    return want


# ---- the hand-derived answers ----------------------------------------------------------------------------------------------
def test_the_tile_constants_the_tests_build_their_sizes_from():
    t = (C.c_int * 2)()
    U.emul_lib().se_tile(t)
    assert (t[0], t[1]) == (U.TW, U.TH)


@pytest.mark.parametrize("bits", [8, 10, 16])
def test_known_answer_flat_pictures(bits):
    w, h = 37, 23
    a, b = np.full((h, w), 5 << (bits - 8), np.int64), np.full((h, w), 9 << (bits - 8), np.int64)
    d = 4 << (bits - 8)
    assert both([a, b], bits) == [(0, 0, 0, 0, 0), (0, 0, w * h * d, w * h * d * d, 1)]
    fr = R.sequence([a, b], bits)
    assert fr[1]["ti"] == 0.0 == tm.siti.ti(w * h * d, w * h * d * d, w * h, bits) and fr[0]["si"] == 0.0  # T1 = n d, ti exactly 0


def test_known_answer_horizontal_ramp_has_constant_q():
    y, x = np.indices((33, 47))
    (s1, s2, *_), = both([3 * x], 8)  # gx = 8 c = 24, gy = 0: q = 24 * 256
    assert (s1, s2) == (6144 * 45 * 31, 6144 * 6144 * 45 * 31) == (8570880, 52659486720)
    assert R.si(s1, s2, 45 * 31) == 0.0 == tm.siti.si(s1, s2, 45 * 31)


def test_known_answer_diagonal_ramp_is_exactly_zero_where_float_magnitudes_are_not():
    y, x = np.indices((33, 47))
    (s1, s2, *_), = both([x + y], 8)  # gx = gy = 8, m2 = 128, M = 128 << 16: sqrt = 2896.3..., q = 2896 everywhere
    assert (s1, s2) == (2896 * 45 * 31, 2896 * 2896 * 45 * 31)
    assert R.si(s1, s2, 45 * 31) == 0.0 == tm.siti.si(s1, s2, 45 * 31)
    assert R.si_f64(x + y, 8) > 0.0  # sqrt(128) summed in floating point: a "variance" from rounding alone


def test_known_answer_single_sample():
    p = np.zeros((40, 41), np.int64)
    p[20, 19] = 255
    # the four edge neighbours: m2 = 4 v^2, q = 2 v 256 = 130560; the four diagonal ones: m2 = 2 v^2, q = round(255 * 256 * sqrt 2) = 92320
    assert (R.quantise(4 * 255 * 255 << 16), R.quantise(2 * 255 * 255 << 16)) == (130560, 92320)
    s1, s2 = 4 * 130560 + 4 * 92320, 4 * 130560 ** 2 + 4 * 92320 ** 2
    assert (s1, s2) == (891520, 102275584000)
    assert both([0 * p, p], 8, batches=[1, 1]) == [(0, 0, 0, 0, 0), (s1, s2, 255, 65025, 1)]


def test_known_answer_vertical_step_edge():
    s = np.zeros((20, 30), np.int64)
    s[:, 15:] = 200  # columns 14 and 15 see gx = 4 * 200, q = 800 * 256, on the 18 interior rows
    (s1, s2, *_), = both([s], 8)
    assert (s1, s2) == (36 * 204800, 36 * 204800 ** 2) == (7372800, 1509949440000)
    n = 28 * 18
    assert R.si(s1, s2, n) == pytest.approx(800 * np.sqrt(36 / n - (36 / n) ** 2), rel=1e-15)


def test_known_answer_half_the_picture_changed():
    w, h, d = 40, 24, -6
    a = np.full((h, w), 100, np.int64)
    b = a.copy()
    b[:, :w // 2] += d
    fr = R.sequence([a, b], 8)
    assert (fr[1]["t1"], fr[1]["t2"]) == (w * h // 2 * d, w * h // 2 * d * d) and fr[1]["ti"] == abs(d) / 2 == 3.0
    assert both([a, b], 8)[1][2:] == (-2880, 17280, 1)
    # the same content at 10 bits (code values 4 x): the same ti on the 8-bit scale
    assert R.sequence([4 * a, 4 * b], 10)[1]["ti"] == 3.0 and both([4 * a, 4 * b], 10, "y10_packed")[1][2:] == (-11520, 276480, 1)


def test_known_answer_16_bit_extremes_stay_inside_the_bounds():
    y, x = np.indices((33, 47))
    M = 65535
    c = ((x + y) % 2) * M  # the largest |d| at every position: T2 = M^2 n; Sobel of a checkerboard is 0
    for lay in ("y16_msb", "y16_low"):
        assert both([c, M - c], 16, lay) == [(0, 0, 0, 0, 0), (0, 0, M * (776 - 775), M * M * 47 * 33, 1)]
    k = np.array([[0, 0, M], [0, 7, M], [0, M, M]])  # the largest m2: gx = 4 M, gy = 2 M, m2 = 20 M^2 < 2^37
    gx, gy = R.sobel(k)
    assert (int(gx[0, 0]), int(gy[0, 0])) == (4 * M, 2 * M) and 20 * M * M < 1 << 37
    q = R.quantise(20 * M * M)
    assert q == 293081 and q * q - q < 20 * M * M <= q * q + q
    assert both([k], 16) == [(q, q * q, 0, 0, 0)]
    corner = np.where((x > 20) | (y > 16), M, 0)  # that neighbourhood inside a picture of more than one tile row
    assert both([corner, M - corner], 16, "y16_msb")[1][3] == M * M * 47 * 33
    # the bounds the header states: S2 < 2^37 n_si < 2^63 and n T2, T1^2 < 2^90 at the largest picture create accepts
    assert (1 << 37) * R.MAX_SAMPLES <= 1 << 63 and R.MAX_SAMPLES * (M * M * R.MAX_SAMPLES) < 1 << 90
    big = tm.siti.ti(-M * R.MAX_SAMPLES // 2, M * M * R.MAX_SAMPLES // 2, R.MAX_SAMPLES, 16)  # half the largest picture changed by -M
    assert big == M / 2 / 256


def test_the_kernels_magnitude_is_the_q_of_the_inequality():
    L = U.emul_lib()
    rng = np.random.default_rng(19)
    Ms = [0, 1, 2, 3, 6, 7, (1 << 37) - 1, 20 * 65535 ** 2, 128 << 16]
    for q in (1, 2, 255, 2896, 65535, 92320, 293081, 370727):
        Ms += [q * q - q, q * q - q + 1, q * q, q * q + q, q * q + q + 1]
    Ms += [int(v) for v in rng.integers(0, 1 << 37, 20000)] + [int(v) << 16 for v in rng.integers(0, 1 << 21, 20000)]
    for M in Ms:
        assert L.se_magnitude(M) == R.quantise(M), M


# ---- emulated kernel == restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,bits", U.CASES)
def test_emulated_kernel_matches_the_restatement_on_the_edge_sizes(layout, bits):
    sizes = U.edge_sizes() + ([(w, 4) for w in U.P10_WIDTHS] if layout == "y10_packed" else [])
    for w, h in sizes:
        seq = U.sequence(w, h, 3, bits, ("random", "extreme", "smooth")[(w + h) % 3])
        want = R.sums(seq, bits)
        # garbage in the pitch padding and in every bit the layout ignores; then an unaligned base: the scalar load path
        got, last = emul_seq(w, h, layout, bits, seq, [1, 2], pad=5, dirty=True, want_last=True)
        assert got == want and (last == seq[-1]).all(), (w, h)
        assert emul_seq(w, h, layout, bits, seq, [3], dirty=True, misalign=True) == want, (w, h, "unaligned")


@pytest.mark.parametrize("layout,bits", U.ONE_PER_LAYOUT)
def test_batch_splits_and_reset_do_not_change_a_bit(layout, bits):
    w, h = 133, 41
    seq = U.sequence(w, h, 4, bits)
    want = R.sums(seq, bits)
    for split in ([1, 1, 1, 1], [4], [3, 1]):
        assert emul_seq(w, h, layout, bits, seq, split, dirty=True) == want, split
    # a reset starts a new sequence: pictures 2 .. 3 as a sequence of their own
    again = R.sums(seq[2:], bits)
    assert again[0][2:] == (0, 0, 0) and emul_seq(w, h, layout, bits, seq, [2, -1, 1]) == want[:2] + again


def test_refusals_match_the_restatement():
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 12, 16, 17):
            for w, h in ((2, 8), (8, 2), (3, 3), (8, 8), (8192, 8193)):
                ok = R.supported(w, h, layout, bits)
                if w * h > 64:  # the geometry is refused before a plane is looked at; the largest accepted one is not run here
                    assert not ok
                    got = U.emulate(w, h, layout, bits, [1], [np.zeros((8, 64), np.uint32)])
                elif ok:
                    got = emul_seq(w, h, layout, bits, U.sequence(w, h, 1, bits), [1])
                else:
                    got = U.emulate(w, h, layout, bits, [1], [np.zeros((8, 64), np.uint32)])
                assert (got is not None) == ok, (layout, bits, w, h)
    assert R.supported(8192, 8192, "y8", 8) and not R.supported(8192, 8193, "y8", 8)


def test_create_refuses_before_touching_the_device():
    L = tm.siti.lib()
    h = C.c_void_p()
    for layout in U.LAYOUT:
        for bits in (7, 8, 9, 10, 16, 17):
            for w, hh in ((2, 8), (8, 2), (0, 0), (8192, 8193), (1 << 26, 3)):
                assert L.tm_siti_create(C.byref(h), w, hh, U.LAYOUT[layout], bits, 1) == tm.ffi.TM_ERR_UNSUPPORTED
            if not R.supported(8, 8, layout, bits):
                assert L.tm_siti_create(C.byref(h), 8, 8, U.LAYOUT[layout], bits, 1) == tm.ffi.TM_ERR_UNSUPPORTED
    assert L.tm_siti_create(C.byref(h), 8, 8, 7, 8, 1) == tm.ffi.TM_ERR_UNSUPPORTED
    assert L.tm_siti_create(None, 8, 8, 0, 8, 1) == tm.ffi.TM_ERR_INVALID_ARG
    assert L.tm_siti_create(C.byref(h), 8, 8, 0, 8, 0) == tm.ffi.TM_ERR_INVALID_ARG
    assert h.value is None


# ---- the integer statement against the float64 one ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10, 12, 16])
@pytest.mark.parametrize("kind", ["random", "smooth", "extreme"])
def test_integer_si_against_the_float64_statement(bits, kind):
    # q 2^-(16 - D) differs from the true magnitude by at most half a unit, i.e. 2^-9 on the 8-bit scale, and a standard deviation
    # moves by at most the RMS of a perturbation; TI has no quantisation at all
    seq = U.sequence(97, 61, 3, bits, kind)
    fr = R.sequence(seq, bits)
    for i, f in enumerate(fr):
        assert abs(f["si"] - R.si_f64(seq[i], bits)) <= 2.0 ** -9 + 1e-9
        if i:
            want = R.ti_f64(seq[i], seq[i - 1], bits)
            assert abs(f["ti"] - want) <= 1e-9 * want


# ---- seeded mistakes: each wrong reading of the text is caught by a hand value or by the float statement -----------------------
def _hand_values(mistake):
    """the literal checks above, against the restatement with one mistake seeded; -> the names of those that fail"""
    failed = []
    y, x = np.indices((33, 47))
    p = np.zeros((40, 41), np.int64)
    p[20, 19] = 255
    s = np.zeros((20, 30), np.int64)
    s[:, 15:] = 200
    a = np.full((24, 40), 100, np.int64)
    b = a.copy()
    b[:, :20] -= 6
    fr = R.sequence([0 * p, p], 8, mistake)
    if (fr[1]["s1"], fr[1]["s2"]) != (891520, 102275584000):
        failed.append("single sample")
    f = R.sequence([3 * x], 8, mistake)[0]
    if (f["s1"], f["s2"], f["si"]) != (8570880, 52659486720, 0.0):
        failed.append("horizontal ramp")
    f = R.sequence([s], 8, mistake)[0]
    if (f["s1"], f["s2"]) != (7372800, 1509949440000) or abs(f["si"] - 800 * np.sqrt(36 / 504 - (36 / 504) ** 2)) > 1e-12:
        failed.append("step edge")
    f = R.sequence([a, b], 8, mistake)[1]
    if (f["t1"], f["t2"], f["ti"]) != (-2880, 17280, 3.0):
        failed.append("half changed")
    seq = U.sequence(97, 61, 2, 8, "random")
    f = R.sequence(seq, 8, mistake)
    if abs(f[1]["si"] - R.si_f64(seq[1], 8)) > 2.0 ** -9 + 1e-9 or abs(f[1]["ti"] - R.ti_f64(seq[1], seq[0], 8)) > 1e-9 * f[1]["ti"]:
        failed.append("float64 statement")
    return failed


def test_the_checks_pass_without_a_mistake():
    assert _hand_values(None) == []


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_seeded_mistakes_are_caught(mistake):
    assert len(R.MISTAKES) >= 5 and _hand_values(mistake), mistake


# ---- ABI, host functions, binding, CLI ---------------------------------------------------------------------------------------
def test_header_is_plain_c99_and_the_library_exports_exactly_it(tmp_path):
    want = declared("turbo_metrics_siti.h")
    assert len(want) == 10 and all(n.startswith("tm_siti") for n in want)
    assert exported(SLIB) == want
    assert sorted(tm.siti.SYMBOLS) == want
    src = tmp_path / "c.c"
    src.write_text('#include "turbo_metrics_siti.h"\n#include <stdio.h>\n'
                   "int main(void) { tm_siti *m = NULL; tm_siti_frame f; f.s1 = 0; f.ti_valid = 0; (void)m;\n"
                   "  printf(\"%.17g %.17g\\n\", tm_siti_si(7372800u, 1509949440000u, 504, 1.0), tm_siti_ti(-2880, 17280, 960, 8, 2.0));\n"
                   "  return (int)f.s1 + f.ti_valid + (sizeof f != 56); }\n")
    exe = str(tmp_path / "c")
    lib_dir = os.path.dirname(SLIB)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                           "-L" + lib_dir, "-lturbometrics_siti", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and [float(v) for v in out.stdout.split()] == [R.si(7372800, 1509949440000, 504), 6.0], (out.returncode, out.stdout, out.stderr)
    assert C.sizeof(tm.siti.SitiFrameC) == 56


def test_the_other_libraries_are_unchanged_in_what_they_export():
    for lib in (tm.ffi.SHIP_LIB_PATH, tm.ffi.LIB_PATH, tm.motion.LIB_PATH, tm.scene.LIB_PATH):
        assert not [n for n in exported(lib) if "siti" in n], lib
    assert not [n for n in tm.ffi.SYMBOLS if "siti" in n]
    assert exported(tm.motion.LIB_PATH) == declared("turbo_metrics_motion.h")


def test_host_functions_match_the_restatement():
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(1, R.MAX_SAMPLES))
        q = rng.integers(0, 1 << 18, 2).astype(object)  # sums of a picture of two magnitudes / two differences: a valid radicand
        k = int(rng.integers(0, n + 1))
        s1, s2 = k * q[0] + (n - k) * q[1], k * q[0] ** 2 + (n - k) * q[1] ** 2
        gain = float(rng.choice([1.0, 255 / 219, 0.5]))
        assert tm.siti.si(s1, s2, n, gain) == R.si(s1, s2, n, gain)
        d = [int(v) - 65535 for v in rng.integers(0, 131071, 2)]
        t1, t2 = k * d[0] + (n - k) * d[1], k * d[0] ** 2 + (n - k) * d[1] ** 2
        bits = int(rng.integers(8, 17))
        assert tm.siti.ti(t1, t2, n, bits, gain) == R.ti(t1, t2, n, bits, gain)
    assert tm.siti.si(0, 0, 1) == 0.0 and tm.siti.si(5, 25, 1) == 0.0 and tm.siti.si(0, 0, 0) == 0.0
    assert tm.siti.si(0, 1 << 32, 1) == 256.0 and tm.siti.ti(0, 16, 1, 10) == 1.0 and tm.siti.ti(-3, 9, 1, 8) == 0.0
    assert tm.siti.LIMITED_RANGE_GAIN == 255 / 219
    # a radicand beyond 2^64: formed exactly, where n s2 in 64 bits would wrap
    n, s1, s2 = 1 << 26, (1 << 26) * 1000 + 1, (1 << 26) * 1000000 + 2000 + (1 << 40)
    assert tm.siti.si(s1, s2, n) == R.si(s1, s2, n) > 0


class _FakeLib:
    """stands in for the library under a Siti object: any call after the plane checks is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_binding_rejects_bad_planes_before_the_library():
    def obj(w, h, layout, bits):
        m = tm.Siti.__new__(tm.Siti)
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
    with pytest.raises(KeyError):
        tm.Siti(16, 8, "nv12", 8)


def test_cli_names_siti_and_refuses_what_it_cannot_do_before_touching_the_device(tmp_path):
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    for p in (a, b):
        with open(p, "wb") as f:
            f.write(b"YUV4MPEG2 W16 H16 F25:1 C420jpeg\nFRAME\n" + bytes(16 * 16 + 2 * 64))

    def run(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)
    for extra in (["--every", "2"], ["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
        for sel in ([], ["-m", "psnr"], ["--motion"]):
            out = run(a, b, "--siti", *sel, *extra)
            assert out.returncode != 0 and ("--siti does not run with" in out.stderr or "--motion does not run with" in out.stderr), (extra, out.stderr)
        out = run(a, b, "--siti", *extra)
        assert out.returncode != 0 and "--siti does not run with" in out.stderr, (extra, out.returncode, out.stderr)
    out = run("--help")
    assert "--siti " in out.stdout and "--siti-gain <X>" in out.stdout and "--siti-range <RANGE>" in out.stdout
    out = run(a, "--siti")  # the distorted argument is still required
    assert out.returncode == 2 and "<DISTORTED>" in out.stderr
    out = run(a, b, "-m", "siti")  # a flag, not a value of -m
    assert out.returncode == 2 and "possible values: psnr, ssim, msssim, ssimulacra2" in out.stderr
    for bad, msg in ((["--siti-gain", "2"], "belong to '--siti'"), (["--siti-range", "limited"], "belong to '--siti'"),
                     (["--siti", "--siti-gain"], "a value is required"), (["--siti", "--siti-gain", "0"], "invalid value '0'"),
                     (["--siti", "--siti-gain", "-1"], "invalid value '-1'"), (["--siti", "--siti-gain", "x"], "invalid value 'x'"),
                     (["--siti", "--siti-gain", "nan"], "invalid value 'nan'"), (["--siti", "--siti-range", "pq"], "possible values: full, limited"),
                     (["--siti", "--siti-range"], "a value is required"),
                     (["--siti", "--siti-gain", "2", "--siti-range", "limited"], "cannot be used together")):
        out = run(a, b, *bad)
        assert out.returncode == 2 and msg in out.stderr, (bad, out.returncode, out.stderr)


def test_the_record_of_the_parents_cli_output_is_well_formed():
    """tests/golden/siti_parent_cli.json: the parent commit's binary without --siti, recorded on the MI355X.  Running the binary again
    needs the GPU, so the byte-for-byte comparison is tests/test_gpu_siti_golden.py; here: the record matches its list of invocations."""
    from tests import test_gpu_siti_golden as G
    g = json.load(open(G.GOLDEN))
    assert sorted(g) == sorted(G.PARENT_CASES) and all(isinstance(v, str) and v for v in g.values())
    args = [a for _, a in G.PARENT_CASES.values()]
    assert not any("siti" in x for a in args for x in a)
    for fmt in ("csv", "json", "json-lines"):
        assert any(a[-2:] == ["--output", fmt] and "--motion" in a for a in args) and any(a[-2:] == ["--output", fmt] and "--motion" not in a for a in args)
