"""CPU tier of LDR-FLIP: the host side of the definition, the hand values, and the SOURCE of the kernels run lane
by lane on the CPU (tests/flip_emul) against the float64 numpy restatement (tests/flip_ref.py), inside the tolerance measured here and
recorded in tests/flip_util.py; ten seeded mistakes in the restatement are each far outside it.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import flip_ref as R
from tests import flip_util as U
from tm_pkg import tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbo-metrics_amd", "libturbometrics_flip.so")
T_W, T_H, HALO = U.tile()
SHAPES = ((1, 1), (7, 5), (21, 21), (T_W - 1, T_H + 1), (T_W, T_H), (T_W + 1, T_H - 1), (33, 17), (130, 70))
HAND = (((0, 0, 0), (255, 255, 255), 0.96737976), ((127, 127, 127), (128, 128, 128), 0.02988465), ((255, 0, 0), (0, 255, 0), 0.98666228))


def uniform(c, w=24, h=18):
    return np.ascontiguousarray(np.broadcast_to(np.array(c, np.uint8), (h, w, 3)))


# ---- the interface and the host side -------------------------------------------------------------------------------------------
def test_flip_map_is_the_header_and_the_library_exports_it():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "turbo_metrics_flip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tm_flip_[a-z0-9_]+)\s*\(", src)))
    assert len(declared) == 9 and "tm_flip_get_map" in declared and "tm_flip_radius" in declared
    mp = open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "flip.map")).read()
    assert sorted(re.findall(r"^\s+(tm_[a-z0-9_]+);", mp, flags=re.M)) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert sorted(n for n in re.findall(r" [TDBRW] (\S+)", out) if not n.startswith(("_init", "_fini", "__bss", "_edata", "_end"))) == declared
    assert sorted(tm.flip.SYMBOLS) == declared
    # no other library gained a symbol
    for name in ("hip", "xpsnr", "motion", "vif", "adm", "scene", "cambi"):
        o = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "turbo-metrics_amd", f"libturbometrics_{name}.so")], capture_output=True, text=True, check=True).stdout
        assert "tm_flip" not in o, name


def test_radius_and_constants():
    assert tm.flip.radius() == (10, 9) == R.radius() == U.emul_radius(U.DEFAULT_PPD)
    assert abs(U.DEFAULT_PPD - 67.02064327658226) < 1e-12 and tm.flip.DEFAULT_PPD == 67.02064327658226
    for ppd in (8, 30, 67, 74, 74.1, 100, 256):
        assert tm.flip.radius(ppd) == R.radius(ppd) == U.emul_radius(ppd)
    assert tm.flip.radius(100) == (14, 13)
    g = U.geom(64, 64)
    assert abs(g.cmax - 41.27609841) < 1e-8 and abs(R.cmax() - g.cmax) < 1e-12
    # every 2-D filter sums to 1: Y, Cx, and the two Cz terms together; G sums to 1, G' and G'' to +1 and -1 by sign
    ws, wf = g.ws.astype(np.float64), g.wf.astype(np.float64)
    assert abs(ws[0].sum() ** 2 - 1) < 1e-6 and abs(ws[1].sum() ** 2 - 1) < 1e-6 and abs(ws[2].sum() ** 2 + ws[3].sum() ** 2 - 1) < 1e-6
    assert abs(wf[0].sum() - 1) < 1e-6
    for f in wf[1:]:
        assert abs(f[f > 0].sum() - 1) < 1e-6 and abs(f[f < 0].sum() + 1) < 1e-6
    assert (wf[:, 0] == 0).all() and (wf[0, 1] > 0)  # radius 9 inside the halo of 10
    assert (wf[1] == -wf[1][::-1]).all() and (wf[2] == wf[2][::-1]).all()


def test_what_create_refuses():
    """the bound of the header: a spatial radius above the halo, i.e. every ppd above 10 / (3 sqrt(0.04 / (2 pi^2))) = 74.048"""
    assert HALO == tm.flip.MAX_RADIUS == 10
    assert U.geom(64, 64, 74.0) is not None and U.geom(64, 64, 74.1) is None and U.geom(64, 64, 100) is None
    assert U.geom(64, 64, 8) is not None and U.geom(64, 64, 7.99) is None and U.geom(64, 64, 256.1) is None
    assert U.geom(0, 4) is None and U.geom(4, 0) is None and U.geom(65536, 32769) is None and U.geom(65536, 32768) is not None
    assert U.geom(8, 8, layout=1) is None
    assert U.emulate(8, 8, [(uniform(0, 8, 8), uniform(9, 8, 8))], ppd=100) is None


# ---- by hand -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b,want", HAND)
def test_hand_values(a, b, want):
    r = R.flip(uniform(a), uniform(b))
    assert abs(r.flip - want).max() < 1e-8 and abs(r.mean - want) < 1e-8 and (r.feature < 1e-7).all()
    e = U.emulate(24, 18, [(uniform(a), uniform(b))])[0]
    assert np.abs(e.flip - want).max() <= U.TOL_PIXEL and abs(e.mean - want) <= U.TOL_MEAN
    # a flat picture has no features: the zero-sum filters act on differences from the centre sample, which are exactly 0
    assert (e.feature == 0).all() and (e.flip == e.color).all()


def test_identical_pictures_are_bitwise_zero():
    for kind in U.KINDS:
        a, _ = U.pair(70, 21, kind, 3)
        e = U.emulate(70, 21, [(a, a.copy())])[0]
        for m in (e.flip, e.color, e.feature):
            assert not m.view(np.uint32).any()
        assert (e.mean, e.min, e.max) == (0.0, 0.0, 0.0)


# ---- the emulated kernels against the restatement --------------------------------------------------------------------------------
def test_emulation_against_the_restatement(capsys):
    """every shape x every kind at the default ppd, and ppd 30 and 8 (smaller radii inside the same halo); prints the largest
    differences: tests/flip_util.py's TOL_PIXEL and TOL_MEAN are 4 x these"""
    worst_px = worst_mean = 0.0
    cases = [(w, h, k, U.DEFAULT_PPD) for (w, h) in SHAPES for k in U.KINDS] + [(70, 37, k, p) for k in U.KINDS for p in (30.0, 8.0, 74.0)]
    for w, h, kind, ppd in cases:
        a, b = U.pair(w, h, kind)
        e = U.emulate(w, h, [(a, b)], ppd=ppd)[0]
        d, dm = U.close(e, R.flip(a, b, ppd))
        worst_px, worst_mean = max(worst_px, d), max(worst_mean, dm)
        # the picture's numbers are those of the returned map
        m = e.flip.astype(np.float64)
        assert abs(e.mean - m.sum() / m.size) <= 1e-12 * max(e.mean, 1e-300) and e.min == m.min() and e.max == m.max()
        assert (e.flip >= 0).all() and (e.flip <= 1 + 1e-6).all()
    with capsys.disabled():
        print(f"\nflip emulation against float64: {worst_px:.3e} per pixel, {worst_mean:.3e} on the mean")
    assert 4 * worst_px <= U.TOL_PIXEL * 1.0001 and 4 * worst_mean <= U.TOL_MEAN * 1.0001  # the recorded figures still hold


def test_pitches_slots_and_reused_buffers():
    # 33 x 17 at a pitch of exactly 99 bytes, and with padded, differing pitches for the two sides
    a, b = U.pair(33, 17, "noise", 1)
    want = R.flip(a, b)
    assert a.strides[0] == 99
    tight = U.emulate(33, 17, [(a, b)])[0]
    pa, ka = U.padded(a, 131)
    pb, kb = U.padded(b, 256, 0x3C)
    loose = U.emulate(33, 17, [(pa, pb)])[0]
    U.close(tight, want)
    for n in ("flip", "color", "feature"):
        assert np.array_equal(getattr(tight, n), getattr(loose, n))
    assert (tight.mean, tight.min, tight.max) == (loose.mean, loose.min, loose.max)
    # 130 x 70 in slot 5 of a batch of 8, other pairs around it; then a second, smaller compute on the same buffers
    pairs = [U.pair(130, 70, U.KINDS[i % len(U.KINDS)], 10 + i) for i in range(8)]
    pairs[5] = U.pair(130, 70, "step", 99)
    got = U.emulate(130, 70, pairs + pairs[5:7], batches=[8, 2], cap=8)
    U.close(got[5], R.flip(*pairs[5]))
    U.close(got[2], R.flip(*pairs[2]))
    for n in ("flip", "color", "feature"):
        assert np.array_equal(getattr(got[8], n), getattr(got[5], n)) and np.array_equal(getattr(got[9], n), getattr(got[6], n))
    assert got[8].mean == got[5].mean and not np.array_equal(got[5].flip, got[4].flip)


# ---- seeded mistakes -------------------------------------------------------------------------------------------------------------
def _mistake_pictures():
    out = [U.pair(48, 40, k, 5) for k in ("noise", "step", "pixel", "smooth")]
    out.append((uniform((255, 0, 255), 48, 40), U.pair(48, 40, "noise", 6)[1]))  # saturated colours: filtered values leave the gamut
    yy, xx = np.indices((40, 48))
    stripes = np.where(((xx // 2) % 2)[..., None] == 0, np.array([0, 0, 255]), np.array([255, 255, 0])).astype(np.uint8)
    out.append((stripes, np.roll(stripes, 1, axis=1)))
    redgreen = np.where(((xx // 2) % 2)[..., None] == 0, np.array([255, 0, 0]), np.array([0, 255, 0])).astype(np.uint8)
    out.append((redgreen, uniform((255, 0, 0), 48, 40)))  # filtered values far outside the gamut: the clamp of step 3
    return out


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_seeded_mistakes_are_far_outside_the_tolerance(mistake, capsys):
    moved = 0.0
    for a, b in _mistake_pictures():
        good, bad = R.flip(a, b), R.flip(a, b, mistake=mistake)
        moved = max(moved, float(np.abs(good.flip - bad.flip).max()))
    with capsys.disabled():
        print(f"\nflip mistake {mistake}: moves a map by {moved:.3e}")
    assert moved > 10 * U.TOL_PIXEL, (mistake, moved)


# ---- the host side of the CLI ------------------------------------------------------------------------------------------------------
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
HOST = os.path.join(ROOT, "turbo-metrics_amd", "host")


def test_pfm_writer_round_trips_through_the_clis_reader(tmp_path):
    exe = str(tmp_path / "flip_pfm_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "host", "flip_pfm_test.cpp"),
                           os.path.join(HOST, "libturbometrics_host.a"), "-L" + os.path.join(ROOT, "turbo-metrics_amd"), "-lturbometrics_hip", "-lz", "-ldl",
                           "-Wl,-rpath," + os.path.join(ROOT, "turbo-metrics_amd")])
    for w, h in ((1, 1), (7, 5), (130, 3)):
        path = str(tmp_path / f"m{w}x{h}.pfm")
        out = subprocess.run([exe, path, str(w), str(h)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and out.stdout == "pfm ok\n", (out.stdout, out.stderr)
        raw = open(path, "rb").read()
        head = b"Pf\n%d %d\n-1.0\n" % (w, h)
        assert raw.startswith(head)
        rows = np.frombuffer(raw[len(head):], "<f4").reshape(h, w)[::-1]  # rows run bottom to top
        yy, xx = np.indices((h, w))
        assert np.array_equal(rows, ((xx + 1) / 1024 - yy * 3).astype(np.float32))


def test_cli_options_of_flip():
    """what the command line refuses before it opens a file or a device (exit code 2, like every usage error), and what the help says"""
    def run(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)
    for args, msg in ((("a", "b", "--flip-ppd", "30"), "belong to '-m flip'"), (("a", "b", "--flip-map", "x"), "belong to '-m flip'"),
                      (("a", "b", "-m", "flip", "--flip-ppd", "300"), "invalid value '300' for '--flip-ppd <X>'"),
                      (("a", "b", "-m", "flip", "--flip-ppd", "7.9"), "invalid value '7.9'"), (("a", "b", "-m", "flip", "--flip-ppd", "x"), "invalid value 'x'"),
                      (("a", "b", "-mflip", "--flip-ppd"), "a value is required for '--flip-ppd <X>'"),
                      (("a", "b", "-m", "flip", "--flip-map"), "a value is required for '--flip-map <PREFIX>'"),
                      (("a", "b", "-m", "flop"), "invalid value 'flop'")):
        out = run(*args)
        assert out.returncode == 2 and msg in out.stderr and out.stdout == "", (args, out.stderr)
    for extra in (("--devices", "2"), ("--ranks", "2"), ("--loop", "deferred")):
        out = run("a", "b", "-m", "flip", "--flip-ppd=30", "--flip-map=p", *extra)
        assert out.returncode == 1 and "-m flip does not run with" in out.stderr
    out = run("missing_a.ppm", "missing_b.ppm", "-m", "flip", "--flip-ppd", "67")  # the options parse: the run ends at the file
    assert out.returncode == 1 and "flip" not in out.stderr.lower()
    text = run("--help").stdout
    assert all(s in text for s in ("-m flip", "--flip-ppd <X>", "--flip-map <PREFIX>"))
    assert "turbo_metrics_flip.h" in open(os.path.join(HOST, "Makefile")).read()
