"""GPU tier of LDR-FLIP: libturbometrics_flip.so through tm.Flip against the emulated kernels and the float64
restatement, inside the tolerance measured on the CPU (tests/flip_util.py); the hand values; pitches, slots, memory kinds, repeats."""
import numpy as np
import pytest

from tests import flip_ref as R
from tests import flip_util as U
from tm_pkg import tm

pytestmark = pytest.mark.gpu

T_W, T_H, HALO = U.tile()
SHAPES = ((1, 1), (7, 5), (21, 21), (T_W - 1, T_H + 1), (T_W, T_H), (T_W + 1, T_H - 1))
HAND = (((0, 0, 0), (255, 255, 255), 0.96737976), ((127, 127, 127), (128, 128, 128), 0.02988465), ((255, 0, 0), (0, 255, 0), 0.98666228))


@pytest.fixture(scope="module", autouse=True)
def _hip():
    tm.init_hip(0)


def _got(f, slot, frame):
    return type("Got", (), dict(flip=f.map(slot), color=f.map(slot, "color"), feature=f.map(slot, "feature"), mean=frame.mean, min=frame.min,
                                max=frame.max))


def _compute(f, pairs, device=False):
    """the pairs as slots 0 .. n-1 of one compute"""
    import torch
    keep = []
    for i, (a, b) in enumerate(pairs):
        if device:
            a, b = torch.from_numpy(np.ascontiguousarray(a)).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda()
            torch.cuda.synchronize()
        keep.append((a, b))
        f.set_pair(i, a, b)
    f.compute(len(pairs))
    return [_got(f, i, fr) for i, fr in enumerate(f.frames(len(pairs)))]


def _picture_numbers(g):
    m = g.flip.astype(np.float64)
    assert abs(g.mean - m.sum() / m.size) <= 1e-12 * max(g.mean, 1e-300) and g.min == m.min() and g.max == m.max()


def test_abi_loads_and_refuses():
    assert tm.flip.radius() == (10, 9) and tm.flip.radius(100) == (14, 13)
    for ppd in (74.1, 100, 7.9, 300):
        with pytest.raises(tm.flip.FlipError) as e:
            tm.Flip(16, 16, ppd=ppd)
        assert e.value.code == tm.ffi.TM_ERR_UNSUPPORTED
    with tm.Flip(16, 16, batch=2) as f:
        assert f.mem_usage() >= 2 * 3 * 16 * 16 * 4
        a = np.zeros((16, 16, 3), np.uint8)
        f.set_pair(0, a, a)
        with pytest.raises(tm.flip.FlipError) as e:
            f.compute(2)  # slot 1 was not set
        assert e.value.code == tm.ffi.TM_ERR_STATE
        with pytest.raises(ValueError):
            f.set_pair(0, a.astype(np.float32), a)
        with pytest.raises(ValueError):
            f.map(0, "other")


@pytest.mark.parametrize("a,b,want", HAND)
def test_hand_values(a, b, want):
    w, h = 70, 20
    pa, pb = (np.ascontiguousarray(np.broadcast_to(np.array(c, np.uint8), (h, w, 3))) for c in (a, b))
    with tm.Flip(w, h, batch=1) as f:
        g = _compute(f, [(pa, pb)])[0]
    assert np.abs(g.flip - want).max() <= U.TOL_PIXEL and abs(g.mean - want) <= U.TOL_MEAN
    assert (g.feature == 0).all() and abs(g.min - want) <= U.TOL_PIXEL and abs(g.max - want) <= U.TOL_PIXEL


def test_identical_pictures_are_bitwise_zero():
    pairs = [(U.pair(70, 21, k, 3)[0],) * 2 for k in U.KINDS]
    with tm.Flip(70, 21, batch=len(pairs)) as f:
        for g in _compute(f, pairs):
            for m in (g.flip, g.color, g.feature):
                assert not m.view(np.uint32).any()
            assert (g.mean, g.min, g.max) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("w,h", SHAPES)
def test_library_against_emulation_and_restatement(w, h):
    pairs = [U.pair(w, h, k, 2) for k in U.KINDS]
    emul = U.emulate(w, h, pairs)
    with tm.Flip(w, h, "rgb8", batch=len(pairs)) as f:
        host = _compute(f, pairs)
        dev = _compute(f, pairs, device=True)
    for g, d, e, (a, b) in zip(host, dev, emul, pairs):
        U.close(g, R.flip(a, b))
        for n in ("flip", "color", "feature"):
            assert np.abs(getattr(g, n).astype(np.float64) - getattr(e, n)).max() <= U.TOL_PIXEL, n
            assert np.array_equal(getattr(g, n), getattr(d, n)), n  # host and device memory
        assert abs(g.mean - e.mean) <= U.TOL_MEAN and (g.mean, g.min, g.max) == (d.mean, d.min, d.max)
        _picture_numbers(g)


def test_pitches():
    a, b = U.pair(33, 17, "noise", 1)
    assert a.strides[0] == 99
    pa, ka = U.padded(a, 131)
    pb, kb = U.padded(b, 256, 0x3C)
    with tm.Flip(33, 17, batch=2) as f:
        tight, loose = _compute(f, [(a, b), (pa, pb)])
        import torch
        da, db = torch.from_numpy(ka).cuda(), torch.from_numpy(kb).cuda()
        f.set_pair(0, da.view(17, 131), db.view(17, 256))
        f.compute(1)
        dev = _got(f, 0, f.frames(1)[0])
    U.close(tight, R.flip(a, b))
    for other in (loose, dev):
        for n in ("flip", "color", "feature"):
            assert np.array_equal(getattr(tight, n), getattr(other, n))
        assert (tight.mean, tight.min, tight.max) == (other.mean, other.min, other.max)


def test_slot_5_of_8_and_repeats():
    pairs = [U.pair(130, 70, U.KINDS[i % len(U.KINDS)], 10 + i) for i in range(8)]
    pairs[5] = U.pair(130, 70, "step", 99)
    with tm.Flip(130, 70, batch=8) as f:
        first = _compute(f, pairs)
        again = _compute(f, pairs)
        short = _compute(f, pairs[5:7])  # a smaller compute on the same buffers
    U.close(first[5], R.flip(*pairs[5]))
    U.close(first[2], R.flip(*pairs[2]))
    e = U.emulate(130, 70, [pairs[5]])[0]
    assert np.abs(first[5].flip.astype(np.float64) - e.flip).max() <= U.TOL_PIXEL and abs(first[5].mean - e.mean) <= U.TOL_MEAN
    for x, y in list(zip(first, again)) + [(first[5], short[0]), (first[6], short[1])]:
        assert x.flip.tobytes() == y.flip.tobytes() and x.color.tobytes() == y.color.tobytes() and x.feature.tobytes() == y.feature.tobytes()
        assert (x.mean, x.min, x.max) == (y.mean, y.min, y.max)
    assert not np.array_equal(first[5].flip, first[4].flip)
    for g in first:
        _picture_numbers(g)


@pytest.mark.parametrize("ppd", (30.0, 8.0, 74.0))
def test_other_ppd(ppd):
    pairs = [U.pair(70, 37, k, 4) for k in ("noise", "step", "pixel")]
    with tm.Flip(70, 37, ppd=ppd, batch=3) as f:
        for g, (a, b) in zip(_compute(f, pairs), pairs):
            U.close(g, R.flip(a, b, ppd))


def test_1080p():
    """one 1920 x 1080 pair; the restatement and the emulation run on three windows of it (two corners, where coordinates clamp, and the
    middle), and are compared where the window's own border is further away than the radius"""
    w, h = 1920, 1080
    rng = np.random.default_rng(11)
    yy, xx = np.indices((h, w))
    a = np.stack([(xx * 255) // (w - 1), (yy * 255) // (h - 1), ((xx // 16 + yy // 16) % 2) * 200], -1).astype(np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-20, 21, (h, w, 3)) * (rng.random((h, w, 1)) < 0.1), 0, 255).astype(np.uint8)
    with tm.Flip(w, h, batch=1) as f:
        g = _compute(f, [(a, b)], device=True)[0]
    _picture_numbers(g)
    assert 0 < g.mean < 1 and g.max <= 1 + 1e-6 and g.min >= 0
    cw, ch, m = 150, 90, HALO
    for x0, y0 in ((0, 0), (w - cw, h - ch), (900, 500)):
        ca, cb = np.ascontiguousarray(a[y0:y0 + ch, x0:x0 + cw]), np.ascontiguousarray(b[y0:y0 + ch, x0:x0 + cw])
        r, e = R.flip(ca, cb), U.emulate(cw, ch, [(ca, cb)])[0]
        ys = slice(0 if y0 == 0 else m, ch if y0 + ch == h else ch - m)
        xs = slice(0 if x0 == 0 else m, cw if x0 + cw == w else cw - m)
        for n in ("flip", "color", "feature"):
            got = getattr(g, n)[y0:y0 + ch, x0:x0 + cw][ys, xs].astype(np.float64)
            assert np.abs(got - getattr(r, n)[ys, xs]).max() <= U.TOL_PIXEL, (n, x0, y0)
            assert np.abs(got - getattr(e, n)[ys, xs]).max() <= U.TOL_PIXEL, (n, x0, y0)


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
import json  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
GOLDEN = os.path.join(ROOT, "tests", "golden", "flip_parent_cli.json")
CW, CH = 96, 40


def _cli(*args, cli=CLI):
    out = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def _ppm(path, img):
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(img).tobytes())


def _ppm_pair(d, kind="smooth", seed=8):
    a, b = U.pair(CW, CH, kind, seed)
    pa, pb = os.path.join(str(d), "a.ppm"), os.path.join(str(d), "b.ppm")
    _ppm(pa, a)
    _ppm(pb, b)
    return pa, pb, a, b


# what the parent commit's binary printed for these arguments on the inputs of _parent_files(dir): recorded once with
# record_parent_cli(<the parent's turbo-metrics>, GOLDEN, <a scratch directory>) on an MI355X
PARENT_CASES = {
    "ppm_ssimu_default": ("ppm", ["-m", "ssimulacra2"]),
    "ppm_psnr_ssimu_json": ("ppm", ["-m", "psnr", "-m", "ssimulacra2", "--output", "json"]),
    "ppm_psnr_jsonl": ("ppm", ["-m", "psnr", "--output", "json-lines"]),
    "ppm_ssim_csv": ("ppm", ["-m", "ssim", "-m", "ssimulacra2", "--output", "csv"]),
    "y4m_vif_cambi_scenes_csv": ("y4m", ["-m", "vif", "-m", "cambi", "--scenes", "--batch", "3", "--output", "csv"]),
    "y4m_xpsnr_motion_jsonl": ("y4m", ["-m", "xpsnr", "--motion", "--output", "json-lines"]),
}


def _parent_files(d, kind):
    if kind == "ppm":
        return _ppm_pair(d)[:2]
    from tests import motion_util
    from tests.test_gpu_motion import _y4m
    seq = motion_util.sequence(160, 96, 4, 8, "smooth")
    a, b = os.path.join(d, "a.y4m"), os.path.join(d, "b.y4m")
    _y4m(a, 160, 96, seq, 8, 1)
    _y4m(b, 160, 96, [(p + 1) % 256 for p in seq], 8, 2)
    return a, b


def _run_parent_cases(cli, tmp):
    out = {}
    for kind in ("ppm", "y4m"):
        d = os.path.join(str(tmp), "in_" + kind)
        os.makedirs(d, exist_ok=True)
        a, b = _parent_files(d, kind)
        for name, (k, args) in PARENT_CASES.items():
            if k == kind:
                out[name] = _cli(a, b, *args, cli=cli)
    return out


def record_parent_cli(cli, dest, tmp):
    with open(dest, "w") as f:
        json.dump(_run_parent_cases(cli, tmp), f, indent=1, sort_keys=True)
        f.write("\n")


def test_cli_without_flip_is_byte_identical_with_the_parents(tmp_path):
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(PARENT_CASES)
    got = _run_parent_cases(CLI, tmp_path)
    for name in PARENT_CASES:
        assert got[name] == want[name], name
        assert "flip" not in got[name].lower()


FLIP_NAMES = ["flip", "flip_min", "flip_max"]


def _binding(a, b, ppd=None):
    with tm.Flip(CW, CH, ppd=ppd, batch=1) as f:
        f.set_pair(0, a, b)
        f.compute(1)
        fr = f.frames(1)[0]
        return [fr.mean, fr.min, fr.max], f.map(0)


@pytest.mark.parametrize("beside", [(), ("-m", "ssimulacra2")])
def test_cli_flip_in_every_output_format(tmp_path, beside):
    pa, pb, a, b = _ppm_pair(tmp_path)
    want, wmap = _binding(a, b)
    assert 0 < want[0] < 1
    base = (pa, pb, "-m", "flip", *beside)
    first = ["ssimulacra2"] if beside else []
    plain = {fmt: _cli(pa, pb, *beside, "--output", fmt) for fmt in ("json-lines", "json", "csv", "default")} if beside else {}
    lines = [json.loads(x) for x in _cli(*base, "--output", "json-lines").splitlines() if x.strip()]
    frame, agg = lines[0], lines[1]
    assert list(frame) == first + FLIP_NAMES and [frame[k] for k in FLIP_NAMES] == want
    assert agg["frame_count"] == 1 and list(agg)[-3:] == FLIP_NAMES and [agg[k]["mean"] for k in FLIP_NAMES] == want
    js = json.loads(_cli(*base, "--output", "json"))
    assert [js[k]["scores"] for k in FLIP_NAMES] == [[v] for v in want] and list(js)[-3:] == FLIP_NAMES and js["flip"]["stats"]["max"] == want[0]
    rows = _cli(*base, "--output", "csv").splitlines()
    assert rows[0] == ",".join(first + FLIP_NAMES) == rows[2] and len(rows) == 4
    assert [float(x) for x in rows[1].split(",")[-3:]] == want and rows[3] == rows[1]
    txt = _cli(*base)
    assert all(f"{n}: Stats {{" in txt for n in ("FLIP", "FLIP_MIN", "FLIP_MAX"))
    if beside:  # the other metric's output is unchanged and comes first
        assert frame["ssimulacra2"] == json.loads(plain["json-lines"].splitlines()[0])["ssimulacra2"]
        assert rows[1].split(",")[0] == plain["csv"].splitlines()[1] and txt.startswith(plain["default"])
        assert js["ssimulacra2"] == json.loads(plain["json"])["ssimulacra2"]
    # --flip-map and --flip-ppd
    prefix = str(tmp_path / "map_")
    _cli(*base, "--flip-map", prefix, "--output", "csv")
    raw = open(prefix + "000000.pfm", "rb").read()
    head = b"Pf\n%d %d\n-1.0\n" % (CW, CH)
    assert raw.startswith(head) and not os.path.exists(prefix + "000001.pfm")
    assert np.array_equal(np.frombuffer(raw[len(head):], "<f4").reshape(CH, CW)[::-1], wmap)
    w30, _ = _binding(a, b, 30.0)
    assert w30 != want and [json.loads(_cli(*base, "--flip-ppd", "30", "--output", "json-lines").splitlines()[0])[k] for k in FLIP_NAMES] == w30


def test_cli_flip_refuses_yuv_and_unsupported_ppd(tmp_path):
    a, b = _parent_files(str(tmp_path), "y4m")
    out = subprocess.run([CLI, a, b, "-m", "flip"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "flip needs 8-bit RGB images" in out.stderr, (out.returncode, out.stderr)
    pa, pb, _, _ = _ppm_pair(tmp_path)
    out = subprocess.run([CLI, pa, pb, "-m", "flip", "--flip-ppd", "100"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "74.04" in out.stderr, (out.returncode, out.stderr)
