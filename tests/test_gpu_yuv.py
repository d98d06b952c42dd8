"""GPU tier of plane-wise YUV PSNR and SSIM: libturbometrics_yuv.so through tm.Yuv against the emulated kernels
(sse, maps and ssim_sum bit-identical: the same arithmetic in the same order) and the numpy restatement (sse and maps bit-identical,
ssim_sum within the derived n 2^-53 sum |v|); pitches, memory kinds, repeats, 1080p and 2160p."""
import numpy as np
import pytest

from tests import yuv_ref as R
from tests import yuv_util as U
from tm_pkg import tm

pytestmark = pytest.mark.gpu

T = U.tile()
E = 4 * (T + 1)
SIZES = ((16, 16), (17, 17), (18, 16), (24, 16), (67, 35), (130, 70),
         (E - 4, E + 4), (E, E), (E + 4, E - 4), (2 * E - 8, 2 * E + 8), (2 * E, 2 * E), (2 * E + 8, 2 * E - 7))
KINDS = ("noise", "smooth", "extreme")


@pytest.fixture(scope="module", autouse=True)
def _hip():
    tm.init_hip(0)


def _torch(p):
    """the same bytes as a torch tensor (signed views: torch has no unsigned 16- / 32-bit kernels to copy with)"""
    import torch
    return torch.from_numpy(p.view({np.uint16: np.int16, np.uint32: np.int32}.get(p.dtype.type, p.dtype)))


def _compute(y, frames, mem="host"):
    """the pairs of plane arrays as slots 0 .. n-1 of one compute -> [yuv_util.Got]"""
    import torch
    keep = []
    for s, (pr, pd) in enumerate(frames):
        if mem == "device":
            pr, pd = [_torch(np.ascontiguousarray(p)).cuda() for p in pr], [_torch(np.ascontiguousarray(p)).cuda() for p in pd]
            torch.cuda.synchronize()
        elif mem == "pinned":
            pr, pd = [_torch(np.ascontiguousarray(p)).pin_memory() for p in pr], [_torch(np.ascontiguousarray(p)).pin_memory() for p in pd]
        keep.append((pr, pd))
        y.set_pair(s, pr, pd)
    y.compute(len(frames))
    return [U.Got(f.sse, [y.ssim_map(s, p) for p in range(3)], f.ssim_sum) for s, f in enumerate(y.frames(len(frames)))]


def _same(a, b):
    return a.sse == b.sse and a.ssim_sum == b.ssim_sum and all(x.tobytes() == z.tobytes() for x, z in zip(a.maps, b.maps))


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_library_against_emulation_and_restatement(layout, bits):
    for w, h in SIZES:
        pairs = [U.pair(w, h, bits, k, seed=w + h) for k in KINDS]
        frames = U.frames_of(layout, pairs, w, h, bits)
        emul = U.emulate(w, h, layout, bits, [len(pairs)], frames)
        with tm.Yuv(w, h, layout, bits, batch=len(pairs)) as y:
            got = _compute(y, frames)
            fr = y.frames(len(pairs))
        for g, e, f, (a, b) in zip(got, emul, fr, pairs):
            assert _same(g, e), (w, h)
            want = R.frame(a, b, bits)
            why = U.agrees(g, want)
            assert why is None, (w, h, why)
            assert f.ssim == tuple(s / m.size for s, m in zip(f.ssim_sum, g.maps))


def test_pitches_memory_kinds_and_repeats():
    w, h, bits = 130, 70, 10
    pairs = [U.pair(w, h, bits, k, seed=4) for k in KINDS]
    for layout in ("p016", "i420", "i420p10"):
        tight = U.frames_of(layout, pairs, w, h, bits)
        loose = U.frames_of(layout, pairs, w, h, bits, pad=5 if layout != "i420p10" else 1)
        with tm.Yuv(w, h, layout, bits, batch=3) as y:
            first = _compute(y, tight)
            again = _compute(y, tight)
            for a, b in zip(first, again):  # two computes of the same input: identical bytes
                assert _same(a, b)
            for frames in (tight, loose):
                for mem in ("host", "pinned", "device"):
                    for a, b in zip(first, _compute(y, frames, mem)):
                        assert _same(a, b), (layout, mem)
            short = _compute(y, tight[1:2])  # a smaller compute on the same buffers
            assert _same(short[0], first[1])
        for g, (a, b) in zip(first, pairs):
            assert U.agrees(g, R.frame(a, b, bits)) is None


def test_state_rules():
    w, h = 32, 32
    (pr, pd), = U.frames_of("nv12", [U.pair(w, h, 8, "noise", 1)], w, h, 8)
    with tm.Yuv(w, h, "nv12", 8, batch=2) as y:
        assert y.mem_usage() > 0
        y.set_pair(0, pr, pd)
        with pytest.raises(tm.yuv.YuvError) as e:
            y.compute(2)  # slot 1 was not set
        assert e.value.code == tm.ffi.TM_ERR_STATE
        y.compute(1)
        with pytest.raises(tm.yuv.YuvError) as e:
            y.compute(1)  # every compute consumes its pictures
        assert e.value.code == tm.ffi.TM_ERR_STATE
        with pytest.raises(tm.yuv.YuvError) as e:
            y.ssim_map(1, 0)  # not a slot of the last compute
        assert e.value.code == tm.ffi.TM_ERR_STATE
        assert y.ssim_map(0, 1).shape == (3, 3)


@pytest.mark.parametrize("w,h,layout,bits", [(1920, 1080, "nv12", 8), (3840, 2160, "p016", 10)])
def test_full_size(w, h, layout, bits):
    """one pair in device memory against the restatement"""
    pairs = [U.pair(w, h, bits, "smooth", seed=2)]
    frames = U.frames_of(layout, pairs, w, h, bits)
    with tm.Yuv(w, h, layout, bits, batch=1) as y:
        g = _compute(y, frames, "device")[0]
    assert U.agrees(g, R.frame(*pairs[0], bits)) is None


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
import json  # noqa: E402
import os  # noqa: E402
import re  # noqa: E402
import subprocess  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
GOLDEN = os.path.join(ROOT, "tests", "golden", "yuv_parent_cli.json")
CW, CH, CN = 98, 42, 3  # 2 columns and 2 rows beyond the last luma block; chroma 49 x 21: one of each
PSNR_NAMES = ["psnr_y", "psnr_u", "psnr_v", "psnr_avg"]
SSIM_NAMES = ["ssim_y", "ssim_u", "ssim_v", "ssim_all"]
FORMATS = ("json-lines", "json", "csv", "default")


def _cli(*args, cli=CLI):
    out = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def _y4m_pairs(d, pairs, names=("a.y4m", "b.y4m")):
    from tests.test_gpu_xpsnr import _y4m
    a, b = os.path.join(str(d), names[0]), os.path.join(str(d), names[1])
    _y4m(a, CW, CH, pairs, 0)
    _y4m(b, CW, CH, pairs, 1)
    return a, b


def _pairs():
    return [U.pair(CW, CH, 8, "smooth", seed=30 + i) for i in range(CN)]


def _binding(pairs, cap=0.0):
    """per frame the eight values, the eight sequence values, and the luma maps, from tm.Yuv and the library's host functions"""
    frames = U.frames_of("i420", pairs, CW, CH, 8)
    with tm.Yuv(CW, CH, "i420", 8, batch=len(pairs)) as y:
        for s, (pr, pd) in enumerate(frames):
            y.set_pair(s, pr, pd)
        y.compute(len(pairs))
        fr = y.frames(len(pairs))
        maps = [y.ssim_map(s, 0) for s in range(len(pairs))]
        ns = y.samples()
    rows = []
    for f in fr:
        ps = [tm.yuv.psnr(s, n, 8, cap) for s, n in zip(f.sse, ns)] + [tm.yuv.psnr(sum(f.sse), sum(ns), 8, cap)]
        rows.append(ps + list(f.ssim) + [tm.yuv.ssim_all(f.ssim, CW, CH)])
    tot = [sum(f.sse[c] for f in fr) for c in range(3)]
    seq = [tm.yuv.psnr(t, n * len(fr), 8, cap) for t, n in zip(tot, ns)] + [tm.yuv.psnr(sum(tot), sum(ns) * len(fr), 8, cap)]
    for k in range(4, 8):
        acc = 0.0
        for r in rows:
            acc += r[k]
        seq.append(acc / len(rows))
    return rows, seq, maps


# what the parent commit's binary printed for these arguments on the inputs of _parent_files(dir): recorded once with
# record_parent_cli(<the parent's turbo-metrics>, GOLDEN, <a scratch directory>) on an MI355X
PARENT_CASES = {
    "y4m_psnr_ssim_default": ("y4m", ["-m", "psnr", "-m", "ssim"]),
    "y4m_ssimu_xpsnr_json": ("y4m", ["-m", "ssimulacra2", "-m", "xpsnr", "--output", "json"]),
    "y4m_psnr_xpsnr_motion_jsonl": ("y4m", ["-m", "psnr", "-m", "xpsnr", "--motion", "--output", "json-lines"]),
    "y4m_vif_adm_scenes_csv": ("y4m", ["-m", "vif", "-m", "adm", "--scenes", "--batch", "2", "--output", "csv"]),
    "y4m_xpsnr_cambi_csv": ("y4m", ["-m", "xpsnr", "-m", "cambi", "--output", "csv"]),
    "ppm_ssim_flip_jsonl": ("ppm", ["-m", "ssim", "-m", "flip", "--output", "json-lines"]),
    "ppm_psnr_ssimu_default": ("ppm", ["-m", "psnr", "-m", "ssimulacra2"]),
}


def _ppm_pair(d):
    rng = np.random.default_rng(77)
    yy, xx = np.indices((CH, CW))
    a = np.stack([(xx * 255) // (CW - 1), (yy * 255) // (CH - 1), (xx + yy) % 256], -1).astype(np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    out = []
    for name, img in (("a.ppm", a), ("b.ppm", b)):
        p = os.path.join(str(d), name)
        with open(p, "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (CW, CH) + np.ascontiguousarray(img).tobytes())
        out.append(p)
    return out


def _parent_files(d, kind):
    return _ppm_pair(d) if kind == "ppm" else _y4m_pairs(d, _pairs())


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


def test_cli_without_the_new_values_is_byte_identical_with_the_parents(tmp_path):
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(PARENT_CASES)
    got = _run_parent_cases(CLI, tmp_path)
    for name in PARENT_CASES:
        assert got[name] == want[name], name
        # no new column name, as a whole word ("xpsnr_y" is an old one)
        assert not re.search(r"(?<![a-z0-9_])(" + "|".join(PSNR_NAMES + SSIM_NAMES) + r")(?![a-z0-9_])|yuv", got[name].lower()), name


@pytest.mark.parametrize("beside", [(), ("-m", "ssimulacra2"), ("-m", "xpsnr")])
@pytest.mark.parametrize("sel", ["psnr", "ssim", "both"])
def test_cli_against_the_binding_in_every_output_format(tmp_path, sel, beside):
    pairs = _pairs()
    a, b = _y4m_pairs(tmp_path, pairs)
    rows, seq, _ = _binding(pairs)
    cols = {"psnr": list(range(4)), "ssim": list(range(4, 8)), "both": list(range(8))}[sel]
    names = [(PSNR_NAMES + SSIM_NAMES)[k] for k in cols]
    flags = {"psnr": ("-m", "psnr-yuv"), "ssim": ("-mssim-yuv",), "both": ("-m", "ssim-yuv", "--metrics", "psnr-yuv")}[sel]
    base = (a, b, *beside, *flags)
    first = {(): [], ("-m", "ssimulacra2"): ["ssimulacra2"], ("-m", "xpsnr"): ["xpsnr_y", "xpsnr_u", "xpsnr_v"]}[beside]
    plain = {fmt: _cli(a, b, *beside, "--output", fmt) for fmt in FORMATS} if beside else {}
    # json-lines: one line per frame, then the aggregates with the sequence values
    lines = [json.loads(x) for x in _cli(*base, "--output", "json-lines").splitlines() if x.strip()]
    assert len(lines) == CN + 1
    for i in range(CN):
        assert list(lines[i]) == first + names and [lines[i][n] for n in names] == [rows[i][k] for k in cols]
    agg = lines[CN]
    assert agg["frame_count"] == CN and list(agg)[-len(names):] == names
    for n, k in zip(names, cols):
        assert agg[n]["sequence"] == seq[k] and agg[n]["min"] == min(r[k] for r in rows) and agg[n]["max"] == max(r[k] for r in rows)
    # json
    js = json.loads(_cli(*base, "--output", "json"))
    assert list(js)[-len(names):] == names
    for n, k in zip(names, cols):
        assert js[n]["scores"] == [r[k] for r in rows] and js[n]["sequence"] == seq[k] and js[n]["stats"]["max"] == max(r[k] for r in rows)
    # csv: the header, a row per frame as it is computed, then the header and the rows again
    out = _cli(*base, "--output", "csv").splitlines()
    assert out[0] == ",".join(first + names) == out[CN + 1] and len(out) == 2 * CN + 2
    for i in range(CN):
        assert [float(x) for x in out[1 + i].split(",")[-len(names):]] == [rows[i][k] for k in cols] and out[CN + 2 + i] == out[1 + i]
    # default
    txt = _cli(*base)
    assert all(f"{n.upper()}: Stats {{" in txt for n in names)
    assert ("PSNR-YUV (sequence): y " in txt) == (sel != "ssim") and ("SSIM-YUV (sequence): y " in txt) == (sel != "psnr")
    if beside:  # the other metric's output is unchanged and comes first
        pl = [json.loads(x) for x in plain["json-lines"].splitlines() if x.strip()]
        for i in range(CN):
            assert [lines[i][n] for n in first] == [pl[i][n] for n in first]
        assert [agg[n] for n in first] == [pl[CN][n] for n in first]
        assert out[1].split(",")[:len(first)] == plain["csv"].splitlines()[1].split(",") and txt.startswith(plain["default"])
        pj = json.loads(plain["json"])
        assert all(js[n] == pj[n] for n in first)


def test_cli_cap_infinity_and_map(tmp_path):
    pairs = _pairs()
    same = [(r, r) for r, _ in pairs[:1]] + pairs[1:2]
    a, b = _y4m_pairs(tmp_path, same)
    # identical pictures: +inf, printed the way -m xpsnr prints it; with --psnr-yuv-cap libvmaf's 6 D + 12 = 60
    rows = _cli(a, b, "-m", "xpsnr", "-m", "psnr-yuv", "-m", "ssim-yuv", "--output", "csv").splitlines()
    cells = rows[1].split(",")
    assert cells[3:7] == [cells[0]] * 4 and "inf" in cells[0].lower() and [float(x) for x in cells[7:]] == [1.0] * 4
    lines = _cli(a, b, "-m", "xpsnr", "-m", "psnr-yuv", "--output", "json-lines").splitlines()
    raw = lines[0]
    assert raw.split('"psnr_y":')[1].split(",")[0] == raw.split('"xpsnr_y":')[1].split(",")[0]
    want, seq, maps = _binding(same, cap=60.0)
    capped = [json.loads(x) for x in _cli(a, b, "-m", "psnr-yuv", "--psnr-yuv-cap", "--output", "json-lines").splitlines()]
    assert [capped[0][n] for n in PSNR_NAMES] == [60.0] * 4 and [capped[1][n] for n in PSNR_NAMES] == want[1][:4]
    assert [capped[2][n]["sequence"] for n in PSNR_NAMES] == seq[:4]
    # --ssim-yuv-map: every pair's luma map
    prefix = str(tmp_path / "map_")
    _cli(a, b, "-m", "ssim-yuv", "--ssim-yuv-map", prefix, "--output", "csv")
    mw, mh = tm.yuv.map_size(CW, CH, 0)
    for i in range(2):
        raw = open(prefix + "%06d.pfm" % i, "rb").read()
        head = b"Pf\n%d %d\n-1.0\n" % (mw, mh)
        assert raw.startswith(head)
        assert np.array_equal(np.frombuffer(raw[len(head):], "<f4").reshape(mh, mw)[::-1], maps[i])
    assert not os.path.exists(prefix + "000002.pfm")


def test_cli_refuses_rgb_input_and_ranks(tmp_path):
    pa, pb = _ppm_pair(tmp_path)
    for sel in ("psnr-yuv", "ssim-yuv"):
        out = subprocess.run([CLI, pa, pb, "-m", sel], capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "psnr-yuv / ssim-yuv need 4:2:0 YUV input" in out.stderr, (out.returncode, out.stderr)
    a, b = _y4m_pairs(tmp_path, _pairs()[:1])
    out = subprocess.run([CLI, a, b, "-m", "psnr-yuv", "--ranks", "2"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "do not run with --ranks" in out.stderr, (out.returncode, out.stderr)
