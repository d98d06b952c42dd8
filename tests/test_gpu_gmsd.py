"""GPU tier of GMSD: libturbometrics_gmsd.so through tm.Gmsd against the emulated kernel source (e1, e2, e_max, n
and the map bit for bit: the same operations in the same order, all correctly rounded) and against the float64 restatement inside the
tolerance measured on the CPU (tests/gmsd_util.py); hand values; pitches, garbage, memory kinds, repeats; the map; state rules; the CLI's
two columns against the binding in the four output and the four input formats; and the CLI without -m gmsd against a recorded run of the
parent commit's binary (tests/golden/gmsd_parent_cli.json)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gmsd_ref as R
from tests import gmsd_util as U
from tm_pkg import tm

pytestmark = pytest.mark.gpu

SIZES = U.shapes()


@pytest.fixture(scope="module", autouse=True)
def _hip():
    tm.init_hip(0)


def _torch(p):
    """the same bytes as a torch tensor (signed views: torch has no unsigned 16- / 32-bit kernels to copy with)"""
    import torch
    return torch.from_numpy(p.view({np.uint16: np.int16, np.uint32: np.int32}.get(p.dtype.type, p.dtype)))


def _compute(v, frames, mem="host"):
    """the pairs of plane arrays as slots 0 .. n-1 of one compute -> [(e1, e2, e_max, n)]"""
    import torch
    keep = []
    for s, (pr, pd) in enumerate(frames):
        if mem == "device":
            pr, pd = _torch(np.ascontiguousarray(pr)).cuda(), _torch(np.ascontiguousarray(pd)).cuda()
            torch.cuda.synchronize()
        elif mem == "pinned":
            pr, pd = _torch(np.ascontiguousarray(pr)).pin_memory(), _torch(np.ascontiguousarray(pd)).pin_memory()
        keep.append((pr, pd))
        v.set_pair(s, pr, pd)
    v.compute(len(frames))
    return [(f.e1, f.e2, f.e_max, f.n) for f in v.frames(len(frames))]


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_library_against_emulation_and_restatement(layout, bits):
    for w, h in SIZES:
        pairs = [U.pair(w, h, bits, k, seed=w + h) for k in U.KINDS]
        frames = U.planes_of(layout, pairs, bits)
        emul, emaps = U.emulate(w, h, layout, bits, [len(pairs)], frames, maps=True)
        with tm.Gmsd(w, h, layout, bits, batch=len(pairs), maps=True) as v:
            got = _compute(v, frames)
            fr = v.frames(len(pairs))
            maps = [v.map(s) for s in range(len(pairs))]
        for kind, g, e, f, m, em, (a, b) in zip(U.KINDS, got, emul, fr, maps, emaps, pairs):
            assert g == e, (w, h, kind)  # bit for bit
            assert m.dtype == np.float32 and np.array_equal(m, em), (w, h, kind)
            want = R.gmsd(a, b, bits)
            assert g[3] == want.n and abs(f.gmsd - want.gmsd) <= U.ABS_TOL and abs(f.gmsm - want.gmsm) <= U.ABS_TOL, (w, h, kind)
            if kind == "identical":
                assert g[:3] == (0.0, 0.0, 0.0) and f.gmsd == 0.0 and f.gmsm == 1.0


def test_hand_values():
    for layout, bits in (("y8", 8), ("y16_msb", 10), ("y16_low", 16), ("y10_packed", 10)):
        k = 1 << (bits - 8)
        flats = [(np.zeros((4, 4), np.int64), np.full((4, 4), v * k, np.int64)) for v in (1, 100, 255)]
        with tm.Gmsd(4, 4, layout, bits, batch=3) as v:
            _compute(v, U.planes_of(layout, flats, bits))
            fr = v.frames(3)
        for f, val in zip(fr, (1, 100, 255)):
            e = 128.0 * val * val / (128.0 * val * val + 24480.0)
            assert f.n == 4 and f.gmsd == 0.0 and abs(f.gmsm - (1 - e)) < 1e-6 and abs(f.e_max - e) < 1e-6, (layout, val)
            assert f.e1 == 4 * f.e_max and f.e2 == 4 * f.e_max * f.e_max
    # 5 x 7: the zero column and row beyond the picture enter S (the literals of tests/test_gmsd_cpu.py)
    a, b = np.zeros((7, 5), np.int64), np.full((7, 5), 60, np.int64)
    with tm.Gmsd(5, 7, "y8", 8, batch=1, maps=True) as v:
        _compute(v, U.planes_of("y8", [(a, b)], 8, pad=3))
        m = v.map(0)
    # S of the flat picture: 240 inside, 120 in column 2 and in row 3, 60 at their crossing
    S = np.array([[240, 240, 120], [240, 240, 120], [240, 240, 120], [120, 120, 60]], np.float64)
    z = np.pad(S, 1)
    gx = sum(z[1 + d:5 + d, 2:5] - z[1 + d:5 + d, 0:3] for d in (-1, 0, 1))
    gy = sum(z[2:6, 1 + d:4 + d] - z[0:4, 1 + d:4 + d] for d in (-1, 0, 1))
    A = gx * gx + gy * gy
    assert A[0, 0] == 2 * 480.0 ** 2 and A[3, 2] == (-360.0) ** 2 + (-360.0) ** 2
    assert np.abs(m - (1 - A / (A + 24480.0))).max() < 1e-6


def test_pitches_garbage_memory_kinds_and_repeats():
    w, h = SIZES[4]  # 2 TW + 1 wide: odd, one sample past a tile edge
    assert w % 2 == 1
    for layout, bits in (("y8", 8), ("y16_msb", 10), ("y16_low", 12), ("y10_packed", 10)):
        pairs = [U.pair(w, h, bits, k, seed=4) for k in ("noise", "blur", "near_peak")]
        tight = U.planes_of(layout, pairs, bits)
        loose = U.planes_of(layout, pairs, bits, pad={"y8": 4, "y10_packed": 1}.get(layout, 5))  # garbage right behind each row; y8: an odd pitch again
        assert layout != "y8" or (tight[0][0].strides[0] % 2 == 1 and loose[0][0].strides[0] % 2 == 1)
        aligned = U.planes_of(layout, pairs, bits, pad=2, aligned=True)
        with tm.Gmsd(w, h, layout, bits, batch=3) as v:
            first = _compute(v, tight)
            assert _compute(v, tight) == first  # a repeated compute: equal bits
            for frames in (tight, loose, aligned):
                for mem in ("host", "pinned", "device"):
                    assert _compute(v, frames, mem) == first, (layout, mem)
            assert _compute(v, tight[1:2]) == first[1:2]  # a smaller compute on the same buffers
        assert first == U.emulate(w, h, layout, bits, [3], tight)


def test_map_pitch_refusal_and_sums_with_and_without_maps():
    w, h = SIZES[5]
    pairs = [U.pair(w, h, 8, k, seed=6) for k in ("noise", "blur")]
    frames = U.planes_of("y8", pairs, 8)
    emul, emaps = U.emulate(w, h, "y8", 8, [2], frames, maps=True)
    with tm.Gmsd(w, h, "y8", 8, batch=2, maps=True) as v:
        with_maps = _compute(v, frames)
        h2, w2 = (h + 1) // 2, (w + 1) // 2
        buf = np.full((h2 + 1, w2 + 5), -3.0, np.float32)
        m = v.map(1, out=buf)  # rows at a caller's pitch
        assert m.shape == (h2, w2) and np.array_equal(m, emaps[1]) and (buf[:, w2:] == -3.0).all() and (buf[h2:] == -3.0).all()
        e = 1.0 - emaps[1].astype(np.float64)  # the map is 1 - e of the emulation, and its sums are the slot's
        assert abs(e.sum() - with_maps[1][0]) < 1e-3 and abs(e.max() - with_maps[1][2]) < 2e-7  # (1 - e rounds to f32 once more)
        with pytest.raises(tm.gmsd.GmsdError) as err:
            v.map(2)
        assert err.value.code == tm.ffi.TM_ERR_STATE
    with tm.Gmsd(w, h, "y8", 8, batch=2) as v:
        assert _compute(v, frames) == with_maps == emul
        with pytest.raises(tm.gmsd.GmsdError) as err:
            v.map(0)  # maps=False refuses
        assert err.value.code == tm.ffi.TM_ERR_STATE


def test_state_rules():
    w, h = 32, 32
    (pr, pd), = U.planes_of("y8", [U.pair(w, h, 8, "noise", 1)], 8)
    with tm.Gmsd(w, h, "y8", 8, batch=2) as v:
        assert v.mem_usage() > 0
        v.set_pair(0, pr, pd)
        with pytest.raises(tm.gmsd.GmsdError) as e:
            v.compute(2)  # slot 1 was not set
        assert e.value.code == tm.ffi.TM_ERR_STATE
        v.compute_async(1)
        with pytest.raises(tm.gmsd.GmsdError) as e:
            v.compute_async(1)  # a compute is pending
        assert e.value.code == tm.ffi.TM_ERR_STATE
        v.sync()
        with pytest.raises(tm.gmsd.GmsdError) as e:
            v.compute(1)  # every compute consumes its pairs
        assert e.value.code == tm.ffi.TM_ERR_STATE
        with pytest.raises(tm.gmsd.GmsdError) as e:
            v.frames(2)  # not slots of the last compute
        assert e.value.code == tm.ffi.TM_ERR_STATE
        assert v.frames(1)[0].n == 256


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gmsd_parent_cli.json")
CW, CH, CN = 99, 43, 3  # odd both ways: the zero column and row enter S
NAMES = ["gmsd", "gmsm"]
FORMATS = ("json-lines", "json", "csv", "default")


def _cli(*args, cli=CLI):
    out = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def _pairs(bits):
    return [U.pair(CW, CH, bits, "blur", seed=30 + i) for i in range(CN)]


def _y4m_pairs(d, pairs, bits):
    """the lumas as two Y4M files with flat chroma"""
    dt = np.uint8 if bits == 8 else "<u2"
    cw, ch = (CW + 1) // 2, (CH + 1) // 2
    out = []
    for side, name in enumerate(("a.y4m", "b.y4m")):
        p = os.path.join(str(d), name)
        with open(p, "wb") as f:
            f.write(f"YUV4MPEG2 W{CW} H{CH} F25:1 Ip A1:1 C420{'jpeg' if bits == 8 else 'p%d' % bits}\n".encode())
            for pr in pairs:
                f.write(b"FRAME\n" + np.asarray(pr[side], dt).tobytes() + np.full((2, ch, cw), 1 << (bits - 1), dt).tobytes())
        out.append(p)
    return out


def _raw_pairs(d, pairs, bits):
    """the same as headerless planar 4:2:0 files"""
    dt = np.uint8 if bits == 8 else "<u2"
    cw, ch = (CW + 1) // 2, (CH + 1) // 2
    out = []
    for side, name in enumerate(("a.yuv", "b.yuv")):
        p = os.path.join(str(d), name)
        with open(p, "wb") as f:
            for pr in pairs:
                f.write(np.asarray(pr[side], dt).tobytes() + np.full((2, ch, cw), 1 << (bits - 1), dt).tobytes())
        out.append(p)
    return out


def _default_values(txt, block, line):
    """the default format: ({name: value} of the `block: Stats { ... }` lines, the value on the `line (sequence): ` line)"""
    m = re.search(r"^%s: Stats \{\n(.*?)\n\}$" % re.escape(block), txt, re.S | re.M)
    q = re.search(r"^%s \(sequence\): (\S+)$" % re.escape(line), txt, re.M)
    assert m and q, (block, line)
    stats = {k: float(v) for k, v in re.findall(r"^\s+(\w+): ([^,\n]+),$", m.group(1), re.M)}
    assert {"min", "max", "mean", "p50"} <= set(stats)
    return stats, float(q.group(1))


def _binding(pairs, bits, population=False, maps=False):
    """per frame the two values and the two sequence values (pooled: from the summed sums) from tm.Gmsd and the library's host functions"""
    layout = "y8" if bits == 8 else "y16_low"
    with tm.Gmsd(CW, CH, layout, bits, batch=len(pairs), maps=maps, population=population) as v:
        _compute(v, U.planes_of(layout, pairs, bits))
        fr = v.frames(len(pairs))
        mp = [v.map(s) for s in range(len(pairs))] if maps else None
    rows = [[f.gmsd, f.gmsm] for f in fr]
    e1 = e2 = 0.0
    for f in fr:
        e1 += f.e1
        e2 += f.e2
    n = sum(f.n for f in fr)
    seq = [tm.gmsd.score(e1, e2, n, population), tm.gmsd.mean(e1, n)]
    return (rows, seq, mp) if maps else (rows, seq)


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("beside", [(), ("-m", "psnr"), ("-m", "xpsnr", "-m", "psnr-hvs", "--siti")])
def test_cli_against_the_binding_in_every_output_format(tmp_path, beside, bits):
    pairs = _pairs(bits)
    a, b = _y4m_pairs(tmp_path, pairs, bits)
    rows, seq = _binding(pairs, bits)
    base = (a, b, *beside, "-m", "gmsd")
    first = {0: [], 2: ["psnr"], 5: ["xpsnr_y", "xpsnr_u", "xpsnr_v", "psnr_hvs", "si", "ti"]}[len(beside)]
    plain = {fmt: _cli(a, b, *beside, "--output", fmt) for fmt in FORMATS} if beside else {}
    # json-lines: one line per frame, then the aggregates with the sequence values
    lines = [json.loads(x) for x in _cli(*base, "--output", "json-lines").splitlines() if x.strip()]
    assert len(lines) == CN + 1
    for i in range(CN):
        assert list(lines[i]) == first + NAMES and [lines[i][n] for n in NAMES] == rows[i]
    agg = lines[CN]
    assert agg["frame_count"] == CN and list(agg)[-2:] == NAMES
    for k, n in enumerate(NAMES):
        assert agg[n]["sequence"] == seq[k] and agg[n]["min"] == min(r[k] for r in rows) and agg[n]["max"] == max(r[k] for r in rows)
    # json
    js = json.loads(_cli(*base, "--output", "json"))
    assert list(js)[-2:] == NAMES
    for k, n in enumerate(NAMES):
        assert js[n]["scores"] == [r[k] for r in rows] and js[n]["sequence"] == seq[k] and js[n]["stats"]["max"] == max(r[k] for r in rows)
    # csv: the header, a row per frame as it is computed, then the header and the rows again
    out = _cli(*base, "--output", "csv").splitlines()
    assert out[0] == ",".join(first + NAMES) == out[CN + 1] and len(out) == 2 * CN + 2
    for i in range(CN):
        assert [float(x) for x in out[1 + i].split(",")[-2:]] == rows[i] and out[CN + 2 + i] == out[1 + i]
    # default
    txt = _cli(*base)
    for k in range(2):  # the Stats block's values and the sequence line's, against the binding
        st, sq = _default_values(txt, ("GMSD", "GMSM")[k], ("GMSD", "GMSM")[k])
        assert st["min"] == min(r[k] for r in rows) and st["max"] == max(r[k] for r in rows) and st["p50"] == sorted(r[k] for r in rows)[CN // 2]
        assert st["min"] == agg[NAMES[k]]["min"] and st["mean"] == agg[NAMES[k]]["mean"] and sq == seq[k]
    order = [txt.index(x) for x in ("GMSD: Stats {", "GMSD (sequence): ", "GMSM: Stats {", "GMSM (sequence): ")]
    assert order == sorted(order)
    if beside:  # the other metrics' output is unchanged and comes first
        pl = [json.loads(x) for x in plain["json-lines"].splitlines() if x.strip()]
        for i in range(CN):
            assert [lines[i][n] for n in first] == [pl[i][n] for n in first]
        assert [agg[n] for n in first] == [pl[CN][n] for n in first]
        assert out[1].split(",")[:len(first)] == plain["csv"].splitlines()[1].split(",") and txt.startswith(plain["default"])
        pj = json.loads(plain["json"])
        assert all(js[n] == pj[n] for n in first)


def test_cli_input_formats_population_and_maps(tmp_path):
    """the four input formats (Y4M 8-bit, Y4M 10-bit, raw 8-bit, raw 10-bit), --gmsd-population, --gmsd-map against map()"""
    for bits in (8, 10):
        pairs = _pairs(bits)
        rows, seq, maps = _binding(pairs, bits, maps=True)
        prow, pseq = _binding(pairs, bits, population=True)
        assert pseq[0] < seq[0] and pseq[1] == seq[1]
        d = tmp_path / str(bits)
        d.mkdir()
        for kind in ("y4m", "raw"):
            a, b = (_y4m_pairs if kind == "y4m" else _raw_pairs)(d, pairs, bits)
            extra = [] if kind == "y4m" else ["--width", str(CW), "--height", str(CH), "--bits", str(bits)]
            prefix = str(d / (kind + "_map"))
            lines = [json.loads(x) for x in _cli(a, b, "-m", "gmsd", "--gmsd-map", prefix, "--batch", "2", *extra, "--output", "json-lines").splitlines() if x.strip()]
            assert [[x["gmsd"], x["gmsm"]] for x in lines[:CN]] == rows and [lines[CN][n]["sequence"] for n in NAMES] == seq
            for i in range(CN):
                with open("%s%06d.pfm" % (prefix, i), "rb") as f:
                    assert f.readline() == b"Pf\n" and f.readline().split() == [str((CW + 1) // 2).encode(), str((CH + 1) // 2).encode()]
                    scale = float(f.readline())
                    data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").reshape((CH + 1) // 2, (CW + 1) // 2)
                assert np.array_equal(data[::-1], maps[i]), (kind, bits, i)  # PFM rows run bottom to top
            assert not os.path.exists("%s%06d.pfm" % (prefix, CN))
            lines = [json.loads(x) for x in _cli(a, b, "-m", "gmsd", "--gmsd-population", *extra, "--output", "json-lines").splitlines() if x.strip()]
            assert [[x["gmsd"], x["gmsm"]] for x in lines[:CN]] == prow and [lines[CN][n]["sequence"] for n in NAMES] == pseq


def test_cli_beside_every_other_selection(tmp_path):
    """-m gmsd beside --motion, --scenes, --siti and the other feature libraries: its two columns come last and are the binding's"""
    pairs = _pairs(8)
    a, b = _y4m_pairs(tmp_path, pairs, 8)
    rows, seq = _binding(pairs, 8)
    sel = ("-m", "ssim", "-m", "vif", "-m", "adm", "-m", "cambi", "-m", "psnr-yuv", "-m", "ssim-yuv", "-m", "psnr-hvs-m", "-m", "ciede2000", "--motion", "--scenes", "--siti")
    lines = [json.loads(x) for x in _cli(a, b, *sel, "-m", "gmsd", "--batch", "2", "--output", "json-lines").splitlines() if x.strip()]
    plain = [json.loads(x) for x in _cli(a, b, *sel, "--batch", "2", "--output", "json-lines").splitlines() if x.strip()]
    assert len(lines) == CN + 1 == len(plain)
    for i in range(CN):
        assert list(lines[i]) == list(plain[i]) + NAMES and [lines[i][n] for n in NAMES] == rows[i]
        assert {k: v for k, v in lines[i].items() if k not in NAMES} == plain[i]
    assert [lines[CN][n]["sequence"] for n in NAMES] == seq and list(lines[CN])[-2:] == NAMES


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


def test_cli_refuses_rgb_input(tmp_path):
    pa, pb = _ppm_pair(tmp_path)
    out = subprocess.run([CLI, pa, pb, "-m", "gmsd"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "gmsd needs YUV input" in out.stderr, (out.returncode, out.stderr)


# what the parent commit's binary printed for these arguments on the inputs of _parent_files(dir, kind): recorded once with
# record_parent_cli(<the parent's turbo-metrics>, GOLDEN, <a scratch directory>) on an MI355X, before the CLI was touched
PARENT_CASES = {
    "y4m8_psnr_ssim_default": ("y4m8", ["-m", "psnr", "-m", "ssim"]),
    "y4m8_ssimu_xpsnr_json": ("y4m8", ["-m", "ssimulacra2", "-m", "xpsnr", "--output", "json"]),
    "y4m8_psnr_yuv_motion_jsonl": ("y4m8", ["-m", "psnr", "-m", "psnr-yuv", "-m", "ssim-yuv", "--motion", "--output", "json-lines"]),
    "y4m10_vif_adm_scenes_csv": ("y4m10", ["-m", "vif", "-m", "adm", "--scenes", "--batch", "2", "--output", "csv"]),
    "y4m10_yuv_cambi_csv": ("y4m10", ["-m", "psnr-yuv", "-m", "cambi", "--output", "csv"]),
    "ppm_ssim_flip_jsonl": ("ppm", ["-m", "ssim", "-m", "flip", "--output", "json-lines"]),
    "y4m8_hvs_ciede_siti_default": ("y4m8", ["-m", "psnr-hvs", "-m", "ciede2000", "--siti"]),
}


def _parent_files(d, kind):
    return _ppm_pair(d) if kind == "ppm" else _y4m_pairs(d, _pairs(int(kind[3:])), int(kind[3:]))


def _run_parent_cases(cli, tmp):
    out = {}
    for kind in ("ppm", "y4m8", "y4m10"):
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
        assert not re.search(r"gmsd|gmsm", got[name].lower()), name
