"""MDSI on the MI355X: libturbometrics_mdsi.so through tm.Mdsi against the emulated kernel source with `==`
(sums, counts and every map value), against the float64 restatement inside the CPU-measured tolerance, the hand values, pitches,
memory kinds, repeats, mixed batches and the map's state rules, the CLI's column against the binding, and the CLI without -m mdsi
against a recorded run of the parent commit's binary (tests/golden/mdsi_parent_cli.json).  The same small shapes as
tests/test_mdsi_cpu.py."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mdsi_ref as R
from tests import mdsi_util as U
from tm_pkg import tm

pytestmark = pytest.mark.gpu

_WANT = {}


def want_of(w, h, bits, kind, f, seed=0):
    key = (w, h, bits, kind, f, seed)
    if key not in _WANT:
        pr = U.pair(w, h, bits, kind, seed=seed, scale=f or R.factor(w, h))
        _WANT[key] = (pr, R.mdsi(pr[0], pr[1], bits, "bt709", f))
    return _WANT[key]


def same(fr, mp, got):
    """a library frame and map against the emulation's Got, bit for bit"""
    return (fr.sum_re == got.sum_re and fr.sum_im == got.sum_im and fr.dev == got.dev and fr.n == got.n and fr.negatives == got.negatives
            and mp.shape == got.map.shape and (mp.view(np.uint32) == got.map.view(np.uint32)).all())


def run(w, h, layout, bits, frames, f=0, matrix="bt709", maps=True):
    with tm.Mdsi(w, h, layout, bits, matrix=matrix, factor=f, batch=len(frames), maps=maps) as t:
        for i, (a, b) in enumerate(frames):
            t.set_pair(i, a, b)
        t.compute(len(frames))
        return t.frames(len(frames)), [t.map(i) for i in range(len(frames))] if maps else None


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_library_equals_emulation_and_meets_the_restatement(layout, bits):
    ci = U.CASES.index((layout, bits))
    for fi, f in enumerate(U.FACTORS):
        shapes = U.shapes(f)
        for si in ((ci + fi) % len(shapes), (ci + fi + 3) % len(shapes)):
            w, h = shapes[si]
            kinds = [U.KINDS[(ci + si + k) % len(U.KINDS)] for k in (0, 2, 5)]
            prs = [want_of(w, h, bits, kind, f) for kind in kinds]
            for aligned in (True, False):
                fr = U.frames_of(layout, [p for p, _ in prs], w, h, bits, pad=3 if not aligned else 0, aligned=aligned)
                frames, maps = run(w, h, layout, bits, fr, f)
                for i, (pr, want) in enumerate(prs):
                    got = U.emulate(w, h, layout, bits, [1], [fr[i]], factor=f)[0]
                    assert same(frames[i], maps[i], got), (f, w, h, kinds[i], aligned)
                    assert frames[i].factor == f and frames[i].n == want.n and frames[i].negatives == want.negatives
                    assert abs(frames[i].mad - want.mad) <= U.MAD_TOL, (f, w, h, kinds[i], frames[i].mad, want.mad)
                    if want.mdsi >= U.MDSI_FLOOR:
                        assert abs(frames[i].mdsi - want.mdsi) <= U.MDSI_TOL, (f, w, h, kinds[i], frames[i].mdsi, want.mdsi)


@pytest.mark.parametrize("layout,bits", [("nv12", 8), ("p016", 10), ("i420", 16)])
def test_identical_pictures_give_exactly_zero(layout, bits):
    for f, (w, h) in ((1, (37, 21)), (3, (50, 35)), (4, (67, 41))):
        pr, _ = want_of(w, h, bits, "identical", f)
        frames, maps = run(w, h, layout, bits, U.frames_of(layout, [pr], w, h, bits), f)
        assert frames[0].mdsi == 0.0 and frames[0].dev == 0.0 and frames[0].sum_im == 0.0 and frames[0].sum_re == frames[0].n and (maps[0] == 1.0).all()


def test_flat_against_flat_at_5_x_5_is_the_hand_value():
    """the value derived in tests/test_mdsi_cpu.py::test_flat_against_flat_at_5_x_5_by_hand, through the restatement that test pins"""
    pr = U.pair(5, 5, 8, "flat_flat")
    want = R.mdsi(pr[0], pr[1], 8, "bt709", 2)
    frames, maps = run(5, 5, "nv12", 8, U.frames_of("nv12", [pr], 5, 5, 8), 2)
    assert abs(frames[0].mad - want.mad) <= U.MAD_TOL and abs(frames[0].mdsi - want.mdsi) <= U.MDSI_TOL and np.abs(maps[0] - want.gcs).max() < 1e-6


def test_automatic_factor_on_a_real_picture():
    pr, want = want_of(640, 641, 8, "chroma_only", 0)
    frames, maps = run(640, 641, "nv12", 8, U.frames_of("nv12", [pr], 640, 641, 8), 0)
    assert frames[0].factor == 3 and maps[0].shape == (214, 214)
    assert abs(frames[0].mad - want.mad) <= U.MAD_TOL and abs(frames[0].mdsi - want.mdsi) <= U.MDSI_TOL


def test_pitches_with_garbage_beside_the_rows():
    w, h, f = 25, 19, 2
    for layout, bits in (("nv12", 8), ("p016", 12), ("i420", 10), ("i420p10", 10)):
        pr, _ = want_of(w, h, bits, "noise", f)
        base = None
        for pad, aligned in ((0, False), (0, True), (7, True), (5, False)):
            frames, maps = run(w, h, layout, bits, U.frames_of(layout, [pr], w, h, bits, pad=pad, aligned=aligned), f)
            cur = (frames[0], maps[0].tobytes())
            base = base or cur
            assert cur == base, (layout, pad, aligned)


def test_memory_kinds_repeats_and_a_mixed_batch():
    import torch
    w, h, f = 70, 37, 2
    kinds = ("noise", "identical", "negative", "chroma_only", "flat_flat")
    prs = [want_of(w, h, 8, kind, f)[0] for kind in kinds]
    fr = U.frames_of("nv12", prs, w, h, 8, aligned=True)
    single = [run(w, h, "nv12", 8, [x], f) for x in fr]
    with tm.Mdsi(w, h, "nv12", 8, factor=f, batch=len(fr), maps=True) as t:
        results = []
        for conv in (lambda p: np.ascontiguousarray(p), lambda p: torch.from_numpy(np.ascontiguousarray(p)).pin_memory(),
                     lambda p: torch.from_numpy(np.ascontiguousarray(p)).cuda(), lambda p: torch.from_numpy(np.ascontiguousarray(p)).cuda()):
            keep = [([conv(p) for p in a], [conv(p) for p in b]) for a, b in fr]
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(keep):
                t.set_pair(i, a, b)
            t.compute(len(fr))
            results.append((t.frames(len(fr)), [t.map(i).tobytes() for i in range(len(fr))]))
        for r in results[1:]:
            assert r == results[0]  # the three memory kinds, and the same input twice: the same bytes
        for i, (frames, maps) in enumerate(single):
            assert results[0][0][i] == frames[0] and results[0][1][i] == maps[0].tobytes(), kinds[i]
        assert results[0][0][1].mdsi == 0.0 and results[0][0][2].negatives > 0
        # state rules: a slot is consumed by its compute; a map only of a slot the last compute covered
        with pytest.raises(tm.mdsi.MdsiError) as e:
            t.compute(1)
        assert e.value.code == tm.ffi.TM_ERR_STATE
        t.set_pair(0, *fr[0])
        t.compute(1)
        assert t.map(0).tobytes() == single[0][1][0].tobytes()
        with pytest.raises(tm.mdsi.MdsiError) as e:
            t.map(1)
        assert e.value.code == tm.ffi.TM_ERR_STATE
    with tm.Mdsi(w, h, "nv12", 8, factor=f, batch=1, maps=False) as t:
        t.set_pair(0, *fr[0])
        t.compute(1)
        assert t.frames(1)[0] == single[0][0][0]
        with pytest.raises(tm.mdsi.MdsiError) as e:
            t.map(0)
        assert e.value.code == tm.ffi.TM_ERR_STATE


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mdsi_parent_cli.json")
CW, CH, CN = 99, 43, 3  # odd both ways: the zero column and row enter the sums at factor 2
FORMATS = ("json-lines", "json", "csv", "default")
BT709 = ("--color-primaries", "1", "--matrix-coefficients", "1")


def _cli(*args, cli=CLI):
    out = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def _pairs(bits):
    return [U.pair(CW, CH, bits, kind, seed=30 + i, scale=2) for i, kind in enumerate(("chroma_only", "negative", "shifted_edges"))]


def _files(d, pairs, bits, header):
    """two planar 4:2:0 files: Y4M with a header, headerless otherwise"""
    dt = np.uint8 if bits == 8 else "<u2"
    out = []
    for side, name in enumerate(("a", "b")):
        p = os.path.join(str(d), name + (".y4m" if header else ".yuv"))
        with open(p, "wb") as f:
            if header:
                f.write(f"YUV4MPEG2 W{CW} H{CH} F25:1 Ip A1:1 C420{'jpeg' if bits == 8 else 'p%d' % bits}\n".encode())
            for pr in pairs:
                f.write((b"FRAME\n" if header else b"") + b"".join(np.asarray(pl, dt).tobytes() for pl in pr[side]))
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


def _binding(pairs, bits, factor=0, matrix="bt601"):
    """per frame the value, the sequence value (the mean of the pairs' values, added in stream order) and the maps from tm.Mdsi"""
    frames, maps = run(CW, CH, "i420", bits, U.frames_of("i420", pairs, CW, CH, bits), factor, matrix)
    col = [f.mdsi for f in frames]
    s = 0.0
    for v in col:
        s += v
    return col, s / len(col), maps


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("beside", [(), ("-m", "psnr"), ("-m", "ciede2000", "-m", "gmsd", "-m", "deitp")])
def test_cli_against_the_binding_in_every_output_format(tmp_path, beside, bits):
    pairs = _pairs(bits)
    a, b = _files(tmp_path, pairs, bits, True)
    col, seq, _ = _binding(pairs, bits)
    assert min(col) > 0.05
    base = (a, b, *beside, "-m", "mdsi")
    first = {0: [], 2: ["psnr"], 6: ["ciede2000", "ciede2000_de", "gmsd", "gmsm", "deitp", "deitp_max"]}[len(beside)]
    plain = {fmt: _cli(a, b, *beside, "--output", fmt) for fmt in FORMATS} if beside else {}
    # json-lines: one line per frame, then the aggregates with the sequence value
    lines = [json.loads(x) for x in _cli(*base, "--output", "json-lines").splitlines() if x.strip()]
    assert len(lines) == CN + 1
    for i in range(CN):
        assert list(lines[i]) == first + ["mdsi"] and lines[i]["mdsi"] == col[i]
    agg = lines[CN]
    assert agg["frame_count"] == CN and list(agg)[-1] == "mdsi"
    assert agg["mdsi"]["sequence"] == seq and agg["mdsi"]["min"] == min(col) and agg["mdsi"]["max"] == max(col)
    # json
    js = json.loads(_cli(*base, "--output", "json"))
    assert list(js)[-1] == "mdsi" and js["mdsi"]["scores"] == col and js["mdsi"]["sequence"] == seq
    # csv: the header, a row per frame as it is computed, then the header and the rows again
    out = _cli(*base, "--output", "csv").splitlines()
    assert out[0] == ",".join(first + ["mdsi"]) == out[CN + 1] and len(out) == 2 * CN + 2
    for i in range(CN):
        assert float(out[1 + i].split(",")[-1]) == col[i] and out[CN + 2 + i] == out[1 + i]
    # default
    txt = _cli(*base)
    st, sq = _default_values(txt, "MDSI", "MDSI")
    assert st["min"] == min(col) and st["max"] == max(col) and st["p50"] == sorted(col)[CN // 2] and sq == seq
    assert txt.rstrip("\n").endswith("MDSI (sequence): " + txt.rstrip("\n").rsplit(": ", 1)[1])  # after every other block
    if beside:  # the other metrics' output is unchanged and comes first
        pl = [json.loads(x) for x in plain["json-lines"].splitlines() if x.strip()]
        for i in range(CN):
            assert [lines[i][n] for n in first] == [pl[i][n] for n in first]
        assert [agg[n] for n in first] == [pl[CN][n] for n in first]
        assert out[1].split(",")[:len(first)] == plain["csv"].splitlines()[1].split(",") and txt.startswith(plain["default"])
        pj = json.loads(plain["json"])
        assert all(js[n] == pj[n] for n in first)


def test_cli_input_formats_factor_matrix_and_maps(tmp_path):
    """the four input formats (Y4M 8-bit, Y4M 10-bit, raw 8-bit, raw 10-bit), --mdsi-factor, --mdsi-map against map(), the matrix"""
    for bits in (8, 10):
        pairs = _pairs(bits)
        factor = 2 if bits == 8 else 3
        col, seq, maps = _binding(pairs, bits, factor)
        wd, hd = -(-CW // factor), -(-CH // factor)
        d = tmp_path / str(bits)
        d.mkdir()
        for header in (True, False):
            a, b = _files(d, pairs, bits, header)
            extra = [] if header else ["--width", str(CW), "--height", str(CH), "--bits", str(bits)]
            prefix = str(d / ("y4m_map" if header else "raw_map"))
            lines = [json.loads(x) for x in _cli(a, b, "-m", "mdsi", "--mdsi-factor", str(factor), "--mdsi-map", prefix, "--batch", "2", *extra,
                                                 "--output", "json-lines").splitlines() if x.strip()]
            assert [x["mdsi"] for x in lines[:CN]] == col and lines[CN]["mdsi"]["sequence"] == seq
            for i in range(CN):
                with open("%s%06d.pfm" % (prefix, i), "rb") as f:
                    assert f.readline() == b"Pf\n" and f.readline().split() == [str(wd).encode(), str(hd).encode()]
                    scale = float(f.readline())
                    data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").reshape(hd, wd)
                assert np.array_equal(data[::-1], maps[i]), (header, bits, i)  # PFM rows run bottom to top
            assert not os.path.exists("%s%06d.pfm" % (prefix, CN))
    # the default factor is the automatic one (1 at 43 rows); the matrix follows --matrix-coefficients as for ciede2000
    pairs = _pairs(8)
    a, b = _files(tmp_path, pairs, 8, True)
    column = lambda *args: [float(x.split(",")[-1]) for x in _cli(a, b, "-m", "mdsi", *args, "--output", "csv").splitlines()[1:CN + 1]]
    c601, c709 = _binding(pairs, 8, 0, "bt601")[0], _binding(pairs, 8, 0, "bt709")[0]
    assert c601 != c709
    assert column() == c601 == column("--mdsi-factor", "1") == column("--matrix-coefficients", "6")  # by height: 43 rows are BT.601
    assert column(*BT709) == c709
    assert column("--mdsi-factor", "2") == _binding(pairs, 8, 2)[0] != c601


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


def test_cli_refusals(tmp_path):
    pa, pb = _ppm_pair(tmp_path)
    out = subprocess.run([CLI, pa, pb, "-m", "mdsi"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "mdsi needs 4:2:0 YUV input" in out.stderr, (out.returncode, out.stderr)
    a, b = _files(tmp_path, _pairs(8), 8, True)
    for args, what in ((("-m", "psnr", "--mdsi-factor", "2"), "belong to '-m mdsi'"), (("-m", "mdsi", "--mdsi-factor", "0"), "--mdsi-factor"),
                       (("-m", "mdsi", "--mdsi-factor", "129"), "--mdsi-factor"), (("-m", "mdsi", "--mdsi-factor", "64"), "at least four positions")):
        out = subprocess.run([CLI, a, b, *args], capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and what in out.stderr, (args, out.returncode, out.stderr)


# what the parent commit's binary printed for these arguments on the inputs of _parent_files(dir, kind): recorded once with
# record_parent_cli(<the parent's turbo-metrics>, GOLDEN, <a scratch directory>) on an MI355X, before the CLI was touched.  The option
# mixes of tests/golden/gmsd_parent_cli.json, and one with the parent's newest columns
PARENT_CASES = {
    "y4m8_psnr_ssim_default": ("y4m8", ["-m", "psnr", "-m", "ssim"]),
    "y4m8_ssimu_xpsnr_json": ("y4m8", ["-m", "ssimulacra2", "-m", "xpsnr", "--output", "json"]),
    "y4m8_psnr_yuv_motion_jsonl": ("y4m8", ["-m", "psnr", "-m", "psnr-yuv", "-m", "ssim-yuv", "--motion", "--output", "json-lines"]),
    "y4m10_vif_adm_scenes_csv": ("y4m10", ["-m", "vif", "-m", "adm", "--scenes", "--batch", "2", "--output", "csv"]),
    "y4m10_yuv_cambi_csv": ("y4m10", ["-m", "psnr-yuv", "-m", "cambi", "--output", "csv"]),
    "ppm_ssim_flip_jsonl": ("ppm", ["-m", "ssim", "-m", "flip", "--output", "json-lines"]),
    "y4m8_hvs_ciede_siti_default": ("y4m8", ["-m", "psnr-hvs", "-m", "ciede2000", "--siti"]),
    "y4m10_gmsd_haarpsi_deitp_default": ("y4m10", ["-m", "gmsd", "-m", "haarpsi", "-m", "deitp"]),
    "y4m10_ciede_deitp_csv": ("y4m10", ["-m", "ciede2000", "-m", "deitp", "--itp-transfer", "hlg", "--output", "csv"]),
}


def _parent_files(d, kind):
    return _ppm_pair(d) if kind == "ppm" else _files(d, _pairs(int(kind[3:])), int(kind[3:]), True)


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


def test_cli_without_the_new_value_is_byte_identical_with_the_parents(tmp_path):
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(PARENT_CASES)
    got = _run_parent_cases(CLI, tmp_path)
    for name in PARENT_CASES:
        assert got[name] == want[name], name
        assert "mdsi" not in got[name].lower(), name
