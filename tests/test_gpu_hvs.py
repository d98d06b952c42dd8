"""GPU tier of PSNR-HVS / PSNR-HVS-M: libturbometrics_hvs.so through tm.Hvs against the emulated kernel source
(s_hvs, s_hvsm and blocks bit for bit: the same operations in the same order, all correctly rounded) and against the float64
restatement inside the tolerance measured on the CPU (tests/hvs_util.py); hand values; pitches, garbage, memory kinds, repeats, state
rules; the CLI's two columns against the binding in the four formats; and the CLI without the new values against a recorded run of the
parent commit's binary (tests/golden/hvs_parent_cli.json)."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import hvs_ref as R
from tests import hvs_util as U
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
    """the pairs of plane arrays as slots 0 .. n-1 of one compute -> [(s_hvs, s_hvsm, blocks)]"""
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
    return [(f.s_hvs, f.s_hvsm, f.blocks) for f in v.frames(len(frames))]


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_library_against_emulation_and_restatement(layout, bits):
    for w, h in SIZES:
        pairs = [U.pair(w, h, bits, k, seed=w + h) for k in U.KINDS]
        frames = U.planes_of(layout, pairs, bits)
        emul = U.emulate(w, h, layout, bits, [len(pairs)], frames)
        with tm.Hvs(w, h, layout, bits, batch=len(pairs)) as v:
            got = _compute(v, frames)
        for kind, g, e, (a, b) in zip(U.KINDS, got, emul, pairs):
            assert g == e, (w, h, kind)  # bit for bit
            want = R.sums(a, b)
            assert g[2] == want.blocks
            assert U.rel_err(g[0], want.s_hvs) <= U.REL_TOL and U.rel_err(g[1], want.s_hvsm) <= U.REL_TOL, (w, h, kind)


def test_hand_values():
    for layout, bits in (("y8", 8), ("y16_msb", 10), ("y16_low", 16)):
        peak = (1 << bits) - 1
        flat = [(np.full((17, 24), base, np.int64), np.full((17, 24), base + d, np.int64)) for base, d in ((0, 1), (peak // 2, 3), (peak - 7, 7))]
        a, _ = U.pair(24, 17, bits, "noise", 3)
        with tm.Hvs(24, 17, layout, bits, batch=4) as v:
            v_ = _compute(v, U.planes_of(layout, flat + [(a, a)], bits))
            fr = v.frames(4)
        for (s2, s1, n), d, f in zip(v_, (1, 3, 7), fr):
            want = 20 * math.log10(peak / (1.608443 * d))
            assert n == 6 and s1 == s2 and abs(f.psnr_hvs - want) < 4e-4 and f.psnr_hvs_m == f.psnr_hvs
        assert v_[3] == (0.0, 0.0, 6) and fr[3].psnr_hvs == math.inf and fr[3].psnr_hvs_m == math.inf
    # the masked-away difference and the block of zero variance of tests/test_hvs_cpu.py
    y, x = np.indices((8, 8))
    a = ((x + y) % 2) * 255
    b = a.copy()
    b[1, 1] += 1
    b[6, 3] -= 1
    c = np.full((8, 8), 100, np.int64)
    d = c.copy()
    d[2:5, 3:7] += np.arange(12).reshape(3, 4)
    with tm.Hvs(8, 8, "y8", 8, batch=2) as v:
        (s2, s1, _), (t2, t1, _) = _compute(v, U.planes_of("y8", [(a, b), (c, d)], 8))
    assert s1 == 0.0 and U.rel_err(s2, R.sums(a, b).s_hvs) <= U.REL_TOL
    r = R.sums(c, d)
    assert U.rel_err(t2, r.s_hvs) <= U.REL_TOL and U.rel_err(t1, r.s_hvsm) <= U.REL_TOL and 0 < t1 < t2


def test_pitches_garbage_memory_kinds_and_repeats():
    w, h = SIZES[-1]
    for layout, bits in (("y8", 8), ("y16_msb", 10), ("y16_low", 12), ("y10_packed", 10)):
        pairs = [U.pair(w, h, bits, k, seed=4) for k in ("noise", "quadrant", "near_peak")]
        tight = U.planes_of(layout, pairs, bits)
        loose = U.planes_of(layout, pairs, bits, pad={"y8": 4, "y10_packed": 1}.get(layout, 5))  # pitch above w, garbage between the rows; y8: 129 + 4 bytes, odd like the tight 129
        assert layout != "y8" or (tight[0][0].strides[0] % 2 == 1 and loose[0][0].strides[0] % 2 == 1)
        aligned = U.planes_of(layout, pairs, bits, pad=2, aligned=True)
        # garbage in the remainder columns and rows
        dirty = []
        for a, b in pairs:
            a2, b2 = a.copy(), b.copy()
            a2[:, 8 * (w // 8):] = 0
            b2[8 * (h // 8):, :] = (1 << bits) - 1
            dirty.append((a2, b2))
        with tm.Hvs(w, h, layout, bits, batch=3) as v:
            first = _compute(v, tight)
            assert _compute(v, tight) == first  # a repeated compute: equal bits
            for frames in (tight, loose, aligned, U.planes_of(layout, dirty, bits)):
                for mem in ("host", "pinned", "device"):
                    assert _compute(v, frames, mem) == first, (layout, mem)
            assert _compute(v, tight[1:2]) == first[1:2]  # a smaller compute on the same buffers
        assert first == U.emulate(w, h, layout, bits, [3], tight)


def test_state_rules():
    w, h = 32, 32
    (pr, pd), = U.planes_of("y8", [U.pair(w, h, 8, "noise", 1)], 8)
    with tm.Hvs(w, h, "y8", 8, batch=2) as v:
        assert v.mem_usage() > 0
        v.set_pair(0, pr, pd)
        with pytest.raises(tm.hvs.HvsError) as e:
            v.compute(2)  # slot 1 was not set
        assert e.value.code == tm.ffi.TM_ERR_STATE
        v.compute(1)
        with pytest.raises(tm.hvs.HvsError) as e:
            v.compute(1)  # every compute consumes its pairs
        assert e.value.code == tm.ffi.TM_ERR_STATE
        with pytest.raises(tm.hvs.HvsError) as e:
            v.frames(2)  # not slots of the last compute
        assert e.value.code == tm.ffi.TM_ERR_STATE
        assert v.frames(1)[0].blocks == 16


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
GOLDEN = os.path.join(ROOT, "tests", "golden", "hvs_parent_cli.json")
CW, CH, CN = 98, 42, 3  # 2 columns and 2 rows beyond the last block
NAMES = ["psnr_hvs", "psnr_hvs_m"]
FORMATS = ("json-lines", "json", "csv", "default")


def _cli(*args, cli=CLI):
    out = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def _pairs(bits):
    return [U.pair(CW, CH, bits, "quadrant", seed=30 + i) for i in range(CN)]


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


def _default_values(txt, block, line):
    """the default format: ({name: value} of the `block: Stats { ... }` lines, the value on the `line (sequence): ` line)"""
    m = re.search(r"^%s: Stats \{\n(.*?)\n\}$" % re.escape(block), txt, re.S | re.M)
    q = re.search(r"^%s \(sequence\): (\S+)$" % re.escape(line), txt, re.M)
    assert m and q, (block, line)
    stats = {k: float(v) for k, v in re.findall(r"^\s+(\w+): ([^,\n]+),$", m.group(1), re.M)}
    assert {"min", "max", "mean", "p50"} <= set(stats)
    return stats, float(q.group(1))


def _binding(pairs, bits):
    """per frame the two values and the two sequence values from tm.Hvs and the library's host function"""
    layout = "y8" if bits == 8 else "y16_low"
    with tm.Hvs(CW, CH, layout, bits, batch=len(pairs)) as v:
        _compute(v, U.planes_of(layout, pairs, bits))
        fr = v.frames(len(pairs))
    rows = [[f.psnr_hvs, f.psnr_hvs_m] for f in fr]
    s2 = s1 = 0.0
    for f in fr:
        s2 += f.s_hvs
        s1 += f.s_hvsm
    n = sum(f.blocks for f in fr)
    return rows, [tm.hvs.psnr(s2, n, bits), tm.hvs.psnr(s1, n, bits)]


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("sel,beside", [("hvs", ()), ("hvsm", ()), ("both", ()), ("both", ("-m", "psnr")), ("both", ("-m", "xpsnr", "-m", "psnr-yuv"))])
def test_cli_against_the_binding_in_every_output_format(tmp_path, sel, beside, bits):
    pairs = _pairs(bits)
    a, b = _y4m_pairs(tmp_path, pairs, bits)
    rows, seq = _binding(pairs, bits)
    cols = {"hvs": [0], "hvsm": [1], "both": [0, 1]}[sel]
    names = [NAMES[k] for k in cols]
    flags = {"hvs": ("-m", "psnr-hvs"), "hvsm": ("-mpsnr-hvs-m",), "both": ("-m", "psnr-hvs-m", "--metrics", "psnr-hvs")}[sel]
    base = (a, b, *beside, *flags)
    first = {(): [], ("-m", "psnr"): ["psnr"], ("-m", "xpsnr", "-m", "psnr-yuv"): ["xpsnr_y", "xpsnr_u", "xpsnr_v", "psnr_y", "psnr_u", "psnr_v", "psnr_avg"]}[beside]
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
    assert ("PSNR_HVS: Stats {" in txt) == (sel != "hvsm") and ("PSNR_HVS_M: Stats {" in txt) == (sel != "hvs")
    assert ("PSNR-HVS (sequence): " in txt) == (sel != "hvsm") and ("PSNR-HVS-M (sequence): " in txt) == (sel != "hvs")
    for k in cols:  # the Stats block's values and the sequence line's, against the binding
        st, sq = _default_values(txt, ("PSNR_HVS", "PSNR_HVS_M")[k], ("PSNR-HVS", "PSNR-HVS-M")[k])
        assert st["min"] == min(r[k] for r in rows) and st["max"] == max(r[k] for r in rows) and st["p50"] == sorted(r[k] for r in rows)[CN // 2]
        assert st["min"] == agg[NAMES[k]]["min"] and st["mean"] == agg[NAMES[k]]["mean"] and sq == seq[k]
    if sel == "both":  # psnr_hvs first, each block followed by its own sequence line
        order = [txt.index(x) for x in ("PSNR_HVS: Stats {", "PSNR-HVS (sequence): ", "PSNR_HVS_M: Stats {", "PSNR-HVS-M (sequence): ")]
        assert order == sorted(order)
    if beside:  # the other metrics' output is unchanged and comes first
        pl = [json.loads(x) for x in plain["json-lines"].splitlines() if x.strip()]
        for i in range(CN):
            assert [lines[i][n] for n in first] == [pl[i][n] for n in first]
        assert [agg[n] for n in first] == [pl[CN][n] for n in first]
        assert out[1].split(",")[:len(first)] == plain["csv"].splitlines()[1].split(",") and txt.startswith(plain["default"])
        pj = json.loads(plain["json"])
        assert all(js[n] == pj[n] for n in first)


def test_cli_prints_infinity_the_way_psnr_y_does(tmp_path):
    pairs = _pairs(8)
    same = [(r, r) for r, _ in pairs[:1]] + pairs[1:2]
    a, b = _y4m_pairs(tmp_path, same, 8)
    rows = _cli(a, b, "-m", "psnr-yuv", "-m", "psnr-hvs", "-m", "psnr-hvs-m", "--output", "csv").splitlines()
    cells = rows[1].split(",")
    assert cells[4:6] == [cells[0]] * 2 and "inf" in cells[0].lower()
    raw = _cli(a, b, "-m", "psnr-yuv", "-m", "psnr-hvs", "--output", "json-lines").splitlines()[0]
    assert raw.split('"psnr_hvs":')[1].rstrip("}").split(",")[0] == raw.split('"psnr_y":')[1].split(",")[0]


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
    for sel in ("psnr-hvs", "psnr-hvs-m"):
        out = subprocess.run([CLI, pa, pb, "-m", sel], capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "psnr-hvs / psnr-hvs-m need YUV input" in out.stderr, (out.returncode, out.stderr)


# what the parent commit's binary printed for these arguments on the inputs of _parent_files(dir, kind): recorded once with
# record_parent_cli(<the parent's turbo-metrics>, GOLDEN, <a scratch directory>) on an MI355X
PARENT_CASES = {
    "y4m8_psnr_ssim_default": ("y4m8", ["-m", "psnr", "-m", "ssim"]),
    "y4m8_ssimu_xpsnr_json": ("y4m8", ["-m", "ssimulacra2", "-m", "xpsnr", "--output", "json"]),
    "y4m8_psnr_yuv_motion_jsonl": ("y4m8", ["-m", "psnr", "-m", "psnr-yuv", "-m", "ssim-yuv", "--motion", "--output", "json-lines"]),
    "y4m10_vif_adm_scenes_csv": ("y4m10", ["-m", "vif", "-m", "adm", "--scenes", "--batch", "2", "--output", "csv"]),
    "y4m10_yuv_cambi_csv": ("y4m10", ["-m", "psnr-yuv", "-m", "cambi", "--output", "csv"]),
    "ppm_ssim_flip_jsonl": ("ppm", ["-m", "ssim", "-m", "flip", "--output", "json-lines"]),
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
        assert not re.search(r"hvs", got[name].lower()), name
