"""GPU tier of CIEDE2000: libturbometrics_ciede.so through tm.Ciede against the float64 restatement
(tests/ciede_ref.py) under the per-position and mean rule of tests/ciede_util.py, maps included (the device's powf, cbrtf, atan2f,
expf, sinf and cosf are not the host libm's, so the emulation is not the yardstick here); determinism across repeats, slot positions,
batch sizes and memory kinds; identical pictures; state rules; the CLI's two columns against the binding in the four formats; and the
CLI without the new value against a recorded run of the parent commit's binary (tests/golden/ciede_parent_cli.json)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ciede_ref as R
from tests import ciede_util as U
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


def _compute(c, frames, mem="host", maps=False):
    """the pairs of plane-array lists as slots 0 .. n-1 of one compute -> [(de_sum, de_max, map or None)]"""
    import torch
    keep = []
    for s, sides in enumerate(frames):
        for side, planes in enumerate(sides):
            if mem == "device":
                planes = [_torch(np.ascontiguousarray(p)).cuda() for p in planes]
                torch.cuda.synchronize()
            elif mem == "pinned":
                planes = [_torch(np.ascontiguousarray(p)).pin_memory() for p in planes]
            keep.append(planes)
            c.set_frame(s, side, planes)
    c.compute(len(frames))
    fr = c.frames(len(frames))
    for f in fr:
        assert f.pixels == c.w * c.h and f.de_mean == f.de_sum / f.pixels and f.score == tm.ciede.score(f.de_sum, f.pixels)
    return [(f.de_sum, f.de_max, c.map(i) if maps else None) for i, f in enumerate(fr)]


def _same(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and x[1] == y[1] and (x[2] is None or y[2] is None or np.array_equal(x[2].view(np.uint32), y[2].view(np.uint32)))
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_library_against_restatement(layout, bits):
    """prints the largest figures of this layout and depth: tests/ciede_util.py records the largest over all of them"""
    worst_a = worst_r = worst_m = 0.0
    wrong = []
    for w, h in SIZES:
        pairs = [U.pair(w, h, bits, k) for k in U.KINDS]
        frames = U.frames_of(layout, pairs, w, h, bits)
        with tm.Ciede(w, h, layout, bits, batch=len(pairs), maps=True) as c:
            got = _compute(c, frames, maps=True)
        with tm.Ciede(w, h, layout, bits, batch=len(pairs)) as c:
            assert _same(_compute(c, frames), got)  # without the maps: the same sums
            with pytest.raises(tm.ciede.CiedeError) as e:
                c.map(0)
            assert e.value.code == tm.ffi.TM_ERR_STATE
        for kind, (a, b), (s, mx, m) in zip(U.KINDS, pairs, got):
            want = R.picture(a, b, bits)
            ea, er = U.errors(m, want)
            mr = U.mean_rel_map(s, m, want)
            worst_a, worst_r, worst_m = max(worst_a, ea), max(worst_r, er), max(worst_m, mr)
            assert mx == float(m.max()) and abs(s - float(m.astype(np.float64).sum())) <= 1e-6 * max(s, 1.0)
            bad = U.agrees(m, want, U.ATOL_GPU, U.RTOL_GPU)
            if bad is not None or mr > U.MEAN_REL_TOL_GPU:
                wrong.append((w, h, kind, bad, mr))
    print(f"measured on the GPU, {layout} {bits}: atol {worst_a:.3e} (want < 1), rtol {worst_r:.3e} (want >= 1), de_mean rel {worst_m:.3e}")
    assert not wrong, wrong[:3]
    assert worst_a <= U.ATOL_GPU / 4 and worst_r <= U.RTOL_GPU / 4 and worst_m <= U.MEAN_REL_TOL_GPU / 4  # the recorded figures hold


@pytest.mark.parametrize("matrix,k", (("bt601", (1.0, 1.0, 1.0)), ("libvmaf", tm.ciede.K_LIBVMAF)))
def test_matrix_and_factors(matrix, k):
    w, h = SIZES[3]
    for layout, bits in (("nv12", 8), ("i420p10", 10)):
        pairs = [U.pair(w, h, bits, kind, 2) for kind in ("noise", "primaries", "hue_sweep")]
        with tm.Ciede(w, h, layout, bits, matrix=matrix, k=k, batch=3, maps=True) as c:
            got = _compute(c, U.frames_of(layout, pairs, w, h, bits), maps=True)
        for (a, b), (s, mx, m) in zip(pairs, got):
            assert U.agrees(m, R.picture(a, b, bits, matrix, k), U.ATOL_GPU, U.RTOL_GPU) is None
            assert U.agrees(m, R.picture(a, b, bits), U.ATOL_GPU, U.RTOL_GPU) is not None


def test_identical_pictures_give_exactly_zero_and_100():
    for layout, bits in U.CASES:
        w, h = SIZES[-1]
        a, _ = U.pair(w, h, bits, "noise", 3)
        b, _ = U.pair(w, h, bits, "hue_sweep", 3)
        frames = U.frames_of(layout, [(a, a), (b, b)], w, h, bits)  # the two sides differ in the bits the kernel must ignore
        with tm.Ciede(w, h, layout, bits, batch=2, maps=True) as c:
            for s, mx, m in _compute(c, frames, maps=True):
                assert s == 0.0 and mx == 0.0 and not m.any()
            assert [f.score for f in c.frames(2)] == [100.0, 100.0]


def test_determinism_pitches_garbage_and_memory_kinds():
    w, h = SIZES[-1]
    for layout, bits in (("nv12", 8), ("p016", 10), ("i420", 12), ("i420p10", 10)):
        pairs = [U.pair(w, h, bits, k, seed=4) for k in ("noise", "hue_sweep", "near_black")]
        tight = U.frames_of(layout, pairs, w, h, bits)
        loose = U.frames_of(layout, pairs, w, h, bits, pad={"i420p10": 1}.get(layout, 5))  # pitch above the row, garbage between the rows
        clean = U.frames_of(layout, pairs, w, h, bits, dirty=False)
        aligned = U.frames_of(layout, pairs, w, h, bits, pad=2, aligned=True)
        with tm.Ciede(w, h, layout, bits, batch=3, maps=True) as c:
            first = _compute(c, tight, maps=True)
            assert _same(_compute(c, tight, maps=True), first)  # a repeated compute: equal bits
            for frames in (tight, loose, clean, aligned):
                for mem in ("host", "pinned", "device"):
                    assert _same(_compute(c, frames, mem, maps=True), first), (layout, mem)
            assert _same(_compute(c, tight[1:2], maps=True), first[1:2])  # a smaller compute on the same buffers
            assert _same(_compute(c, [tight[2], tight[0]], maps=True), [first[2], first[0]])  # other slot positions
        with tm.Ciede(w, h, layout, bits, batch=7) as c:  # another batch capacity
            assert _same(_compute(c, tight + tight[:1]), first + first[:1])


def test_state_rules():
    w, h = 34, 18
    (ref, dis), = U.frames_of("i420", [U.pair(w, h, 8, "noise", 1)], w, h, 8)
    with tm.Ciede(w, h, "i420", 8, batch=2, maps=True) as c:
        assert c.mem_usage() > 0
        c.set_pair(0, ref, dis)
        c.set_frame(1, 0, ref)
        with pytest.raises(tm.ciede.CiedeError) as e:
            c.compute(2)  # slot 1 has one side only
        assert e.value.code == tm.ffi.TM_ERR_STATE
        with pytest.raises(tm.ciede.CiedeError) as e:
            c.frames(1)  # nothing was computed
        assert e.value.code == tm.ffi.TM_ERR_STATE
        c.compute(1)
        with pytest.raises(tm.ciede.CiedeError) as e:
            c.compute(1)  # every compute consumes its pictures
        assert e.value.code == tm.ffi.TM_ERR_STATE
        for bad in (lambda: c.frames(2), lambda: c.map(1)):  # not slots of the last compute
            with pytest.raises(tm.ciede.CiedeError) as e:
                bad()
            assert e.value.code == tm.ffi.TM_ERR_STATE
        assert c.frames(1)[0].pixels == w * h and c.map(0).shape == (h, w)
        with pytest.raises(tm.ciede.CiedeError) as e:
            c.set_frame(2, 0, ref)
        assert e.value.code == tm.ffi.TM_ERR_INVALID_ARG


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ciede_parent_cli.json")
CW, CH, CN = 99, 43, 3  # odd in both directions; by height the CLI's colour dispatch takes BT.601 (H.273 code 6)
NAMES = ["ciede2000", "ciede2000_de"]
FORMATS = ("json-lines", "json", "csv", "default")
BT709 = ("--color-primaries", "1", "--matrix-coefficients", "1")


def _cli(*args, cli=CLI):
    out = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def _pairs(bits):
    return [U.pair(CW, CH, bits, kind, seed=30 + i) for i, kind in enumerate(("quadrant", "hue_sweep", "near_peak"))][:CN]


def _y4m_pairs(d, pairs, bits):
    dt = np.uint8 if bits == 8 else "<u2"
    out = []
    for side, name in enumerate(("a.y4m", "b.y4m")):
        p = os.path.join(str(d), name)
        with open(p, "wb") as f:
            f.write(f"YUV4MPEG2 W{CW} H{CH} F25:1 Ip A1:1 C420{'jpeg' if bits == 8 else 'p%d' % bits}\n".encode())
            for pr in pairs:
                f.write(b"FRAME\n" + b"".join(np.asarray(pl, dt).tobytes() for pl in pr[side]))
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


def _binding(pairs, bits, matrix="bt601", k=(1.0, 1.0, 1.0)):
    """per frame the two values, the two sequence values and the maps from tm.Ciede and the library's host function"""
    with tm.Ciede(CW, CH, "i420", bits, matrix=matrix, k=k, batch=len(pairs), maps=True) as c:
        got = _compute(c, U.frames_of("i420", pairs, CW, CH, bits), maps=True)
        fr = c.frames(len(pairs))
    rows = [[f.score, f.de_mean] for f in fr]
    s, n = sum(f.de_sum for f in fr), sum(f.pixels for f in fr)
    return rows, [tm.ciede.score(s, n), s / n], [g[2] for g in got]


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("beside", [(), ("-m", "psnr"), ("-m", "psnr-yuv", "-m", "xpsnr")])
def test_cli_against_the_binding_in_every_output_format(tmp_path, beside, bits):
    pairs = _pairs(bits)
    a, b = _y4m_pairs(tmp_path, pairs, bits)
    rows, seq, _ = _binding(pairs, bits)
    base = (a, b, *beside, "-m", "ciede2000")
    first = {(): [], ("-m", "psnr"): ["psnr"], ("-m", "psnr-yuv", "-m", "xpsnr"): ["xpsnr_y", "xpsnr_u", "xpsnr_v", "psnr_y", "psnr_u", "psnr_v", "psnr_avg"]}[beside]
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
    assert all(np.isfinite(r).all() for r in rows) and all(r[0] <= 100.0 for r in rows)
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
    order = [txt.index(x) for x in ("CIEDE2000: Stats {", "CIEDE2000 (sequence): ", "CIEDE2000_DE: Stats {", "CIEDE2000 mean dE00 (sequence): ")]
    assert order == sorted(order)
    for k in range(2):
        st, sq = _default_values(txt, ("CIEDE2000", "CIEDE2000_DE")[k], ("CIEDE2000", "CIEDE2000 mean dE00")[k])
        assert st["min"] == min(r[k] for r in rows) and st["max"] == max(r[k] for r in rows) and st["p50"] == sorted(r[k] for r in rows)[CN // 2]
        assert st["min"] == agg[NAMES[k]]["min"] and st["mean"] == agg[NAMES[k]]["mean"] and sq == seq[k]
    if beside:  # the other metrics' output is unchanged and comes first
        pl = [json.loads(x) for x in plain["json-lines"].splitlines() if x.strip()]
        for i in range(CN):
            assert [lines[i][n] for n in first] == [pl[i][n] for n in first]
        assert [agg[n] for n in first] == [pl[CN][n] for n in first]
        assert out[1].split(",")[:len(first)] == plain["csv"].splitlines()[1].split(",") and txt.startswith(plain["default"])
        pj = json.loads(plain["json"])
        assert all(js[n] == pj[n] for n in first)


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = (int(t) for t in f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").reshape(h, w)
    return data[::-1]  # PFM rows run bottom to top


def test_cli_matrix_libvmaf_and_maps(tmp_path):
    pairs = _pairs(8)
    a, b = _y4m_pairs(tmp_path, pairs, 8)
    col = lambda *args: [[json.loads(x)[n] for n in NAMES] for x in _cli(a, b, "-m", "ciede2000", *args, "--output", "json-lines").splitlines()[:CN]]
    r601, _, maps601 = _binding(pairs, 8, "bt601")
    r709, _, _ = _binding(pairs, 8, "bt709")
    rvmaf, _, _ = _binding(pairs, 8, "libvmaf", tm.ciede.K_LIBVMAF)
    assert r601 != r709 and r709 != rvmaf
    assert col() == r601 == col("--matrix-coefficients", "6") == col("--matrix-coefficients", "5")  # 2 = by height: 43 rows are BT.601
    assert col(*BT709) == r709 == col("--matrix-coefficients", "1")
    assert col("--ciede-libvmaf") == rvmaf == col("--ciede-libvmaf", *BT709)
    prefix = str(tmp_path / "de_")
    assert col("--ciede-map", prefix, "--batch", "2") == r601
    for i in range(CN):
        m = _read_pfm(prefix + "%06d.pfm" % i)
        assert m.shape == (CH, CW) and np.array_equal(m.view(np.uint32), maps601[i].view(np.uint32))
    assert not os.path.exists(prefix + "%06d.pfm" % CN)


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


def test_cli_refuses_rgb_and_full_range_input(tmp_path):
    pa, pb = _ppm_pair(tmp_path)
    out = subprocess.run([CLI, pa, pb, "-m", "ciede2000"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "ciede2000 needs 4:2:0 YUV input" in out.stderr, (out.returncode, out.stderr)
    a, b = _y4m_pairs(tmp_path, _pairs(8)[:1], 8)
    out = subprocess.run([CLI, a, b, "-m", "ciede2000", "--full-range"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0, out.stdout


# what the parent commit's binary printed for these arguments on the inputs of _parent_files(dir, kind): recorded once with
# record_parent_cli(<the parent's turbo-metrics>, GOLDEN, <a scratch directory>) on an MI355X
PARENT_CASES = {
    "y4m8_psnr_ssim_default": ("y4m8", ["-m", "psnr", "-m", "ssim"]),
    "y4m8_ssimu_xpsnr_json": ("y4m8", ["-m", "ssimulacra2", "-m", "xpsnr", "--output", "json"]),
    "y4m8_yuv_hvs_motion_jsonl": ("y4m8", ["-m", "psnr", "-m", "psnr-yuv", "-m", "ssim-yuv", "-m", "psnr-hvs", "-m", "psnr-hvs-m", "--motion", "--output", "json-lines"]),
    "y4m10_vif_adm_scenes_csv": ("y4m10", ["-m", "vif", "-m", "adm", "--scenes", "--batch", "2", "--output", "csv"]),
    "y4m10_hvs_cambi_csv": ("y4m10", ["-m", "psnr-hvs", "-m", "psnr-yuv", "-m", "cambi", "--output", "csv"]),
    "y4m10_hvs_default": ("y4m10", ["-m", "psnr-hvs-m", "-m", "ssim-yuv", *BT709]),
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


def test_cli_without_the_new_value_is_byte_identical_with_the_parents(tmp_path):
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(PARENT_CASES)
    got = _run_parent_cases(CLI, tmp_path)
    for name in PARENT_CASES:
        assert got[name] == want[name], name
        assert not re.search(r"ciede", got[name].lower()), name
