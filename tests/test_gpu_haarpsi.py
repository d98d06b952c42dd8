"""GPU tier of HaarPSI: libturbometrics_haarpsi.so through tm.HaarPsi against the emulated kernel source (Q, WS and
the map bit for bit: the same operations in the same order, all correctly rounded, the exponential included) and against the float64
restatement inside the tolerance measured on the CPU (tests/haarpsi_util.py); hand values; pitches, garbage, memory kinds, repeats; the
map; state rules; the CLI's column against the binding in the four output and the four input formats; and the CLI without -m haarpsi
against a recorded run of the parent commit's binary (tests/golden/haarpsi_parent_cli.json)."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import haarpsi_ref as R
from tests import haarpsi_util as U
from tm_pkg import tm

pytestmark = pytest.mark.gpu

SIZES = U.shapes()
BATCH_KINDS = ("noise", "blur", "ramp_one")  # batch 3, different content per slot

_REF = {}


def _want(w, h, bits, kind, seed):
    """the float64 restatement of one test picture, computed once"""
    key = (w, h, bits, kind, seed)
    if key not in _REF:
        _REF[key] = R.haarpsi(*U.pair(w, h, bits, kind, seed=seed), bits)
    return _REF[key]


@pytest.fixture(scope="module", autouse=True)
def _hip():
    tm.init_hip(0)


def _torch(p):
    """the same bytes as a torch tensor (signed views: torch has no unsigned 16- / 32-bit kernels to copy with)"""
    import torch
    return torch.from_numpy(p.view({np.uint16: np.int16, np.uint32: np.int32}.get(p.dtype.type, p.dtype)))


class Placed:
    """a plane inside a larger buffer of garbage: `view` is the host array the emulation reads, tensor(mem) the same bytes at the same
    base offset and pitch in host, pinned or device memory, a strided view that the binding hands on as it is (a numpy array would be
    copied tight before the library sees it, and a host plane is staged to a pitch of the library's own: only a DEVICE view carries
    its base and pitch to the kernel)"""

    def __init__(self, p, base, pitch):
        p = np.ascontiguousarray(p)
        self.rows, self.cols, self.base, self.pitch = p.shape[0], p.shape[1], base, pitch
        n = base + self.rows * pitch
        raw = np.random.default_rng(11).integers(0, 256, n * p.itemsize + 16, dtype=np.uint8)
        off = (-raw.ctypes.data) % 16  # the buffer's first element is 16-byte aligned, as a device allocation's is
        self.flat = raw[off:off + n * p.itemsize].view(p.dtype)
        self.view = self.flat[base:].reshape(self.rows, pitch)[:, :self.cols]
        self.view[:] = p

    def tensor(self, mem):
        t = _torch(self.flat)
        t = t.cuda() if mem == "device" else t.pin_memory() if mem == "pinned" else t
        return t[self.base:].view(self.rows, self.pitch)[:, :self.cols]


def place(p, aligned, pad=3):
    """aligned: base and pitch multiples of 16 bytes (the wide loads), garbage behind each row; otherwise a base 1 element in and a pitch
    that is no multiple of 16 bytes (the sample-by-sample path)"""
    cols, sz = p.shape[1], p.itemsize
    if aligned:
        pl = Placed(p, 16 // sz, ((cols + pad) * sz + 15) // 16 * 16 // sz)
    else:
        pitch = cols + pad
        pl = Placed(p, 1, pitch + 1 if pitch * sz % 16 == 0 else pitch)
    assert ((pl.view.ctypes.data % 16 == 0) and (pl.pitch * sz % 16 == 0)) == bool(aligned)
    assert aligned or (pl.view.ctypes.data % 16 != 0 and pl.pitch * sz % 16 != 0)
    return pl


def place_all(frames, aligned, pad=3):
    return [tuple(place(p, aligned, pad) for p in pr) for pr in frames]


def views(placed):
    return [tuple(pl.view for pl in pr) for pr in placed]


def _compute(v, frames, mem="host"):
    """the pairs as slots 0 .. n-1 of one compute -> [(q, ws)].  A pair of Placed planes goes in as strided tensors in `mem`; a pair of
    plain arrays as tight copies (numpy for "host")"""
    import torch
    keep = []
    for s, (pr, pd) in enumerate(frames):
        if isinstance(pr, Placed):
            pr, pd = pr.tensor(mem), pd.tensor(mem)
            if mem == "device":
                sz = pr.element_size()
                assert (pr.data_ptr() % 16 == 0) == (pr.stride(0) * sz % 16 == 0) and pr.stride(0) > pr.shape[1]
        elif mem == "device":
            pr, pd = _torch(np.ascontiguousarray(pr)).cuda(), _torch(np.ascontiguousarray(pd)).cuda()
        elif mem == "pinned":
            pr, pd = _torch(np.ascontiguousarray(pr)).pin_memory(), _torch(np.ascontiguousarray(pd)).pin_memory()
        keep.append((pr, pd))
        v.set_pair(s, pr, pd)
    if mem == "device":
        torch.cuda.synchronize()
    v.compute(len(frames))
    return [(f.q, f.ws) for f in v.frames(len(frames))]


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_library_against_emulation_and_restatement(layout, bits):
    """every size of the sparse tile-edge set, batch 3 with different content per slot, as device tensors that are views into larger
    buffers: once with a base 1 element in and a pitch that is no multiple of 16 bytes (the kernel's sample-by-sample path), once with
    base and pitch 16-byte aligned (the wide loads); the emulation reads the same layout on the host.  Then a compute of fewer slots
    than the batch from tight host arrays (the staging upload)"""
    for w, h in SIZES:
        pairs = [U.pair(w, h, bits, k, seed=w + h) for k in BATCH_KINDS]
        tight = U.planes_of(layout, pairs, bits)
        for aligned in (False, True):
            placed = place_all(tight, aligned)
            emul, emaps = U.emulate(w, h, layout, bits, [len(pairs)], views(placed), maps=True)
            with tm.HaarPsi(w, h, layout, bits, batch=len(pairs), maps=True) as v:
                got = _compute(v, placed, "device")
                fr = v.frames(len(pairs))
                maps = [v.map(s) for s in range(len(pairs))]
                fewer = _compute(v, tight[1:3])
            assert fewer == emul[1:3], (w, h, aligned)
            for kind, g, e, f, m, em in zip(BATCH_KINDS, got, emul, fr, maps, emaps):
                assert g == e, (w, h, kind, aligned)  # bit for bit
                assert m.dtype == np.float32 and np.array_equal(m, em), (w, h, kind, aligned)
                want = _want(w, h, bits, kind, w + h)
                assert abs(f.haarpsi - want.haarpsi) <= U.ABS_TOL, (w, h, kind, f.haarpsi, want.haarpsi)
                assert np.abs(m.astype(np.float64) - want.sim).max() < 3e-7


def test_hand_values():
    """the literals of tests/test_haarpsi_cpu.py: zero against flat v at 4 x 4 (WS = 64 v, two kinds of position), identical pictures,
    two black pictures, and zero against flat 100 at 16 x 16"""
    for layout, bits in (("y8", 8), ("y16_msb", 10), ("y16_low", 16), ("y10_packed", 10)):
        k = 1 << (bits - 8)
        flats = [(np.zeros((4, 4), np.int64), np.full((4, 4), v * k, np.int64)) for v in (1, 100, 255)]
        with tm.HaarPsi(4, 4, layout, bits, batch=3) as v:
            _compute(v, U.planes_of(layout, flats, bits))
            fr = v.frames(3)
        for f, val in zip(fr, (1, 100, 255)):
            sA = 30.0 / (val * val + 30.0)
            sB = 1.0 - (val * val / (val * val + 120.0) + val * val / (val * val + 30.0)) / 2
            want = R.logit((R.sigmoid(sA) + R.sigmoid(sB)) / 2) ** 2
            assert f.ws == 64 * val * k and abs(f.haarpsi - want) <= U.ABS_TOL, (layout, val)
    a, _ = U.pair(33, 19, 8, "noise", 3)
    z = np.zeros((19, 33), np.int64)
    with tm.HaarPsi(33, 19, "y8", 8, batch=2, maps=True) as v:
        _compute(v, U.planes_of("y8", [(a, a), (z, z)], 8))
        same, black = v.frames(2)
        assert abs(same.haarpsi - 1.0) <= U.ABS_TOL and abs(same.q / same.ws - U.kernel_q(1.0)) < 1e-12
        assert (v.map(0) == 1.0).all() and (v.map(1) == 1.0).all()
        assert (black.q, black.ws) == (0.0, 0) and math.isnan(black.haarpsi)
    with tm.HaarPsi(16, 16, "y8", 8) as v:
        _compute(v, U.planes_of("y8", [(np.zeros((16, 16), np.int64), np.full((16, 16), 100, np.int64))], 8))
        assert abs(v.frames(1)[0].haarpsi - 0.141890556) <= U.ABS_TOL + 1e-9


def test_pitches_garbage_memory_kinds_and_repeats():
    """one odd size: tight planes, planes with garbage behind each row at a pitch that is no multiple of 16 bytes and a base 1 element
    in, and 16-byte aligned ones, each in host, pinned and device memory as strided views that keep base and pitch"""
    w, h = SIZES[8]  # 2 TW + 9 wide: odd, the halo past a tile edge and the picture edge
    assert w % 2 == 1
    for layout, bits in (("y8", 8), ("y16_msb", 10), ("y16_low", 12), ("y10_packed", 10)):
        pairs = [U.pair(w, h, bits, k, seed=4) for k in ("noise", "blur", "near_peak")]
        tight = U.planes_of(layout, pairs, bits)
        loose = place_all(tight, False, pad={"y8": 4, "y10_packed": 1}.get(layout, 5))
        aligned = place_all(tight, True, pad=2)
        with tm.HaarPsi(w, h, layout, bits, batch=3) as v:
            first = _compute(v, tight)
            assert _compute(v, tight) == first  # a repeated compute: equal bits
            for frames in (tight, loose, aligned):
                for mem in ("host", "pinned", "device"):
                    assert _compute(v, frames, mem) == first, (layout, mem)
            assert _compute(v, tight[1:2]) == first[1:2]  # a smaller compute on the same buffers
        assert first == U.emulate(w, h, layout, bits, [3], tight) == U.emulate(w, h, layout, bits, [3], views(loose))


def test_map_pitch_refusal_and_sums_with_and_without_maps():
    w, h = SIZES[6]
    pairs = [U.pair(w, h, 8, k, seed=6) for k in ("noise", "blur")]
    frames = U.planes_of("y8", pairs, 8)
    emul, emaps = U.emulate(w, h, "y8", 8, [2], frames, maps=True)
    with tm.HaarPsi(w, h, "y8", 8, batch=2, maps=True) as v:
        with_maps = _compute(v, frames)
        h2, w2 = (h + 1) // 2, (w + 1) // 2
        buf = np.full((h2 + 1, w2 + 5), -3.0, np.float32)
        m = v.map(1, out=buf)  # rows at a caller's pitch
        assert m.shape == (h2, w2) and np.array_equal(m, emaps[1]) and (buf[:, w2:] == -3.0).all() and (buf[h2:] == -3.0).all()
        assert m.max() <= 1.0 and m.min() > 0.0
        with pytest.raises(tm.haarpsi.HaarPsiError) as err:
            v.map(2)
        assert err.value.code == tm.ffi.TM_ERR_STATE
    with tm.HaarPsi(w, h, "y8", 8, batch=2) as v:
        assert _compute(v, frames) == with_maps == emul
        with pytest.raises(tm.haarpsi.HaarPsiError) as err:
            v.map(0)  # maps=False refuses
        assert err.value.code == tm.ffi.TM_ERR_STATE


def test_state_rules():
    w, h = 32, 32
    (pr, pd), = U.planes_of("y8", [U.pair(w, h, 8, "noise", 1)], 8)
    with tm.HaarPsi(w, h, "y8", 8, batch=2) as v:
        assert v.mem_usage() > 0
        v.set_pair(0, pr, pd)
        with pytest.raises(tm.haarpsi.HaarPsiError) as e:
            v.compute(2)  # slot 1 was not set
        assert e.value.code == tm.ffi.TM_ERR_STATE
        v.compute_async(1)
        with pytest.raises(tm.haarpsi.HaarPsiError) as e:
            v.compute_async(1)  # a compute is pending
        assert e.value.code == tm.ffi.TM_ERR_STATE
        v.sync()
        with pytest.raises(tm.haarpsi.HaarPsiError) as e:
            v.compute(1)  # every compute consumes its pairs: a slot not set again
        assert e.value.code == tm.ffi.TM_ERR_STATE
        with pytest.raises(tm.haarpsi.HaarPsiError) as e:
            v.frames(2)  # not slots of the last compute
        assert e.value.code == tm.ffi.TM_ERR_STATE
        assert v.frames(1)[0].ws > 0


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
GOLDEN = os.path.join(ROOT, "tests", "golden", "haarpsi_parent_cli.json")
CW, CH, CN = 99, 43, 3  # odd both ways: the zero column and row enter S
NAME = "haarpsi"
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


def _binding(pairs, bits, maps=False):
    """per frame the value and the sequence value (from the summed Q and WS) from tm.HaarPsi and the library's host function"""
    layout = "y8" if bits == 8 else "y16_low"
    with tm.HaarPsi(CW, CH, layout, bits, batch=len(pairs), maps=maps) as v:
        _compute(v, U.planes_of(layout, pairs, bits))
        fr = v.frames(len(pairs))
        mp = [v.map(s) for s in range(len(pairs))] if maps else None
    rows = [f.haarpsi for f in fr]
    q = 0.0
    for f in fr:
        q += f.q
    seq = tm.haarpsi.score(q, sum(f.ws for f in fr))
    return (rows, seq, mp) if maps else (rows, seq)


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("beside", [(), ("-m", "psnr"), ("-m", "xpsnr", "-m", "gmsd", "--siti")])
def test_cli_against_the_binding_in_every_output_format(tmp_path, beside, bits):
    pairs = _pairs(bits)
    a, b = _y4m_pairs(tmp_path, pairs, bits)
    rows, seq = _binding(pairs, bits)
    base = (a, b, *beside, "-m", "haarpsi")
    first = {0: [], 2: ["psnr"], 5: ["xpsnr_y", "xpsnr_u", "xpsnr_v", "si", "ti", "gmsd", "gmsm"]}[len(beside)]
    plain = {fmt: _cli(a, b, *beside, "--output", fmt) for fmt in FORMATS} if beside else {}
    # json-lines: one line per frame, then the aggregates with the sequence value
    lines = [json.loads(x) for x in _cli(*base, "--output", "json-lines").splitlines() if x.strip()]
    assert len(lines) == CN + 1
    for i in range(CN):
        assert list(lines[i]) == first + [NAME] and lines[i][NAME] == rows[i]
    agg = lines[CN]
    assert agg["frame_count"] == CN and list(agg)[-1] == NAME
    assert agg[NAME]["sequence"] == seq and agg[NAME]["min"] == min(rows) and agg[NAME]["max"] == max(rows)
    # json
    js = json.loads(_cli(*base, "--output", "json"))
    assert list(js)[-1] == NAME and js[NAME]["scores"] == rows and js[NAME]["sequence"] == seq and js[NAME]["stats"]["max"] == max(rows)
    # csv: the header, a row per frame as it is computed, then the header and the rows again
    out = _cli(*base, "--output", "csv").splitlines()
    assert out[0] == ",".join(first + [NAME]) == out[CN + 1] and len(out) == 2 * CN + 2
    for i in range(CN):
        assert float(out[1 + i].split(",")[-1]) == rows[i] and out[CN + 2 + i] == out[1 + i]
    # default
    txt = _cli(*base)
    st, sq = _default_values(txt, "HaarPSI", "HaarPSI")
    assert st["min"] == min(rows) and st["max"] == max(rows) and st["p50"] == sorted(rows)[CN // 2]
    assert st["min"] == agg[NAME]["min"] and st["mean"] == agg[NAME]["mean"] and sq == seq
    assert txt.index("HaarPSI: Stats {") < txt.index("HaarPSI (sequence): ")
    if beside:  # the other metrics' output is unchanged and comes first
        pl = [json.loads(x) for x in plain["json-lines"].splitlines() if x.strip()]
        for i in range(CN):
            assert [lines[i][n] for n in first] == [pl[i][n] for n in first]
        assert [agg[n] for n in first] == [pl[CN][n] for n in first]
        assert out[1].split(",")[:len(first)] == plain["csv"].splitlines()[1].split(",") and txt.startswith(plain["default"])
        pj = json.loads(plain["json"])
        assert all(js[n] == pj[n] for n in first)


def test_cli_input_formats_maps_and_a_value_that_is_not_finite(tmp_path):
    """the four input formats (Y4M 8-bit, Y4M 10-bit, raw 8-bit, raw 10-bit), --haarpsi-map against map(); two black pictures print as
    psnr_u prints its non-finite values"""
    for bits in (8, 10):
        pairs = _pairs(bits)
        rows, seq, maps = _binding(pairs, bits, maps=True)
        d = tmp_path / str(bits)
        d.mkdir()
        for kind in ("y4m", "raw"):
            a, b = (_y4m_pairs if kind == "y4m" else _raw_pairs)(d, pairs, bits)
            extra = [] if kind == "y4m" else ["--width", str(CW), "--height", str(CH), "--bits", str(bits)]
            prefix = str(d / (kind + "_map"))
            lines = [json.loads(x) for x in _cli(a, b, "-m", "haarpsi", "--haarpsi-map", prefix, "--batch", "2", *extra, "--output", "json-lines").splitlines() if x.strip()]
            assert [x[NAME] for x in lines[:CN]] == rows and lines[CN][NAME]["sequence"] == seq
            for i in range(CN):
                with open("%s%06d.pfm" % (prefix, i), "rb") as f:
                    assert f.readline() == b"Pf\n" and f.readline().split() == [str((CW + 1) // 2).encode(), str((CH + 1) // 2).encode()]
                    scale = float(f.readline())
                    data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").reshape((CH + 1) // 2, (CW + 1) // 2)
                assert np.array_equal(data[::-1], maps[i]), (kind, bits, i)  # PFM rows run bottom to top
            assert not os.path.exists("%s%06d.pfm" % (prefix, CN))
    d = tmp_path / "black"
    d.mkdir()
    z = np.zeros((CH, CW), np.int64)
    a, b = _y4m_pairs(d, [(z, z)], 8)
    lines = [json.loads(x) for x in _cli(a, b, "-m", "haarpsi", "--output", "json-lines").splitlines() if x.strip()]
    assert lines[0] == {NAME: None} and lines[1][NAME]["sequence"] is None and lines[1][NAME]["min"] is None
    assert _cli(a, b, "-m", "haarpsi", "--output", "csv").splitlines()[:2] == [NAME, "NaN"]
    assert "HaarPSI (sequence): NaN" in _cli(a, b, "-m", "haarpsi")


def test_cli_beside_every_other_selection(tmp_path):
    """-m haarpsi beside --motion, --scenes, --siti and the other feature libraries: its column comes last and is the binding's"""
    pairs = _pairs(8)
    a, b = _y4m_pairs(tmp_path, pairs, 8)
    rows, seq = _binding(pairs, 8)
    sel = ("-m", "ssim", "-m", "vif", "-m", "adm", "-m", "cambi", "-m", "psnr-yuv", "-m", "ssim-yuv", "-m", "psnr-hvs-m", "-m", "ciede2000", "-m", "gmsd", "--motion", "--scenes", "--siti")
    lines = [json.loads(x) for x in _cli(a, b, *sel, "-m", "haarpsi", "--batch", "2", "--output", "json-lines").splitlines() if x.strip()]
    plain = [json.loads(x) for x in _cli(a, b, *sel, "--batch", "2", "--output", "json-lines").splitlines() if x.strip()]
    assert len(lines) == CN + 1 == len(plain)
    for i in range(CN):
        assert list(lines[i]) == list(plain[i]) + [NAME] and lines[i][NAME] == rows[i]
        assert {k: v for k, v in lines[i].items() if k != NAME} == plain[i]
    assert lines[CN][NAME]["sequence"] == seq and list(lines[CN])[-1] == NAME


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
    out = subprocess.run([CLI, pa, pb, "-m", "haarpsi"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "haarpsi needs YUV input" in out.stderr, (out.returncode, out.stderr)


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
    "y4m10_gmsd_psnr_default": ("y4m10", ["-m", "gmsd", "-m", "psnr"]),
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
        assert "haarpsi" not in got[name].lower(), name
