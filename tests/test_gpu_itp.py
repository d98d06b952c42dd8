"""GPU tier of dE ITP: libturbometrics_itp.so through tm.Itp against the emulated kernel source (de_sum, de_max
and the whole map bit for bit: the same operations in the same order, all correctly rounded, log2 / exp2 / pow included) and against the
float64 restatement inside the tolerance measured on the CPU (tests/itp_util.py); hand values; pitches, garbage, memory kinds, repeats,
slot positions, batch sizes; the map; state rules; the CLI's columns against the binding in the four output and the four input formats;
and the CLI without -m deitp against a recorded run of the parent commit's binary (tests/golden/itp_parent_cli.json)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import itp_ref as R
from tests import itp_util as U
from tm_pkg import tm

pytestmark = pytest.mark.gpu

SIZES = U.shapes()
BATCH_KINDS = ("noise", "near_black", "one_code")  # batch 3, different content per slot
TRANSFERS = ("pq", "hlg")

_REF = {}


def _want(w, h, bits, kind, transfer, seed):
    """the float64 restatement of one test picture, computed once"""
    key = (w, h, bits, kind, transfer, seed)
    if key not in _REF:
        pr = U.pair(w, h, bits, kind, seed=seed)
        _REF[key] = R.picture(pr[0], pr[1], bits, transfer)
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
    base offset and pitch in host, pinned or device memory, a strided view that the binding hands on as it is (only a DEVICE view
    carries its base and pitch to the kernel: a host plane is staged to a pitch of the library's own)"""

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
    """[(ref planes, dis planes)] -> the same with every plane Placed; Cb and Cr get one pitch (equal shapes)"""
    return [tuple([place(p, aligned, pad) for p in side] for side in pr) for pr in frames]


def views(placed):
    return [tuple([pl.view for pl in side] for side in pr) for pr in placed]


def _compute(v, frames, mem="host", maps=False):
    """the pairs as slots 0 .. n-1 of one compute -> [(de_sum, de_max, map or None)].  Placed planes go in as strided tensors in `mem`;
    plain arrays as tight copies (numpy for "host")"""
    import torch
    keep = []
    for s, pr in enumerate(frames):
        sides = []
        for side in pr:
            if isinstance(side[0], Placed):
                t = [pl.tensor(mem) for pl in side]
                if mem == "device":
                    assert all((p.data_ptr() % 16 == 0) == (p.stride(0) * p.element_size() % 16 == 0) and p.stride(0) > p.shape[1] for p in t)
            elif mem == "device":
                t = [_torch(np.ascontiguousarray(p)).cuda() for p in side]
            elif mem == "pinned":
                t = [_torch(np.ascontiguousarray(p)).pin_memory() for p in side]
            else:
                t = list(side)
            sides.append(t)
        keep.append(sides)
        v.set_pair(s, sides[0], sides[1])
    if mem == "device":
        torch.cuda.synchronize()
    v.compute(len(frames))
    return [(f.de_sum, f.de_max, v.map(s) if maps else None) for s, f in enumerate(v.frames(len(frames)))]


def _same(got, want):
    return len(got) == len(want) and all(g[:2] == e[:2] and (g[2] is None or e[2] is None or (g[2].dtype == np.float32 and np.array_equal(g[2].view(np.uint32), e[2].view(np.uint32))))
                                         for g, e in zip(got, want))


_DEVICE = {"atol": 0.0, "rtol": 0.0, "mean": 0.0}


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_library_against_emulation_and_restatement(layout, bits):
    """every shape, both transfers, batch 3 with different content per slot, as device tensors that are views into larger buffers: once
    with a base 1 element in and a pitch that is no multiple of 16 bytes (the kernel's sample-by-sample path), once with base and pitch
    16-byte aligned (the wide loads); the emulation reads the same layout on the host.  Then a compute of fewer slots than the batch from
    tight host arrays (the staging upload).  Prints the device's own figures against the restatement"""
    for w, h in SIZES:
        pairs = [U.pair(w, h, bits, k, seed=w + h) for k in BATCH_KINDS]
        tight = U.frames_of(layout, pairs, w, h, bits)
        for transfer in TRANSFERS:
            for aligned in (False, True):
                placed = place_all(tight, aligned)
                emul = U.emulate(w, h, layout, bits, [len(pairs)], views(placed), transfer=transfer)
                with tm.Itp(w, h, layout, bits, transfer=transfer, batch=len(pairs), maps=True) as v:
                    got = _compute(v, placed, "device", maps=True)
                    fewer = _compute(v, tight[1:3], maps=True)
                assert _same(got, emul), (w, h, transfer, aligned)  # bit for bit
                assert _same(fewer, emul[1:3]), (w, h, transfer, aligned)
            for kind, g in zip(BATCH_KINDS, got):
                want = _want(w, h, bits, kind, transfer, w + h)
                why = U.agrees(g[2], want, U.ATOL, U.RTOL)
                assert why is None, (w, h, transfer, kind, why)
                assert U.mean_rel(g[0], want) <= U.MEAN_REL_TOL and abs(g[1] - want.de_max) <= U.ATOL + U.RTOL * want.de_max
                a, r = U.errors(g[2], want)
                _DEVICE.update(atol=max(_DEVICE["atol"], a), rtol=max(_DEVICE["rtol"], r), mean=max(_DEVICE["mean"], U.mean_rel(g[0], want)))
    print("device figures so far: atol %.3e rtol %.3e mean rel %.3e" % (_DEVICE["atol"], _DEVICE["rtol"], _DEVICE["mean"]))
    assert _DEVICE["atol"] <= U.ATOL_LIMIT


def test_hand_values():
    """identical pictures give exactly 0; a neutral 512 -> 513 luma step at 10 bits the restatement's value (about 0.82); the sides
    exchanged the same bits"""
    w, h = 33, 19
    a, b = U.pair(w, h, 10, "noise", 3)
    g = (np.full((h, w), 512), np.full(((h + 1) // 2, (w + 1) // 2), 512), np.full(((h + 1) // 2, (w + 1) // 2), 512))
    g1 = (g[0] + 1, g[1], g[2])
    want = R.picture(g, g1, 10, "pq")
    for layout in ("p016", "i420", "i420p10"):
        with tm.Itp(w, h, layout, 10, batch=4, maps=True) as v:
            same, step, fwd, bwd = _compute(v, U.frames_of(layout, [(a, a), (g, g1), (a, b), (b, a)], w, h, 10, dirty=False), maps=True)
            fr = v.frames(4)
        assert same[:2] == (0.0, 0.0) and not same[2].any()
        assert abs(fr[1].de_mean - want.de_mean) <= U.ATOL and abs(want.de_mean - 0.82) < 0.005 and fr[1].pixels == w * h
        assert fr[1].de_mean == fr[1].de_sum / (w * h) and (step[2] == np.float32(step[1])).all()
        assert _same([fwd], [bwd])


def test_pitches_garbage_memory_kinds_slots_batches_and_repeats():
    """one odd size of more than one tile each way: tight planes, planes with garbage behind each row at a pitch that is no multiple of
    16 bytes and a base 1 element in, and 16-byte aligned ones, each in host, pinned and device memory; repeats, batch 1 against batch
    3, and a pair moved to another slot"""
    w, h = 259, 37
    for layout, bits in (("nv12", 8), ("p016", 10), ("i420", 12), ("i420p10", 10)):
        pairs = [U.pair(w, h, bits, k, seed=4) for k in ("noise", "near_neutral", "near_peak")]
        tight = U.frames_of(layout, pairs, w, h, bits)
        loose = place_all(tight, False, pad={"nv12": 4, "i420p10": 1}.get(layout, 5))
        aligned = place_all(tight, True, pad=2)
        with tm.Itp(w, h, layout, bits, batch=3) as v:
            first = _compute(v, tight)
            assert _compute(v, tight) == first  # a repeated compute: equal bits
            for frames in (tight, loose, aligned):
                for mem in ("host", "pinned", "device"):
                    assert _compute(v, frames, mem) == first, (layout, mem)
            assert _compute(v, tight[1:2]) == first[1:2]  # batch 1 on the same buffers, the pair in another slot
            assert _compute(v, [tight[2], tight[0]]) == [first[2], first[0]]
        with tm.Itp(w, h, layout, bits, batch=1) as v:
            assert [_compute(v, [f])[0] for f in tight] == first
        assert _same(first, U.emulate(w, h, layout, bits, [3], tight, maps=False))


def test_map_pitch_refusal_and_sums_with_and_without_maps():
    w, h = SIZES[5]
    pairs = [U.pair(w, h, 10, k, seed=6) for k in ("noise", "primaries")]
    frames = U.frames_of("p016", pairs, w, h, 10)
    emul = U.emulate(w, h, "p016", 10, [2], frames, transfer="hlg")
    with tm.Itp(w, h, "p016", 10, transfer="hlg", batch=2, maps=True) as v:
        with_maps = _compute(v, frames, maps=True)
        assert _same(with_maps, emul)
        buf = np.full((h, w + 3), -3.0, np.float32)
        L = tm.itp.lib()
        assert L.tm_itp_get_map(v._h, 1, buf.ctypes.data, (w + 3) * 4) == tm.ffi.TM_OK  # rows at a caller's pitch
        assert np.array_equal(buf[:, :w], emul[1][2]) and (buf[:, w:] == -3.0).all()
        for pitch in (4 * w - 4, 4 * w + 2):
            assert L.tm_itp_get_map(v._h, 1, buf.ctypes.data, pitch) == tm.ffi.TM_ERR_INVALID_ARG
        with pytest.raises(tm.itp.ItpError) as err:
            v.map(2)
        assert err.value.code == tm.ffi.TM_ERR_STATE
    with tm.Itp(w, h, "p016", 10, transfer="hlg", batch=2) as v:
        assert [g[:2] for g in _compute(v, frames)] == [g[:2] for g in with_maps]
        with pytest.raises(tm.itp.ItpError) as err:
            v.map(0)  # maps=False refuses
        assert err.value.code == tm.ffi.TM_ERR_STATE


def test_state_rules():
    w, h = 32, 32
    (pr, pd), = U.frames_of("nv12", [U.pair(w, h, 8, "noise", 1)], w, h, 8)
    with tm.Itp(w, h, "nv12", 8, batch=2) as v:
        assert v.mem_usage() > 0
        v.set_pair(0, pr, pd)
        with pytest.raises(tm.itp.ItpError) as e:
            v.compute(2)  # slot 1 was not set
        assert e.value.code == tm.ffi.TM_ERR_STATE
        v.compute_async(1)
        with pytest.raises(tm.itp.ItpError) as e:
            v.compute_async(1)  # a compute is pending
        assert e.value.code == tm.ffi.TM_ERR_STATE
        v.sync()
        with pytest.raises(tm.itp.ItpError) as e:
            v.compute(1)  # every compute consumes its pairs: a slot not set again
        assert e.value.code == tm.ffi.TM_ERR_STATE
        with pytest.raises(tm.itp.ItpError) as e:
            v.frames(2)  # not slots of the last compute
        assert e.value.code == tm.ffi.TM_ERR_STATE
        assert v.frames(1)[0].de_sum > 0


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
GOLDEN = os.path.join(ROOT, "tests", "golden", "itp_parent_cli.json")
CW, CH, CN = 99, 43, 3  # odd both ways
NAMES = ["deitp", "deitp_max"]
FORMATS = ("json-lines", "json", "csv", "default")


def _cli(*args, cli=CLI):
    out = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def _pairs(bits):
    return [U.pair(CW, CH, bits, "near_neutral", seed=30 + i) for i in range(CN)]


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


def _binding(pairs, bits, transfer="pq"):
    """per frame the two values, the two sequence values and the maps from tm.Itp"""
    with tm.Itp(CW, CH, "i420", bits, transfer=transfer, batch=len(pairs), maps=True) as c:
        got = _compute(c, U.frames_of("i420", pairs, CW, CH, bits), maps=True)
        fr = c.frames(len(pairs))
    rows = [[f.de_mean, f.de_max] for f in fr]
    s = 0.0
    for f in fr:
        s += f.de_sum
    return rows, [s / sum(f.pixels for f in fr), max(f.de_max for f in fr)], [g[2] for g in got]


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("beside", [(), ("-m", "psnr"), ("-m", "ciede2000", "-m", "gmsd", "--siti")])
def test_cli_against_the_binding_in_every_output_format(tmp_path, beside, bits):
    pairs = _pairs(bits)
    a, b = _files(tmp_path, pairs, bits, True)
    rows, seq, _ = _binding(pairs, bits)
    base = (a, b, *beside, "-m", "deitp")
    first = {0: [], 2: ["psnr"], 5: ["ciede2000", "ciede2000_de", "si", "ti", "gmsd", "gmsm"]}[len(beside)]
    plain = {fmt: _cli(a, b, *beside, "--output", fmt) for fmt in FORMATS} if beside else {}
    # json-lines: one line per frame, then the aggregates with the sequence values
    lines = [json.loads(x) for x in _cli(*base, "--output", "json-lines").splitlines() if x.strip()]
    assert len(lines) == CN + 1
    for i in range(CN):
        assert list(lines[i]) == first + NAMES and [lines[i][n] for n in NAMES] == rows[i]
    agg = lines[CN]
    assert agg["frame_count"] == CN and list(agg)[-2:] == NAMES
    for k, n in enumerate(NAMES):
        col = [r[k] for r in rows]
        assert agg[n]["sequence"] == seq[k] and agg[n]["min"] == min(col) and agg[n]["max"] == max(col)
    # json
    js = json.loads(_cli(*base, "--output", "json"))
    assert list(js)[-2:] == NAMES
    for k, n in enumerate(NAMES):
        assert js[n]["scores"] == [r[k] for r in rows] and js[n]["sequence"] == seq[k]
    # csv: the header, a row per frame as it is computed, then the header and the rows again
    out = _cli(*base, "--output", "csv").splitlines()
    assert out[0] == ",".join(first + NAMES) == out[CN + 1] and len(out) == 2 * CN + 2
    for i in range(CN):
        assert [float(t) for t in out[1 + i].split(",")[-2:]] == rows[i] and out[CN + 2 + i] == out[1 + i]
    # default
    txt = _cli(*base)
    for k, (block, line) in enumerate((("DEITP", "dE ITP mean"), ("DEITP_MAX", "dE ITP max"))):
        st, sq = _default_values(txt, block, line)
        col = [r[k] for r in rows]
        assert st["min"] == min(col) and st["max"] == max(col) and st["p50"] == sorted(col)[CN // 2] and sq == seq[k]
    assert txt.index("DEITP: Stats {") < txt.index("dE ITP mean (sequence): ") < txt.index("DEITP_MAX: Stats {")
    if beside:  # the other metrics' output is unchanged and comes first
        pl = [json.loads(x) for x in plain["json-lines"].splitlines() if x.strip()]
        for i in range(CN):
            assert [lines[i][n] for n in first] == [pl[i][n] for n in first]
        assert [agg[n] for n in first] == [pl[CN][n] for n in first]
        assert out[1].split(",")[:len(first)] == plain["csv"].splitlines()[1].split(",") and txt.startswith(plain["default"])
        pj = json.loads(plain["json"])
        assert all(js[n] == pj[n] for n in first)


def test_cli_input_formats_transfer_and_maps(tmp_path):
    """the four input formats (Y4M 8-bit, Y4M 10-bit, raw 8-bit, raw 10-bit), --itp-transfer, --itp-map against map()"""
    for bits in (8, 10):
        pairs = _pairs(bits)
        transfer = "hlg" if bits == 8 else "pq"
        rows, seq, maps = _binding(pairs, bits, transfer)
        d = tmp_path / str(bits)
        d.mkdir()
        for header in (True, False):
            a, b = _files(d, pairs, bits, header)
            extra = [] if header else ["--width", str(CW), "--height", str(CH), "--bits", str(bits)]
            prefix = str(d / ("y4m_map" if header else "raw_map"))
            lines = [json.loads(x) for x in _cli(a, b, "-m", "deitp", "--itp-transfer", transfer, "--itp-map", prefix, "--batch", "2", *extra,
                                                 "--output", "json-lines").splitlines() if x.strip()]
            assert [[x[n] for n in NAMES] for x in lines[:CN]] == rows and [lines[CN][n]["sequence"] for n in NAMES] == seq
            for i in range(CN):
                with open("%s%06d.pfm" % (prefix, i), "rb") as f:
                    assert f.readline() == b"Pf\n" and f.readline().split() == [str(CW).encode(), str(CH).encode()]
                    scale = float(f.readline())
                    data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").reshape(CH, CW)
                assert np.array_equal(data[::-1], maps[i]), (header, bits, i)  # PFM rows run bottom to top
            assert not os.path.exists("%s%06d.pfm" % (prefix, CN))
    # the default transfer is pq
    pairs = _pairs(10)
    a, b = _files(tmp_path, pairs, 10, True)
    assert _cli(a, b, "-m", "deitp", "--output", "csv") == _cli(a, b, "-m", "deitp", "--itp-transfer", "pq", "--output", "csv")


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
    out = subprocess.run([CLI, pa, pb, "-m", "deitp"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "deitp needs 4:2:0 YUV input" in out.stderr, (out.returncode, out.stderr)


# what the parent commit's binary printed for these arguments on the inputs of _parent_files(dir, kind): recorded once with
# record_parent_cli(<the parent's turbo-metrics>, GOLDEN, <a scratch directory>) on an MI355X, before the CLI was touched.  The option
# mixes of tests/golden/haarpsi_parent_cli.json, and one with the parent's newest column
PARENT_CASES = {
    "y4m8_psnr_ssim_default": ("y4m8", ["-m", "psnr", "-m", "ssim"]),
    "y4m8_ssimu_xpsnr_json": ("y4m8", ["-m", "ssimulacra2", "-m", "xpsnr", "--output", "json"]),
    "y4m8_psnr_yuv_motion_jsonl": ("y4m8", ["-m", "psnr", "-m", "psnr-yuv", "-m", "ssim-yuv", "--motion", "--output", "json-lines"]),
    "y4m10_vif_adm_scenes_csv": ("y4m10", ["-m", "vif", "-m", "adm", "--scenes", "--batch", "2", "--output", "csv"]),
    "y4m10_yuv_cambi_csv": ("y4m10", ["-m", "psnr-yuv", "-m", "cambi", "--output", "csv"]),
    "ppm_ssim_flip_jsonl": ("ppm", ["-m", "ssim", "-m", "flip", "--output", "json-lines"]),
    "y4m8_hvs_ciede_siti_default": ("y4m8", ["-m", "psnr-hvs", "-m", "ciede2000", "--siti"]),
    "y4m10_gmsd_haarpsi_psnr_default": ("y4m10", ["-m", "gmsd", "-m", "haarpsi", "-m", "psnr"]),
    "y4m10_ciede_haarpsi_csv": ("y4m10", ["-m", "ciede2000", "-m", "haarpsi", "--output", "csv"]),
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
        assert "deitp" not in got[name].lower(), name
