"""GPU tier of XPSNR (libturbometrics_xpsnr.so on the MI355X): rounded weighted SSE bit-identical with the CPU restatement
(tests/xpsnr_ref.py) and scores ==, on moving synthetic sequences; batch splits, reset, memory kinds and layouts give the same bits."""
import numpy as np
import pytest

from tests import xpsnr_ref as R
from tests import xpsnr_util as U
from tm_pkg import tm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _hip():
    tm.init_hip(0)


def _want(w, h, bits, fps, n, first=0):
    seq = R.Sequence(w, h, bits, fps)
    pics = [U.pictures(w, h, first + i, bits) for i in range(n)]
    return pics, [seq.push(r, d) for r, d in pics], seq


def _torch(p):
    """the same bytes as a torch tensor (signed views: torch has no unsigned 16- / 32-bit kernels to copy with)"""
    import torch
    return torch.from_numpy(p.view({np.uint16: np.int16, np.uint32: np.int32}.get(p.dtype.type, p.dtype)))


def _run(x, layout, w, h, bits, pics, batches, mem="host", pad=0):
    out, i = [], 0
    for n in batches:
        for s in range(n):
            ref, dis = pics[i + s]
            pr, pd = U.layout_planes(layout, ref, w, h, bits, pad), U.layout_planes(layout, dis, w, h, bits, pad)
            if mem == "device":
                pr, pd = [_torch(p).cuda() for p in pr], [_torch(p).cuda() for p in pd]
            elif mem == "pinned":
                pr, pd = [_torch(p).pin_memory() for p in pr], [_torch(p).pin_memory() for p in pd]
            x.set_pair(s, pr, pd)
        x.compute(n)
        out += x.frames(n)
        i += n
    return out


def _check(got, want):
    assert [f.wsse for f in got] == [wv[0] for wv in want]
    assert [f.xpsnr for f in got] == [wv[1] for wv in want]


@pytest.mark.parametrize("w,h,layout,bits,fps,batches", [
    (1920, 1080, "nv12", 8, (30, 1), [3, 1]),
    (1920, 1080, "nv12", 8, (60, 1), [1, 3]),
    (3840, 2160, "p016", 10, (25, 1), [2, 1]),
    (3840, 2160, "i420", 10, (50, 1), [2, 1]),
    (640, 480, "i420", 8, (25, 1), [3]),
    (1279, 719, "i420", 8, (60, 1), [2, 2]),
    (40, 40, "nv12", 8, (25, 1), [2, 1]),
    (1280, 720, "i420p10", 10, (25, 1), [2, 1]),   # chroma block width 22: groups of 4 start inside the block
    (854, 480, "i420p10", 10, (60, 1), [3]),       # chroma block width 14
    (1280, 720, "p016", 10, (25, 1), [3]),
])
def test_bit_identical_with_the_restatement(w, h, layout, bits, fps, batches):
    pics, want, _ = _want(w, h, bits, fps, sum(batches))
    with tm.Xpsnr(w, h, layout, bits, fps=fps, batch=max(batches)) as x:
        _check(_run(x, layout, w, h, bits, pics, batches), want)


def test_batch_splits_reset_memory_kinds_and_layouts_give_the_same_bits():
    w, h, bits, fps = 352, 288, 10, (60, 1)
    pics, want, _ = _want(w, h, bits, fps, 9)
    with tm.Xpsnr(w, h, "i420", bits, fps=fps, batch=9) as x:
        for batches in ([9], [4, 1, 4], [1] * 9):
            _check(_run(x, "i420", w, h, bits, pics, batches), want)
            x.reset()
        # without reset the history continues: the first frame then differs from a fresh sequence's
        _run(x, "i420", w, h, bits, pics, [2])
        again = _run(x, "i420", w, h, bits, pics, [1])
        assert again[0].wsse != want[0][0]
        x.reset()
        _check(_run(x, "i420", w, h, bits, pics, [9]), want)
        for mem in ("pinned", "device"):
            x.reset()
            _check(_run(x, "i420", w, h, bits, pics, [4, 5], mem=mem, pad=5), want)
    for layout in ("p016", "i420p10"):
        with tm.Xpsnr(w, h, layout, bits, fps=fps, batch=4) as x:
            _check(_run(x, layout, w, h, bits, pics, [4, 4, 1]), want)
            x.reset()
            _check(_run(x, layout, w, h, bits, pics, [3, 3, 3], mem="device"), want)


def test_nv12_layouts_and_memory_kinds_at_1080p():
    w, h, fps = 1920, 1080, (25, 1)
    pics, want, _ = _want(w, h, 8, fps, 3)
    for layout, mem in (("nv12", "host"), ("nv12", "device"), ("nv12", "pinned"), ("i420", "device")):
        with tm.Xpsnr(w, h, layout, 8, fps=fps, batch=3) as x:
            _check(_run(x, layout, w, h, 8, pics, [3], mem=mem), want)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------
import json  # noqa: E402
import math  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "turbo-metrics_amd", "bin", "turbo-metrics")


def _y4m(path, w, h, pics, side, fps=(25, 1)):
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{w} H{h} F{fps[0]}:{fps[1]} Ip A1:1 C420jpeg\n".encode())
        for p in pics:
            f.write(b"FRAME\n")
            for pl in p[side]:
                f.write(np.asarray(pl, np.uint8).tobytes())


def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)


def _json_lines(out):
    lines = [json.loads(line) for line in out.stdout.splitlines() if line.strip()]
    return [d for d in lines if "frame_count" not in d], [d for d in lines if "frame_count" in d]


@pytest.mark.parametrize("fps", [(25, 1), (60, 1)])
def test_cli_xpsnr_json_lines_match_the_restatement(tmp_path, fps):
    w, h, n = 320, 180, 7
    pics, want, seq = _want(w, h, 8, fps, n)
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    _y4m(a, w, h, pics, 0, fps)
    _y4m(b, w, h, pics, 1, fps)
    out = _cli(a, b, "-m", "xpsnr", "--output", "json-lines", "--batch", "3")
    assert out.returncode == 0, out.stderr
    frames, agg = _json_lines(out)
    assert len(frames) == n and len(agg) == 1 and agg[0]["frame_count"] == n
    for f, (_, sc) in zip(frames, want):
        assert sorted(f) == ["xpsnr_u", "xpsnr_v", "xpsnr_y"]
        for c, k in enumerate(("xpsnr_y", "xpsnr_u", "xpsnr_v")):
            assert f[k] == (None if math.isinf(sc[c]) else sc[c]), (f, sc)
    for c, k in enumerate(("xpsnr_y", "xpsnr_u", "xpsnr_v")):
        assert agg[0][k]["sequence"] == seq.sequence_scores()[c]
    # --xpsnr-fps overrides the Y4M rate (across 32: the temporal order changes)
    other = R.Sequence(w, h, 8, (60, 1) if fps == (25, 1) else (25, 1))
    ow = [other.push(r, d) for r, d in pics]
    out = _cli(a, b, "-m", "xpsnr", "--output", "json-lines", "--xpsnr-fps", "60" if fps == (25, 1) else "25/1")
    assert out.returncode == 0, out.stderr
    frames, _ = _json_lines(out)
    assert [f["xpsnr_y"] for f in frames] == [s[1][0] for s in ow]


def test_cli_xpsnr_beside_ssimulacra2_leaves_its_values_alone(tmp_path):
    w, h, n = 320, 180, 5
    pics, want, _ = _want(w, h, 8, (25, 1), n)
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    _y4m(a, w, h, pics, 0)
    _y4m(b, w, h, pics, 1)
    alone = _cli(a, b, "-m", "ssimulacra2", "--output", "json-lines", "--batch", "2")
    both = _cli(a, b, "-m", "xpsnr", "-m", "ssimulacra2", "--output", "json-lines", "--batch", "2")
    assert alone.returncode == 0 and both.returncode == 0, (alone.stderr, both.stderr)
    fa, ga = _json_lines(alone)
    fb, gb = _json_lines(both)
    assert len(fa) == len(fb) == n
    for x, y, (_, sc) in zip(fa, fb, want):
        # the ssimulacra2 field is the same text, and the XPSNR fields follow it
        assert json.dumps(x["ssimulacra2"]) == json.dumps(y["ssimulacra2"])
        assert y["xpsnr_y"] == sc[0]
    assert json.dumps(ga[0]["ssimulacra2"]) == json.dumps(gb[0]["ssimulacra2"])
    la = [ln for ln in alone.stdout.splitlines() if ln.strip()]
    lb = [ln for ln in both.stdout.splitlines() if ln.strip()]
    for x, y in zip(la[:-1], lb[:-1]):
        assert y.startswith(x[:-1] + ",\"xpsnr_y\":")  # the line alone, byte for byte, then the XPSNR fields


def test_cli_xpsnr_refuses_rgb_images(tmp_path):
    ppm = b"P6\n16 16\n255\n" + bytes(16 * 16 * 3)
    a, b = tmp_path / "a.ppm", tmp_path / "b.ppm"
    a.write_bytes(ppm)
    b.write_bytes(ppm)
    out = _cli(str(a), str(b), "-m", "xpsnr")
    assert out.returncode != 0 and "xpsnr" in out.stderr, (out.returncode, out.stderr)


# ---- content, dirty bytes, memory kinds and alignments, D = 16, b = 256, 130 slots, the fps boundary ------------------------------
from tests import xpsnr_twin as T  # noqa: E402


def _twin(w, h, bits, fps, pics):
    seq = T.Sequence(w, h, bits, fps)
    return [seq.push(r, d) for r, d in pics], seq


def _hand_over(planes, mem, vec):
    """numpy planes -> what set_pair gets.  device / pinned: torch copies; vec=False hands over views at a storage offset of one
    element (no longer 16-byte aligned: the kernels' per-sample loads).  Device copies carry garbage past every row (the planes come
    from layout_planes dirty= with padding) and the element before an offset view is garbage too."""
    import torch
    out = []
    for p in planes:
        t = _torch(np.ascontiguousarray(p))
        if not vec:
            flat = torch.full((t.numel() + 1,), 0x55, dtype=t.dtype)
            flat[1:] = t.reshape(-1)
            t = flat[1:].view(t.shape)
        if mem == "device":
            t = t.cuda() if vec else (lambda f: f[1:].view(t.shape))(flat.cuda())
        elif mem == "pinned":
            t = t.pin_memory() if vec else (lambda f: f[1:].view(t.shape))(flat.pin_memory())
        elif vec:
            t = np.ascontiguousarray(p)
        out.append(t)
    return out


def _run_dirty(x, layout, w, h, bits, pics, batches, mem, vec, pad):
    out, i = [], 0
    keep = []
    for n in batches:
        for s in range(n):
            sides = [_hand_over(U.layout_planes(layout, pics[i + s][side], w, h, bits, pad, dirty=U.dirt_seed(i + s, side)), mem, vec)
                     for side in (0, 1)]
            keep.append(sides)
            x.set_pair(s, *sides)
        x.compute(n)
        out += x.frames(n)
        i += n
    return out


@pytest.mark.parametrize("w,h,layout,bits,kind,pad", [
    (352, 288, "i420", 10, "random", 8),     # bits above D; pitch 720 bytes: 16-byte aligned rows with vec
    (352, 288, "p016", 12, "steps", 8),      # low bits of P016 words
    (352, 288, "nv12", 8, "stripes", 16),
    (390, 270, "i420p10", 10, "random", 4),  # packed bits 30-31, absent samples of the last run
    (256, 130, "i420", 16, "checker", 8),    # D = 16 full-scale checkerboard
    (256, 130, "p016", 16, "flat", 8),
    (176, 144, "i420", 12, "identical", 8),  # wsse 0: +inf
])
def test_dirty_bytes_content_memory_kinds_and_alignment(w, h, layout, bits, kind, pad):
    fps, batches = (60, 1), [2, 1]
    pics = [U.pictures(w, h, n, bits, kind) for n in range(3)]
    want, _ = _twin(w, h, bits, fps, pics)
    with tm.Xpsnr(w, h, layout, bits, fps=fps, batch=2) as x:
        for mem in ("host", "pinned", "device"):
            for vec in (True, False):
                x.reset()
                _check(_run_dirty(x, layout, w, h, bits, pics, batches, mem, vec, pad), want)


@pytest.mark.parametrize("w,h,layout,bits,kind", [
    (1920, 1080, "i420", 16, "random"),
    (3840, 2160, "p016", 16, "checker"),
    (7680, 4320, "p016", 10, "synth"),       # b = 256: the LDS tile exactly full
    (7680, 4320, "i420", 16, "random"),
])
def test_full_scale_and_the_largest_blocks(w, h, layout, bits, kind):
    fps = (60, 1)
    pics = [U.pictures(w, h, n, bits, kind) for n in range(2)]
    want, _ = _twin(w, h, bits, fps, pics)
    with tm.Xpsnr(w, h, layout, bits, fps=fps, batch=2) as x:
        _check(_run(x, layout, w, h, bits, pics, [2], mem="device"), want)


def test_known_answers_on_the_gpu():
    """the hand-derived answers of tests/test_xpsnr_cpu.py: checkerboard at bval 1 and 2, period-4 stripes at bval 2"""
    cases = [(480, 270, "nv12", 8, "checker", [(470016000, 117504000, 117504000), (528768000, 132192000, 132192000)])]
    aa = R.avg_act(2560, 1440, 8)
    for kind, ws in (("checker", [1 / 255, 1 / 4]), ("stripes", [1 / (9 * 255), 1 / (8 * 255)])):
        cases.append((2560, 1440, "nv12", 8, kind,
                      [tuple(int(n * 255 * 255 * wt * aa + 0.5) for n in (2560 * 1440, 1280 * 720, 1280 * 720)) for wt in ws]))
    for w, h, layout, bits, kind, want in cases:
        pics = [U.pictures(w, h, n, bits, kind) for n in range(2)]
        with tm.Xpsnr(w, h, layout, bits, fps=(25, 1), batch=2) as x:
            assert [f.wsse for f in _run(x, layout, w, h, bits, pics, [2], mem="device")] == want, (w, h, kind)


def test_130_slots_in_one_compute_and_in_splits():
    """k_xpsnr_finish on ceil(130 / 64) = 3 workgroups; 48 x 48 has b = 4 (weights, smoothing)"""
    w, h, bits, fps = 48, 48, 8, (60, 1)
    assert R.block_size(w, h) == 4
    pics = [U.pictures(w, h, n, bits, "random") for n in range(130)]
    want, _ = _twin(w, h, bits, fps, pics)
    with tm.Xpsnr(w, h, "nv12", bits, fps=fps, batch=130) as x:
        for batches in ([130], [65, 65], [128, 2]):
            x.reset()
            _check(_run(x, "nv12", w, h, bits, pics, batches), want)


@pytest.mark.parametrize("fps", [(32, 1), (63, 2)])
def test_the_temporal_order_at_its_boundary(fps):
    w, h, bits = 640, 360, 10
    pics, want, _ = _want(w, h, bits, fps, 3)
    assert R.second_order(*fps) == (fps == (32, 1))
    with tm.Xpsnr(w, h, "i420", bits, fps=fps, batch=3) as x:
        _check(_run(x, "i420", w, h, bits, pics, [3], mem="device"), want)


# ---- the CLI on 9..16-bit Y4M, headerless input, odd sizes, the read-ahead pool, partial batches, NTSC rates --------------------
def _y4m_hi(path, w, h, pics, side, bits, fps=(25, 1), header=True):
    """Y4M (C420p10 / p12 / p16, little-endian 16-bit words) or headerless planar frames"""
    with open(path, "wb") as f:
        if header:
            f.write(f"YUV4MPEG2 W{w} H{h} F{fps[0]}:{fps[1]} Ip A1:1 C420p{bits}\n".encode())
        for p in pics:
            if header:
                f.write(b"FRAME\n")
            for pl in p[side]:
                f.write(np.asarray(pl, "<u2" if bits > 8 else np.uint8).tobytes())


def _cli_scores(*args, env=None):
    out = subprocess.run([CLI, *args, "-m", "xpsnr", "--output", "json-lines"], capture_output=True, text=True, timeout=300,
                         env=None if env is None else {**os.environ, **env})
    assert out.returncode == 0, out.stderr
    frames, agg = _json_lines(out)
    return out, frames, agg


def _cli_check(frames, agg, want, seq):
    assert len(frames) == len(want) and agg[0]["frame_count"] == len(want)
    for f, (_, sc) in zip(frames, want):
        for c, k in enumerate(("xpsnr_y", "xpsnr_u", "xpsnr_v")):
            assert f[k] == (None if math.isinf(sc[c]) else sc[c]), (f, sc)
    for c, k in enumerate(("xpsnr_y", "xpsnr_u", "xpsnr_v")):
        assert agg[0][k]["sequence"] == seq.sequence_scores()[c]


@pytest.mark.parametrize("bits", [10, 12, 16])
def test_cli_high_bit_depth_y4m(tmp_path, bits):
    """10-bit goes through the packed ring (TM_XPSNR_I420P10_PACKED); TM_PACK10=0 hands 16-bit words over instead: same stdout"""
    w, h, n, fps = 330, 270, 5, (25, 1)
    pics = [U.pictures(w, h, i, bits, "random" if bits == 16 else "synth") for i in range(n)]
    want, seq = _twin(w, h, bits, fps, pics)
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    _y4m_hi(a, w, h, pics, 0, bits, fps)
    _y4m_hi(b, w, h, pics, 1, bits, fps)
    out, frames, agg = _cli_scores(a, b, "--batch", "2")
    _cli_check(frames, agg, want, seq)
    if bits == 10:
        again, _, _ = _cli_scores(a, b, "--batch", "2", env={"TM_PACK10": "0"})
        assert again.stdout == out.stdout


@pytest.mark.parametrize("batch", [1, 4])
def test_cli_headerless_odd_size_partial_batches(tmp_path, batch):
    w, h, n, bits = 161, 97, 7, 8
    pics = [U.pictures(w, h, i, bits, "steps") for i in range(n)]
    want, seq = _twin(w, h, bits, (25, 1), pics)
    a, b = str(tmp_path / "a.yuv"), str(tmp_path / "b.yuv")
    _y4m_hi(a, w, h, pics, 0, bits, header=False)
    _y4m_hi(b, w, h, pics, 1, bits, header=False)
    _, frames, agg = _cli_scores(a, b, "--width", str(w), "--height", str(h), "--bits", "8", "--batch", str(batch))
    _cli_check(frames, agg, want, seq)


@pytest.mark.parametrize("fps", [(60000, 1001), (30000, 1001)])
def test_cli_ntsc_rates_and_the_read_ahead_pool(tmp_path, fps):
    """F60000:1001 is second order, F30000:1001 first order; 640 x 360 (>= 256 rows) starts the read-ahead pool"""
    w, h, n = 640, 360, 6
    pics = [U.pictures(w, h, i, 8) for i in range(n)]
    want, seq = _twin(w, h, 8, fps, pics)
    assert seq.second == (fps == (60000, 1001))
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    _y4m(a, w, h, pics, 0, fps)
    _y4m(b, w, h, pics, 1, fps)
    _, frames, agg = _cli_scores(a, b, "--batch", "4")
    _cli_check(frames, agg, want, seq)
