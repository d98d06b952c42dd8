"""GPU tier of VMAF integer motion (libturbometrics_motion.so on the MI355X): sad bit-identical with the CPU restatement
(tests/motion_ref.py) and motion equal as doubles; memory kinds, pitches, dirty bytes, batch splits, the hand-derived answers, and
the CLI's --motion in every output format.  No tolerance anywhere: the arithmetic is integer up to sad."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import motion_ref as R
from tests import motion_util as U
from tm_pkg import tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")


@pytest.fixture(scope="module", autouse=True)
def _hip():
    tm.init_hip(0)


def _torch(p):
    """the same bytes as a torch tensor (signed views: torch has no unsigned 16- / 32-bit kernels to copy with)"""
    import torch
    return torch.from_numpy(p.view({np.uint16: np.int16, np.uint32: np.int32}.get(p.dtype.type, p.dtype)))


def _hand_over(p, mem, aligned):
    """plane array -> what set_frame gets: numpy (host), pinned or device torch tensors; aligned=False offsets the base by one
    element and keeps the odd pitch, so that the kernel's per-sample path runs"""
    if mem == "host":
        return p
    import torch
    rows, cols = p.shape
    pitch = (cols + 63) // 64 * 64 if aligned else cols + 1
    buf = torch.zeros(rows * pitch + 64, dtype=_torch(p[:1]).dtype)
    off = 0 if aligned else 1
    view = buf[off:off + rows * pitch].view(rows, pitch)[:, :cols]
    view.copy_(_torch(np.ascontiguousarray(p)))
    if mem == "pinned":
        buf = buf.pin_memory()
    else:
        buf = buf.cuda()
    return buf[off:off + rows * pitch].view(rows, pitch)[:, :cols]


def _run(m, layout, bits, seq, batches, mem="host", aligned=True, pad=0, dirty=True):
    got, i = [], 0
    for b in batches:
        if b < 0:
            m.reset()
            b = -b
        keep = [_hand_over(U.luma_plane(layout, seq[i + s], bits, pad=pad, dirty=(i + s if dirty else None)), mem, aligned) for s in range(b)]
        for s, p in enumerate(keep):
            m.set_frame(s, p)
        m.compute(b)
        got += [tuple(f) for f in m.frames(b)]
        i += b
    return got


@pytest.mark.parametrize("w,h,layout,bits,n", [
    (1920, 1080, "y8", 8, 3), (3840, 2160, "y16_msb", 10, 3), (1920, 1080, "y10_packed", 10, 3), (1280, 720, "y16_low", 12, 3),
    (1280, 720, "y16_low", 16, 3), (7680, 4320, "y8", 8, 2), (333, 177, "y16_msb", 12, 4), (3, 3, "y8", 8, 4), (3, 3, "y10_packed", 10, 4)])
def test_bit_identical_with_the_restatement(w, h, layout, bits, n):
    seq = U.sequence(w, h, n, bits, "random" if w * h < 4000000 else "smooth")
    want = R.sequence(seq, bits)
    with tm.Motion(w, h, layout, bits, batch=n) as m:
        assert _run(m, layout, bits, seq, [1, n - 1], pad=3) == want
        assert m.mem_usage() > 0


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_memory_kinds_pitches_and_dirty_bytes(layout, bits):
    w, h = 250, 37
    seq = U.sequence(w, h, 5, bits, "extreme" if bits == 16 else "random")
    want = R.sequence(seq, bits)
    with tm.Motion(w, h, layout, bits, batch=5) as m:
        for mem, aligned in (("host", True), ("pinned", True), ("pinned", False), ("device", True), ("device", False)):
            m.reset()
            assert _run(m, layout, bits, seq, [2, 3], mem, aligned, pad=0 if mem != "host" else 7) == want, (mem, aligned)


def test_batch_splits_of_130_slots_and_reset():
    w, h, bits = 160, 50, 10
    seq = U.sequence(w, h, 130, bits, "smooth")
    want = R.sequence(seq, bits)
    with tm.Motion(w, h, "y16_msb", bits, batch=130) as m:
        assert _run(m, "y16_msb", bits, seq, [130], "device") == want
        m.reset()
        assert _run(m, "y16_msb", bits, seq, [1, 64, 2, 50, 13], "device") == want
        assert _run(m, "y16_msb", bits, seq[:7], [-3, 4]) == want[:7]
        # a slot that was not set again is an error, not a stale picture
        with pytest.raises(tm.motion.MotionError) as e:
            m.compute(1)
        assert e.value.code == tm.ffi.TM_ERR_STATE


def test_known_answers_on_the_gpu():
    for bits in (8, 10, 16):
        w, h = 37, 23
        a, b = np.full((h, w), 5 << (bits - 8), np.int64), np.full((h, w), 9 << (bits - 8), np.int64)
        lay = "y8" if bits == 8 else "y16_msb"
        with tm.Motion(w, h, lay, bits, batch=2) as m:
            assert _run(m, lay, bits, [a, b], [2]) == [(0, 0.0), (871424, 4.0)]
    s = np.where(np.indices((48, 64))[1] % 2 == 1, 255, 0).astype(np.int64)
    with tm.Motion(64, 48, "y8", 8, batch=2) as m:
        assert _run(m, "y8", 8, [s, 255 - s], [1, 1]) == [(0, 0.0), (6036000, 7.6751708984375)]
    p = np.zeros((40, 41), np.int64)
    p[20, 19] = 255
    with tm.Motion(41, 40, "y8", 8, batch=2) as m:
        assert _run(m, "y8", 8, [0 * p, p], [2]) == [(0, 0.0), (65282, R.from_sad(65282, 41, 40))]
    f = np.full((9, 11), 65535, np.int64)
    with tm.Motion(11, 9, "y16_low", 16, batch=2) as m:
        assert [g[0] for g in _run(m, "y16_low", 16, [0 * f, f], [2])] == [0, 65535 * 99]


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def _y4m(path, w, h, lumas, bits, seed):
    rng = np.random.default_rng(seed)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    dt = np.uint8 if bits == 8 else "<u2"
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C420{'jpeg' if bits == 8 else 'p%d' % bits}\n".encode())
        for y in lumas:
            f.write(b"FRAME\n" + np.asarray(y, dt).tobytes())
            for _ in range(2):
                f.write(rng.integers(0, 1 << bits, (ch, cw)).astype(dt).tobytes())


def _cli(*args, env=None):
    out = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300, env=None if env is None else {**os.environ, **env})
    assert out.returncode == 0, out.stderr
    return out.stdout


def _files(tmp_path, w, h, n, bits):
    seq = U.sequence(w, h, n, bits, "smooth")
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    _y4m(a, w, h, seq, bits, 1)
    _y4m(b, w, h, [(p + 1) % (1 << bits) for p in seq], bits, 2)
    mo = [f[1] for f in R.sequence(seq, bits)]
    return a, b, mo, R.motion2(mo)


@pytest.mark.parametrize("bits,env,batch", [(8, None, "3"), (10, None, "4"), (10, {"TM_PACK10": "0"}, "7"), (12, None, "2")])
def test_cli_motion_in_every_output_format(tmp_path, bits, env, batch):
    w, h, n = 322, 182, 7  # 7 pictures in batches of 3 / 4 / 2: a partial last batch; 7: exactly one
    a, b, mo, mo2 = _files(tmp_path, w, h, n, bits)
    base = (a, b, "--motion", "--batch", batch)
    lines = [json.loads(x) for x in _cli(*base, "--output", "json-lines", env=env).splitlines() if x.strip()]
    frames, agg = [d for d in lines if "frame_count" not in d], [d for d in lines if "frame_count" in d][0]
    assert [f["motion"] for f in frames] == mo and [f["motion2"] for f in frames] == mo2
    assert all(set(f) == {"motion", "motion2"} for f in frames)
    assert agg["frame_count"] == n and agg["motion"]["min"] == 0.0 and agg["motion"]["max"] == max(mo) and agg["motion2"]["max"] == max(mo2)
    js = json.loads(_cli(*base, "--output", "json", env=env))
    assert js["motion"]["scores"] == mo and js["motion2"]["scores"] == mo2 and js["frame_count"] == n
    assert js["motion"]["stats"]["mean"] == agg["motion"]["mean"] and js["motion2"]["stats"]["mean"] == agg["motion2"]["mean"]
    rows = _cli(*base, "--output", "csv", env=env).splitlines()
    assert rows[0] == "motion,motion2" and len(rows) >= 1 + n
    assert [tuple(float(v) for v in r.split(",")) for r in rows[1:1 + n]] == list(zip(mo, mo2))
    txt = _cli(*base, env=env)
    assert "MOTION: Stats {" in txt and "MOTION2: Stats {" in txt


def test_cli_one_frame_file(tmp_path):
    a, b, mo, mo2 = _files(tmp_path, 64, 48, 1, 8)
    lines = [json.loads(x) for x in _cli(a, b, "--motion", "--output", "json-lines").splitlines() if x.strip()]
    assert lines[0] == {"motion": 0.0, "motion2": 0.0} and lines[1]["frame_count"] == 1


@pytest.mark.parametrize("sel", [["-m", "psnr", "-m", "ssimulacra2"], ["-m", "xpsnr", "-m", "psnr"]])
def test_cli_motion_leaves_the_other_columns_alone(tmp_path, sel):
    a, b, mo, mo2 = _files(tmp_path, 320, 180, 6, 8)
    for fmt in ("json-lines", "csv"):
        plain = _cli(a, b, *sel, "--batch", "4", "--output", fmt).splitlines()
        with_m = _cli(a, b, *sel, "--motion", "--batch", "4", "--output", fmt).splitlines()
        assert len(plain) == len(with_m)
        if fmt == "csv":
            ncol = len(plain[0].split(","))
            assert [r.split(",")[:ncol] for r in with_m] == [r.split(",") for r in plain]
            assert with_m[0].split(",")[ncol:] == ["motion", "motion2"]
            assert [tuple(float(v) for v in r.split(",")[ncol:]) for r in with_m[1:7]] == list(zip(mo, mo2))
        else:
            for p, q in zip(plain, with_m):
                p, q = json.loads(p), json.loads(q)
                assert {k: v for k, v in q.items() if not k.startswith("motion")} == p
                assert list(q)[:len(p)] == list(p)  # motion / motion2 come after every other column
            assert [json.loads(q)["motion2"] for q in with_m[:6]] == mo2
    # without --motion every output is what the parent printed: no motion key anywhere
    assert "motion" not in _cli(a, b, *sel, "--output", "json")


def test_cli_motion_refuses_rgb_images(tmp_path):
    a = str(tmp_path / "a.ppm")
    with open(a, "wb") as f:
        f.write(b"P6\n16 16\n255\n" + bytes(16 * 16 * 3))
    out = subprocess.run([CLI, a, a, "--motion"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "motion" in out.stderr, (out.returncode, out.stderr)
