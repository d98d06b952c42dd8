"""GPU tier of P.910 SI / TI (libturbometrics_siti.so on the MI355X): every sum bit-identical with the integer restatement
(tests/siti_ref.py), si / ti equal as doubles with the library's host functions; layouts, edge sizes, pitches, dirty bits, unaligned
bases, memory kinds, batch splits, reset, repeatability, the state rules of the feature libraries, the binding with torch device
tensors, and the CLI's --siti in every output format.  No tolerance anywhere: what the device produces is integer."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import siti_ref as R
from tests import siti_util as U
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
    buf = buf.pin_memory() if mem == "pinned" else buf.cuda()
    return buf[off:off + rows * pitch].view(rows, pitch)[:, :cols]


def _run(m, layout, bits, seq, batches, mem="host", aligned=True, pad=0, dirty=True):
    """-> [(s1, s2, t1, t2, ti_valid)], after checking si / ti of every frame against the restatement's doubles"""
    got, i = [], 0
    for b in batches:
        if b < 0:
            m.reset()
            b = -b
        keep = [_hand_over(U.luma_plane(layout, seq[i + s], bits, pad=pad, dirty=(i + s if dirty else None)), mem, aligned) for s in range(b)]
        for s, p in enumerate(keep):
            m.set_frame(s, p)
        m.compute(b)
        for f in m.frames(b):
            n_si, n = (m.w - 2) * (m.h - 2), m.w * m.h
            assert f.si == R.si(f.s1, f.s2, n_si) and f.ti == (R.ti(f.t1, f.t2, n, bits) if f.ti_valid else 0.0)
            got.append(tuple(f[:5]))
        i += b
    return got


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_edge_sizes_bit_identical_with_the_restatement(layout, bits):
    sizes = U.edge_sizes() + ([(w, 5) for w in U.P10_WIDTHS] if layout == "y10_packed" else [])
    for w, h in sizes:
        seq = U.sequence(w, h, 4, bits, ("random", "extreme", "smooth")[(w + h) % 3])
        want = R.sums(seq, bits)
        with tm.Siti(w, h, layout, bits, batch=4) as m:
            assert _run(m, layout, bits, seq, [1, 3], pad=5) == want, (w, h)
            assert _run(m, layout, bits, seq, [-4], "device", aligned=False) == want, (w, h, "unaligned")
            assert m.mem_usage() > 0


@pytest.mark.parametrize("layout,bits", U.ONE_PER_LAYOUT)
def test_memory_kinds_pitches_and_dirty_bits(layout, bits):
    w, h = 250, 37
    seq = U.sequence(w, h, 5, bits, "random")
    want = R.sums(seq, bits)
    with tm.Siti(w, h, layout, bits, batch=5) as m:
        for mem, aligned in (("host", True), ("pinned", True), ("pinned", False), ("device", True), ("device", False)):
            m.reset()
            assert _run(m, layout, bits, seq, [2, 3], mem, aligned, pad=0 if mem != "host" else 7) == want, (mem, aligned)


def test_batch_splits_and_reset_give_identical_frames():
    w, h, bits = 133, 41, 10
    seq = U.sequence(w, h, 4, bits, "random")
    want = R.sums(seq, bits)
    with tm.Siti(w, h, "y16_msb", bits, batch=4) as m:
        for split in ([1, 1, 1, 1], [4], [3, 1]):
            m.reset()
            assert _run(m, "y16_msb", bits, seq, split, "device") == want, split
        again = R.sums(seq[2:], bits)
        assert again[0][2:] == (0, 0, 0) and _run(m, "y16_msb", bits, seq, [-2, -2]) == want[:2] + again
        # a slot that was not set again is an error, not a stale picture
        with pytest.raises(tm.siti.SitiError) as e:
            m.compute(1)
        assert e.value.code == tm.ffi.TM_ERR_STATE


def test_twenty_repeats_are_bit_identical():
    w, h, bits = 500, 130, 8
    seq = U.sequence(w, h, 3, bits, "random")
    want = R.sums(seq, bits)
    planes = [_hand_over(U.luma_plane("y8", p, bits), "device", True) for p in seq]
    with tm.Siti(w, h, "y8", bits, batch=3) as m:
        for _ in range(20):
            m.reset()
            for s, p in enumerate(planes):
                m.set_frame(s, p)
            m.compute(3)
            assert [tuple(f[:5]) for f in m.frames(3)] == want


def test_known_answers_on_the_gpu():
    p = np.zeros((40, 41), np.int64)
    p[20, 19] = 255
    with tm.Siti(41, 40, "y8", 8, batch=2) as m:
        assert _run(m, "y8", 8, [0 * p, p], [2]) == [(0, 0, 0, 0, 0), (891520, 102275584000, 255, 65025, 1)]
    y, x = np.indices((33, 47))
    with tm.Siti(47, 33, "y8", 8, batch=1) as m:
        (s1, s2, *_), = _run(m, "y8", 8, [x + y], [1])
        assert (s1, s2) == (2896 * 45 * 31, 2896 * 2896 * 45 * 31) and m.frames(1)[0].si == 0.0
    c = ((x + y) % 2) * 65535
    with tm.Siti(47, 33, "y16_low", 16, batch=2) as m:
        assert _run(m, "y16_low", 16, [c, 65535 - c], [2]) == [(0, 0, 0, 0, 0), (0, 0, 65535 * (776 - 775), 65535 ** 2 * 47 * 33, 1)]


# ---- the state rules of the feature libraries (tests/test_gpu_feature_state.py holds the other ten to them) --------------------
def test_state_rules():
    L = tm.siti.lib()
    w, h = 1920, 1080
    import torch
    y = torch.zeros((h, w), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    hnd = C.c_void_p()
    assert L.tm_siti_create(C.byref(hnd), w, h, 0, 8, 64) == tm.ffi.TM_OK
    try:
        out = (tm.siti.SitiFrameC * 64)()
        assert L.tm_siti_compute_async(hnd, 1) == tm.ffi.TM_ERR_STATE      # compute without set
        assert L.tm_siti_get(hnd, 0, 1, out) == tm.ffi.TM_ERR_STATE          # nothing computed yet
        assert L.tm_siti_compute_async(hnd, 0) == tm.ffi.TM_ERR_INVALID_ARG
        assert L.tm_siti_compute_async(hnd, 65) == tm.ffi.TM_ERR_INVALID_ARG
        for s in range(64):
            assert L.tm_siti_set_frame(hnd, s, y.data_ptr(), w, tm.ffi.TM_MEM_DEVICE) == tm.ffi.TM_OK
        assert L.tm_siti_set_frame(hnd, 64, y.data_ptr(), w, tm.ffi.TM_MEM_DEVICE) == tm.ffi.TM_ERR_INVALID_ARG
        assert L.tm_siti_set_frame(hnd, 0, y.data_ptr(), w - 1, tm.ffi.TM_MEM_DEVICE) == tm.ffi.TM_ERR_INVALID_ARG
        assert L.tm_siti_compute_async(hnd, 64) == tm.ffi.TM_OK
        assert L.tm_siti_compute_async(hnd, 64) == tm.ffi.TM_ERR_STATE       # a second compute (in flight, or once done: slots not set again; the in-flight rule alone: tests/host/siti_host_test.cpp)
        assert L.tm_siti_get(hnd, 0, 64, out) == tm.ffi.TM_OK                 # get synchronises
        assert all((f.s1, f.s2, f.t1, f.t2) == (0, 0, 0, 0) for f in out) and [f.ti_valid for f in out] == [0] + [1] * 63
        assert L.tm_siti_get(hnd, 60, 5, out) == tm.ffi.TM_ERR_STATE          # beyond the last compute
        assert L.tm_siti_sync(hnd) == tm.ffi.TM_OK and L.tm_siti_reset(hnd) == tm.ffi.TM_OK
    finally:
        L.tm_siti_destroy(hnd)


def test_binding_with_torch_device_tensors():
    import torch
    w, h, bits = 200, 64, 12
    seq = U.sequence(w, h, 3, bits, "smooth")
    want = R.sequence(seq, bits)
    dev = [torch.from_numpy(p.astype(np.int16)).cuda() for p in seq]  # y16_low: the value in the low bits
    torch.cuda.synchronize()
    with tm.Siti(w, h, "y16_low", bits, batch=3) as m:
        for s, t in enumerate(dev):
            m.set_frame(s, t)
        m.compute(3)
        got = m.frames(3)
    assert [f._asdict() for f in got] == want
    assert max(f.si for f in got) == R.sequence_scores(want)[0] and max(f.ti for f in got[1:]) == R.sequence_scores(want)[1]


@pytest.mark.parametrize("w,h,layout,bits", [(1920, 1080, "y8", 8), (3840, 2160, "y10_packed", 10)])
def test_large_pictures(w, h, layout, bits):
    seq = U.sequence(w, h, 2, bits, "random")
    with tm.Siti(w, h, layout, bits, batch=2) as m:
        assert _run(m, layout, bits, seq, [2], dirty=False) == R.sums(seq, bits)


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def _cli(*args, env=None):
    out = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300, env=None if env is None else {**os.environ, **env})
    assert out.returncode == 0, out.stderr
    return out.stdout


def _files(tmp_path, w, h, n, bits):
    seq = U.sequence(w, h, n, bits, "smooth")
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    U.y4m(a, seq, bits)
    U.y4m(b, [(p + 1) % (1 << bits) for p in seq], bits)
    return a, b, R.sequence(seq, bits)


@pytest.mark.parametrize("bits,batch", [(8, "3"), (10, "4")])
def test_cli_siti_in_every_output_format(tmp_path, bits, batch):
    w, h, n = 322, 182, 7
    a, b, fr = _files(tmp_path, w, h, n, bits)
    si, ti = [f["si"] for f in fr], [f["ti"] for f in fr]
    seq_si, seq_ti = R.sequence_scores(fr)
    assert ti[0] == 0.0 and seq_ti == max(ti[1:]) > 0
    base = (a, b, "--siti", "--batch", batch)
    lines = [json.loads(x) for x in _cli(*base, "--output", "json-lines").splitlines() if x.strip()]
    frames, agg = [d for d in lines if "frame_count" not in d], [d for d in lines if "frame_count" in d][0]
    assert [f["si"] for f in frames] == si and [f["ti"] for f in frames] == ti and all(list(f) == ["si", "ti"] for f in frames)
    assert agg["frame_count"] == n and agg["si"]["sequence"] == seq_si == agg["si"]["max"] and agg["ti"]["sequence"] == seq_ti
    assert agg["ti"]["min"] == min(ti[1:]) and agg["ti"]["mean"] == pytest.approx(np.mean(ti[1:]), rel=1e-14)  # the first picture is left out
    js = json.loads(_cli(*base, "--output", "json"))
    assert js["si"]["scores"] == si and js["ti"]["scores"] == ti and js["si"]["sequence"] == seq_si and js["ti"]["sequence"] == seq_ti
    rows = _cli(*base, "--output", "csv").splitlines()
    assert rows[0] == "si,ti" and [tuple(float(v) for v in r.split(",")) for r in rows[1:1 + n]] == list(zip(si, ti))
    assert rows[1 + n:] == rows[:1 + n]  # the end-of-stream table repeats the rows
    txt = _cli(*base)
    assert "SI: Stats {" in txt and "TI: Stats {" in txt and "SI / TI (sequence): si " in txt
    # gain: --siti-range limited is 255 / 219 on both
    g = [json.loads(x) for x in _cli(*base, "--siti-range", "limited", "--output", "json-lines").splitlines() if x.strip()][:n]
    assert [f["si"] for f in g] == [tm.siti.si(f["s1"], f["s2"], (w - 2) * (h - 2), 255 / 219) for f in fr]
    assert [f["ti"] for f in g[1:]] == [tm.siti.ti(f["t1"], f["t2"], w * h, bits, 255 / 219) for f in fr[1:]]
    g2 = [json.loads(x) for x in _cli(*base, "--siti-gain", "2", "--output", "json-lines").splitlines() if x.strip()][:n]
    assert [f["si"] for f in g2] == [2 * v for v in si]


def test_cli_one_frame_file(tmp_path):
    a, b, fr = _files(tmp_path, 64, 48, 1, 8)
    lines = [json.loads(x) for x in _cli(a, b, "--siti", "--output", "json-lines").splitlines() if x.strip()]
    assert lines[0] == {"si": fr[0]["si"], "ti": 0.0} and lines[1]["frame_count"] == 1 and lines[1]["ti"]["sequence"] == 0.0 and lines[1]["ti"]["max"] == 0.0


def test_cli_siti_leaves_the_other_columns_alone(tmp_path):
    a, b, fr = _files(tmp_path, 320, 180, 6, 8)
    sel = ["-m", "psnr", "--motion", "--scenes"]
    for fmt in ("json-lines", "csv"):
        plain = _cli(a, b, *sel, "--batch", "4", "--output", fmt).splitlines()
        with_s = _cli(a, b, *sel, "--siti", "--batch", "4", "--output", fmt).splitlines()
        assert len(plain) == len(with_s)
        if fmt == "csv":
            ncol = len(plain[0].split(","))
            assert [r.split(",")[:ncol] for r in with_s] == [r.split(",") for r in plain]
            assert with_s[0].split(",")[ncol:] == ["si", "ti"]
            assert [tuple(float(v) for v in r.split(",")[ncol:]) for r in with_s[1:7]] == [(f["si"], f["ti"]) for f in fr]
        else:
            for p, q in zip(plain, with_s):
                p, q = json.loads(p), json.loads(q)
                assert {k: v for k, v in q.items() if k not in ("si", "ti")} == p
                assert list(q)[:len(p)] == list(p) and list(q)[len(p):] == ["si", "ti"]
    assert '"si"' not in _cli(a, b, *sel, "--output", "json")


def test_cli_siti_refuses_rgb_images(tmp_path):
    a = str(tmp_path / "a.ppm")
    with open(a, "wb") as f:
        f.write(b"P6\n16 16\n255\n" + bytes(16 * 16 * 3))
    out = subprocess.run([CLI, a, a, "--siti"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "siti" in out.stderr, (out.returncode, out.stderr)


def test_cli_refusals(tmp_path):
    a, b, _ = _files(tmp_path, 16, 16, 1, 8)
    for extra in (["--every", "2"], ["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
        out = subprocess.run([CLI, a, b, "--siti", *extra], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "--siti does not run with" in out.stderr, (extra, out.returncode, out.stderr)
