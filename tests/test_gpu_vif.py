"""GPU tier of VMAF's VIF (libturbometrics_vif.so on the MI355X): num / den of every scale against the CPU restatement
(tests/vif_ref.py) within 1e-9 (flat pictures exactly); memory kinds, pitches and dirty bytes; batches with distinct pairs per slot;
the same batch twice is bit-identical; a slot not set again is TM_ERR_STATE; the CLI's -m vif alone and beside -m psnr."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import vif_ref as R
from tests import vif_util as U
from tests.test_gpu_motion import _hand_over, _y4m
from tm_pkg import tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
RTOL = 1e-9  # derived in tests/test_vif_cpu.py: log2 and the order of adding at most 2^23 non-negative terms
SEEN = {"rel": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _hip():
    tm.init_hip(0)


def _close(got, want, what):
    """got: VifFrame; want: vif_ref.vif's list"""
    for s in range(4):
        for k, g in (("num", got.num[s]), ("den", got.den[s])):
            w = want[s][k]
            rel = abs(g - w) / max(abs(w), 1e-300) if g != w else 0.0
            SEEN["rel"] = max(SEEN["rel"], rel)
            print(f"{what} scale {s} {k}: gpu {g!r} restatement {w!r} rel {rel:.3e}")
            assert rel <= RTOL, (what, s, k, g, w)
    sc = R.scores(want)
    assert all(abs(a - b) <= 2e-9 for a, b in zip(list(got.scales) + [got.vif], sc))


def _set(v, slot, layout, bits, ref, dis, mem="host", aligned=True, pad=0, dirty=None):
    planes = [_hand_over(U.luma_plane(layout, p, bits, pad=pad, dirty=None if dirty is None else dirty + i), mem, aligned) for i, p in enumerate((ref, dis))]
    v.set_pair(slot, *planes)
    return planes


def _one_pair(layout, bits, w, h, kind):
    ref, dis = U.pair(w, h, bits, kind)
    with tm.Vif(w, h, layout, bits, batch=1) as v:
        keep = _set(v, 0, layout, bits, ref, dis, pad=3, dirty=5)
        v.compute(1)
        _close(v.frames(1)[0], R.vif(ref, dis, bits), f"{layout} {bits} {w}x{h} {kind}")
        assert v.mem_usage() > 0 and keep


@pytest.mark.parametrize("w,h", [(32, 32), (33, 47), (75, 35), (100, 40)])
@pytest.mark.parametrize("layout,bits", U.CASES)
def test_matches_the_restatement(layout, bits, w, h):
    _one_pair(layout, bits, w, h, U.CONTENTS[(U.CASES.index((layout, bits)) + w) % len(U.CONTENTS)])


@pytest.mark.parametrize("layout,bits,w,h", [("y8", 8, 1920, 1080), ("y16_msb", 10, 1920, 1080), ("y10_packed", 10, 1280, 720), ("y16_low", 16, 1280, 720)])
def test_matches_the_restatement_at_full_size(layout, bits, w, h):
    _one_pair(layout, bits, w, h, "blurred")


@pytest.mark.parametrize("kind", U.CONTENTS)
def test_every_content(kind):
    w, h = 200, 90
    for layout, bits in (("y8", 8), ("y16_msb", 16)):
        ref, dis = U.pair(w, h, bits, kind, seed=3)
        with tm.Vif(w, h, layout, bits, batch=1) as v:
            _set(v, 0, layout, bits, ref, dis)
            v.compute(1)
            _close(v.frames(1)[0], R.vif(ref, dis, bits), f"{layout} {bits} {kind}")


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_flat_pictures_are_exactly_one(layout, bits):
    w, h = 53, 37
    M = (1 << bits) - 1
    with tm.Vif(w, h, layout, bits, batch=1) as v:
        for lr, ld in ((1, 1), (M, M), (0, M), (M // 3, M // 2 + 1)):
            _set(v, 0, layout, bits, np.full((h, w), lr, np.int64), np.full((h, w), ld, np.int64), pad=2, dirty=3)
            v.compute(1)
            f = v.frames(1)[0]
            assert list(f.num) == list(f.den) == [float(a * b) for a, b in R.sizes(w, h)], (lr, ld, f)
            assert list(f.scales) == [1.0] * 4 and f.vif == 1.0


@pytest.mark.parametrize("layout,bits", [("y8", 8), ("y16_msb", 10), ("y16_low", 12), ("y10_packed", 10)])
def test_memory_kinds_pitches_and_dirty_bytes(layout, bits):
    w, h = 250, 37
    ref, dis = U.pair(w, h, bits, "blurred", seed=9)
    want = R.vif(ref, dis, bits)
    with tm.Vif(w, h, layout, bits, batch=2) as v:
        seen = []
        for mem, aligned in (("host", True), ("pinned", True), ("pinned", False), ("device", True), ("device", False)):
            keep = _set(v, 0, layout, bits, ref, dis, mem, aligned, pad=0 if mem != "host" else 7, dirty=21)
            v.compute(1)
            f = v.frames(1)[0]
            _close(f, want, f"{layout} {mem} {aligned}")
            seen.append((f.num, f.den))
            del keep
        assert all(s == seen[0] for s in seen)  # the same samples: the same bits, whatever the memory kind, pitch or dirty bytes


def test_batches_with_distinct_pairs_per_slot_twice_and_the_state_rule():
    w, h, bits, cap = 96, 64, 10, 5
    pairs = [U.pair(w, h, bits, U.CONTENTS[i % len(U.CONTENTS)], seed=i) for i in range(cap)]
    want = [R.vif(r, d, bits) for r, d in pairs]
    with tm.Vif(w, h, "y16_msb", bits, batch=cap) as v:
        for n in (1, 3, cap):
            runs = []
            for _ in range(2):
                keep = [_set(v, i, "y16_msb", bits, *pairs[i], mem="device") for i in range(n)]
                v.compute(n)
                fr = v.frames(n)
                for i in range(n):
                    _close(fr[i], want[i], f"batch {n} slot {i}")  # slot i holds pair i's answer
                runs.append([(f.num, f.den) for f in fr])
                del keep
            assert runs[0] == runs[1]  # no floating-point atomics: bit-identical
        # a slot that was not set again is an error, not a stale pair
        with pytest.raises(tm.vif.VifError) as e:
            v.compute(1)
        assert e.value.code == tm.ffi.TM_ERR_STATE
        _set(v, 0, "y16_msb", bits, *pairs[0])
        with pytest.raises(tm.vif.VifError) as e:
            v.compute(2)
        assert e.value.code == tm.ffi.TM_ERR_STATE


def test_largest_difference_seen():
    print(f"largest relative difference of num / den, GPU vs restatement: {SEEN['rel']:.3e}")
    assert SEEN["rel"] <= RTOL


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def _cli(*args, env=None):
    out = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300, env=None if env is None else {**os.environ, **env})
    assert out.returncode == 0, out.stderr
    return out.stdout


def _files(tmp_path, w, h, n, bits):
    pairs = [U.pair(w, h, bits, "blurred", seed=i) for i in range(n)]
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    _y4m(a, w, h, [p[0] for p in pairs], bits, 1)
    _y4m(b, w, h, [p[1] for p in pairs], bits, 2)
    return a, b, [R.scores(R.vif(r, d, bits)) for r, d in pairs]


NAMES = ["vif_scale0", "vif_scale1", "vif_scale2", "vif_scale3", "vif"]


def _near(got, want):
    """to the printed digits: the shortest round-trip text of a double that is within 1e-9 (relative) of the restatement's"""
    return all(abs(g - w) <= 2e-9 * max(abs(w), 1.0) for g, w in zip(got, want))


@pytest.mark.parametrize("bits,batch", [(8, "3"), (10, "4"), (12, "7")])
def test_cli_vif_alone_in_every_output_format(tmp_path, bits, batch):
    w, h, n = 322, 182, 7
    a, b, want = _files(tmp_path, w, h, n, bits)
    base = (a, b, "-m", "vif", "--batch", batch)
    lines = [json.loads(x) for x in _cli(*base, "--output", "json-lines").splitlines() if x.strip()]
    frames, agg = [d for d in lines if "frame_count" not in d], [d for d in lines if "frame_count" in d][0]
    assert len(frames) == n and all(list(f) == NAMES for f in frames)
    assert all(_near([f[k] for k in NAMES], wv) for f, wv in zip(frames, want))
    assert agg["frame_count"] == n and list(agg) == ["frame_count"] + NAMES
    assert _near([agg[k]["mean"] for k in NAMES], [float(np.mean([wv[i] for wv in want])) for i in range(5)])
    js = json.loads(_cli(*base, "--output", "json"))
    assert [js[k]["scores"] for k in NAMES] == [[f[k] for f in frames] for k in NAMES] and js["frame_count"] == n
    rows = _cli(*base, "--output", "csv").splitlines()
    assert rows[0] == ",".join(NAMES) and len(rows) >= 1 + n
    assert [[float(v) for v in r.split(",")] for r in rows[1:1 + n]] == [[f[k] for k in NAMES] for f in frames]
    txt = _cli(*base)
    assert "VIF_SCALE0: Stats {" in txt and "VIF: Stats {" in txt
    # --every keeps every second pair: VIF has no history
    ev = [json.loads(x) for x in _cli(*base, "--every", "2", "--output", "json-lines").splitlines() if x.strip()]
    assert [f for f in ev if "frame_count" not in f] == frames[::2]


def test_cli_vif_beside_psnr_leaves_the_other_columns_alone(tmp_path):
    a, b, want = _files(tmp_path, 320, 180, 6, 8)
    for fmt in ("json-lines", "csv"):
        plain = _cli(a, b, "-m", "psnr", "--batch", "4", "--output", fmt).splitlines()
        with_v = _cli(a, b, "-m", "psnr", "-m", "vif", "--batch", "4", "--output", fmt).splitlines()
        assert len(plain) == len(with_v)
        if fmt == "csv":
            assert [r.split(",")[:1] for r in with_v] == [r.split(",") for r in plain]
            assert with_v[0].split(",")[1:] == NAMES
            assert all(_near([float(x) for x in r.split(",")[1:]], wv) for r, wv in zip(with_v[1:7], want))
        else:
            for p, q in zip(plain, with_v):
                p, q = json.loads(p), json.loads(q)
                assert {k: v for k, v in q.items() if not k.startswith("vif")} == p
                assert list(q)[:len(p)] == list(p)  # the VIF columns come after every other column
    # without -m vif every output is what the parent printed: no vif key anywhere
    for fmt in ("json", "json-lines", "csv", "default"):
        assert "vif" not in _cli(a, b, "-m", "psnr", "--output", fmt).lower()


def test_cli_vif_refusals(tmp_path):
    a = str(tmp_path / "a.ppm")
    with open(a, "wb") as f:
        f.write(b"P6\n32 32\n255\n" + bytes(32 * 32 * 3))
    out = subprocess.run([CLI, a, a, "-m", "vif"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "vif" in out.stderr, (out.returncode, out.stderr)
    y, z, _ = _files(tmp_path, 64, 48, 2, 8)
    for extra in (["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
        out = subprocess.run([CLI, y, z, "-m", "vif", *extra], capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "-m vif does not run with" in out.stderr, (extra, out.returncode, out.stderr)
