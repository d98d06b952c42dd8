"""GPU tier of VMAF's ADM (libturbometrics_adm.so on the MI355X): the 24 sums of every pair against the CPU restatement
(tests/adm_ref.py) within the bound derived in tests/test_adm_cpu.py (the exact properties exactly); memory kinds, pitches and dirty
bytes; batches with distinct pairs per slot; the same batch twice is bit-identical; a slot not set again is TM_ERR_STATE; the CLI's
-m adm alone, beside -m psnr and beside -m vif --motion; and the CLI without -m adm against a recorded run of the parent commit's
binary on the same inputs (tests/golden/adm_parent_cli.json)."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import adm_ref as R
from tests import adm_util as U
from tests import vif_ref
from tests.test_adm_cpu import rtol
from tests.test_gpu_motion import _hand_over, _y4m
from tm_pkg import tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
GOLDEN = os.path.join(ROOT, "tests", "golden", "adm_parent_cli.json")
SEEN = {"rel": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _hip():
    tm.init_hip(0)


def _close(got, want, w, h, what):
    """got: AdmFrame; want: adm_ref.adm's list"""
    for s in range(4):
        for k, gs in (("num", got.num_cube[s]), ("den", got.den_cube[s])):
            for b in range(3):
                g, x = gs[b], want[s][k][b]
                rel = abs(g - x) / max(abs(x), 1e-300) if g != x else 0.0
                SEEN["rel"] = max(SEEN["rel"], rel)
                print(f"{what} scale {s} {k}[{R.BANDS[b]}]: gpu {g!r} restatement {x!r} rel {rel:.3e} bound {rtol(want[s]['area']):.3e}")
                assert rel <= rtol(want[s]["area"]), (what, s, k, b, g, x)
    sc = R.scores([p["num"] for p in want], [p["den"] for p in want], w, h)
    # the scores: cube roots of sums within the bound above (a third of it each) and of the C library (tests/test_adm_cpu.py: 5e-15)
    assert all(abs(a - b) <= (rtol(want[0]["area"]) + 5e-15) * b for a, b in zip(list(got.scales) + [got.adm2], sc))


def _set(v, slot, layout, bits, ref, dis, mem="host", aligned=True, pad=0, dirty=None):
    planes = [_hand_over(U.luma_plane(layout, p, bits, pad=pad, dirty=None if dirty is None else dirty + i), mem, aligned) for i, p in enumerate((ref, dis))]
    v.set_pair(slot, *planes)
    return planes


def _one_pair(layout, bits, w, h, kind):
    ref, dis = U.pair(w, h, bits, kind)
    with tm.Adm(w, h, layout, bits, batch=1) as v:
        keep = _set(v, 0, layout, bits, ref, dis, pad=3, dirty=5)
        v.compute(1)
        _close(v.frames(1)[0], R.adm(ref, dis, bits), w, h, f"{layout} {bits} {w}x{h} {kind}")
        assert v.mem_usage() > 0 and keep


@pytest.mark.parametrize("w,h", [(32, 32), (33, 47), (75, 35), (131, 70)])
@pytest.mark.parametrize("layout,bits", U.CASES)
def test_matches_the_restatement(layout, bits, w, h):
    _one_pair(layout, bits, w, h, U.CONTENTS[(U.CASES.index((layout, bits)) + w) % len(U.CONTENTS)])


@pytest.mark.parametrize("layout,bits,w,h", [("y8", 8, 1920, 1080), ("y16_msb", 10, 1920, 1080), ("y10_packed", 10, 1280, 720), ("y16_low", 16, 1280, 720)])
def test_matches_the_restatement_at_full_size(layout, bits, w, h):
    _one_pair(layout, bits, w, h, "noisy")


@pytest.mark.parametrize("kind", U.CONTENTS)
def test_every_content(kind):
    w, h = 200, 90
    for layout, bits in (("y8", 8), ("y16_msb", 16)):
        ref, dis = U.pair(w, h, bits, kind, seed=3)
        with tm.Adm(w, h, layout, bits, batch=1) as v:
            _set(v, 0, layout, bits, ref, dis)
            v.compute(1)
            _close(v.frames(1)[0], R.adm(ref, dis, bits), w, h, f"{layout} {bits} {kind}")


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_the_exact_properties_are_exact(layout, bits):
    """identical and flat pictures: N == Dn bit for bit, every score 1.0; a mid-grey distorted picture: N == 0; half contrast:
    8 N == Dn (derivations: tests/test_adm_cpu.py)"""
    w, h = 75, 45
    M, unit = (1 << bits) - 1, 1 << (bits - 8)
    ref = U.pair(w, h, bits, "blurred", seed=2)[0]
    half = np.random.default_rng(11).integers(-60, 61, (h, w))
    with tm.Adm(w, h, layout, bits, batch=1) as v:
        for pic in (ref, np.full((h, w), 1, np.int64), np.full((h, w), M, np.int64)):
            _set(v, 0, layout, bits, pic, pic, pad=2, dirty=3)
            v.compute(1)
            f = v.frames(1)[0]
            assert f.num_cube == f.den_cube and list(f.scales) == [1.0] * 4 and f.adm2 == 1.0, f
        _set(v, 0, layout, bits, ref, np.full((h, w), 1 << (bits - 1), np.int64), pad=2, dirty=3)
        v.compute(1)
        f = v.frames(1)[0]
        assert all(n == (0.0, 0.0, 0.0) for n in f.num_cube) and all(min(d) > 0.0 for d in f.den_cube) and 0.0 < f.adm2 < 1.0, f
        _set(v, 0, layout, bits, (128 + 2 * half) * unit, (128 + half) * unit, mem="device")
        v.compute(1)
        f = v.frames(1)[0]
        assert all(tuple(8.0 * n for n in ns) == ds for ns, ds in zip(f.num_cube, f.den_cube)) and min(min(d) for d in f.den_cube) > 0.0, f


@pytest.mark.parametrize("layout,bits", [("y8", 8), ("y16_msb", 10), ("y16_low", 12), ("y10_packed", 10)])
def test_memory_kinds_pitches_and_dirty_bytes(layout, bits):
    w, h = 250, 37
    ref, dis = U.pair(w, h, bits, "noisy", seed=9)
    want = R.adm(ref, dis, bits)
    with tm.Adm(w, h, layout, bits, batch=2) as v:
        seen = []
        for mem, aligned in (("host", True), ("pinned", True), ("pinned", False), ("device", True), ("device", False)):
            keep = _set(v, 0, layout, bits, ref, dis, mem, aligned, pad=0 if mem != "host" else 7, dirty=21)
            v.compute(1)
            f = v.frames(1)[0]
            _close(f, want, w, h, f"{layout} {mem} {aligned}")
            seen.append((f.num_cube, f.den_cube))
            del keep
        assert all(s == seen[0] for s in seen)  # the same samples: the same bits, whatever the memory kind, pitch or dirty bytes


def test_batches_with_distinct_pairs_per_slot_twice_and_the_state_rule():
    w, h, bits, cap = 96, 64, 10, 5
    pairs = [U.pair(w, h, bits, U.CONTENTS[i % len(U.CONTENTS)], seed=i) for i in range(cap)]
    want = [R.adm(r, d, bits) for r, d in pairs]
    with tm.Adm(w, h, "y16_msb", bits, batch=cap) as v:
        for n in (1, 3, cap):
            runs = []
            for _ in range(2):
                keep = [_set(v, i, "y16_msb", bits, *pairs[i], mem="device") for i in range(n)]
                v.compute(n)
                fr = v.frames(n)
                for i in range(n):
                    _close(fr[i], want[i], w, h, f"batch {n} slot {i}")  # slot i holds pair i's answer
                runs.append([(f.num_cube, f.den_cube) for f in fr])
                del keep
            assert runs[0] == runs[1]  # no floating-point atomics: bit-identical
        # a slot that was not set again is an error, not a stale pair
        with pytest.raises(tm.adm.AdmError) as e:
            v.compute(1)
        assert e.value.code == tm.ffi.TM_ERR_STATE
        _set(v, 0, "y16_msb", bits, *pairs[0])
        with pytest.raises(tm.adm.AdmError) as e:
            v.compute(2)
        assert e.value.code == tm.ffi.TM_ERR_STATE


def test_largest_difference_seen():
    print(f"largest relative difference of the 24 sums, GPU vs restatement: {SEEN['rel']:.3e}")
    assert SEEN["rel"] <= rtol(2 ** 19)


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def _cli(*args, cli=CLI):
    out = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def _files(tmp_path, w, h, n, bits):
    pairs = [U.pair(w, h, bits, "noisy", seed=i) for i in range(n)]
    a, b = os.path.join(str(tmp_path), "a.y4m"), os.path.join(str(tmp_path), "b.y4m")
    _y4m(a, w, h, [p[0] for p in pairs], bits, 1)
    _y4m(b, w, h, [p[1] for p in pairs], bits, 2)
    want = []
    for r, d in pairs:
        res = R.adm(r, d, bits)
        sc = R.scores([p["num"] for p in res], [p["den"] for p in res], w, h)
        want.append([sc[4]] + sc[:4])
    return a, b, want, pairs


NAMES = ["adm2", "adm_scale0", "adm_scale1", "adm_scale2", "adm_scale3"]


def _near(got, want):
    """to the printed digits: the shortest round-trip text of a double within 2e-9 (relative) of the restatement's, far above the
    bound of the sums"""
    return all(abs(g - w) <= 2e-9 * max(abs(w), 1.0) for g, w in zip(got, want))


@pytest.mark.parametrize("bits,batch", [(8, "3"), (10, "4"), (12, "7")])
def test_cli_adm_alone_in_every_output_format(tmp_path, bits, batch):
    w, h, n = 322, 182, 7
    a, b, want, _ = _files(tmp_path, w, h, n, bits)
    base = (a, b, "-m", "adm", "--batch", batch)
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
    assert "ADM2: Stats {" in txt and "ADM_SCALE3: Stats {" in txt
    # --every keeps every second pair: ADM has no history
    ev = [json.loads(x) for x in _cli(*base, "--every", "2", "--output", "json-lines").splitlines() if x.strip()]
    assert [f for f in ev if "frame_count" not in f] == frames[::2]


def test_cli_adm_beside_psnr_leaves_the_other_columns_alone(tmp_path):
    a, b, want, _ = _files(tmp_path, 320, 180, 6, 8)
    for fmt in ("json-lines", "csv"):
        plain = _cli(a, b, "-m", "psnr", "--batch", "4", "--output", fmt).splitlines()
        with_a = _cli(a, b, "-m", "psnr", "-m", "adm", "--batch", "4", "--output", fmt).splitlines()
        assert len(plain) == len(with_a)
        if fmt == "csv":
            assert [r.split(",")[:1] for r in with_a] == [r.split(",") for r in plain]
            assert with_a[0].split(",")[1:] == NAMES
            assert all(_near([float(x) for x in r.split(",")[1:]], wv) for r, wv in zip(with_a[1:7], want))
        else:
            for p, q in zip(plain, with_a):
                p, q = json.loads(p), json.loads(q)
                assert {k: v for k, v in q.items() if not k.startswith("adm")} == p
                assert list(q)[:len(p)] == list(p)  # the ADM columns come after every other column


def test_cli_prints_all_six_inputs_of_the_model_in_one_run(tmp_path):
    """-m adm beside -m vif --motion: motion2, vif_scale0 .. 3 and adm2 of every pair, each equal to what its own run prints"""
    w, h, n = 320, 180, 5
    a, b, want, pairs = _files(tmp_path, w, h, n, 8)
    rows = _cli(a, b, "-m", "vif", "-m", "adm", "--motion", "--batch", "3", "--output", "csv").splitlines()
    head = rows[0].split(",")
    assert head == ["motion", "motion2", "vif_scale0", "vif_scale1", "vif_scale2", "vif_scale3", "vif"] + NAMES
    body = [[float(x) for x in r.split(",")] for r in rows[1:1 + n]]
    assert all(_near(r[7:], wv) for r, wv in zip(body, want))
    vif_want = [vif_ref.scores(vif_ref.vif(r, d, 8)) for r, d in pairs]
    assert all(_near(r[2:7], wv) for r, wv in zip(body, vif_want))
    alone = [[float(x) for x in r.split(",")] for r in _cli(a, b, "--motion", "--batch", "3", "--output", "csv").splitlines()[1:1 + n]]
    assert [r[:2] for r in body] == alone
    only = [[float(x) for x in r.split(",")] for r in _cli(a, b, "-m", "adm", "--output", "csv").splitlines()[1:1 + n]]
    assert [r[7:] for r in body] == only  # the batch size and the neighbours change no bit


def test_cli_adm_refusals(tmp_path):
    a = str(tmp_path / "a.ppm")
    with open(a, "wb") as f:
        f.write(b"P6\n32 32\n255\n" + bytes(32 * 32 * 3))
    out = subprocess.run([CLI, a, a, "-m", "adm"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "adm" in out.stderr, (out.returncode, out.stderr)
    y, z, _, _ = _files(tmp_path, 64, 48, 2, 8)
    for extra in (["--devices", "2"], ["--ranks", "2"], ["--loop", "reference"], ["--loop", "deferred"]):
        out = subprocess.run([CLI, y, z, "-m", "adm", *extra], capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "-m adm does not run with" in out.stderr, (extra, out.returncode, out.stderr)


# what the parent commit's binary printed for these arguments on the inputs of _files(dir, 160, 96, 4, 8) / (.., 10): recorded once
# with record_parent_cli(<the parent's turbo-metrics>, GOLDEN) on an MI355X
PARENT_CASES = {
    "psnr_jsonl_8": (8, ["-m", "psnr", "--output", "json-lines"]),
    "psnr_ssimu_json_8": (8, ["-m", "psnr", "-m", "ssimulacra2", "--output", "json"]),
    "vif_motion_psnr_csv_8": (8, ["-m", "vif", "--motion", "-m", "psnr", "--batch", "3", "--output", "csv"]),
    "vif_default_10": (10, ["-m", "vif"]),
    "xpsnr_ssim_csv_10": (10, ["-m", "xpsnr", "-m", "ssim", "--output", "csv"]),
    "motion_jsonl_10": (10, ["--motion", "--output", "json-lines"]),
}


def _run_parent_cases(cli, tmp):
    out = {}
    for bits in (8, 10):
        d = os.path.join(str(tmp), f"in{bits}")
        os.makedirs(d, exist_ok=True)
        a, b, _, _ = _files(d, 160, 96, 4, bits)
        for name, (bb, args) in PARENT_CASES.items():
            if bb == bits:
                out[name] = _cli(a, b, *args, cli=cli)
    return out


def record_parent_cli(cli, dest, tmp):
    with open(dest, "w") as f:
        json.dump(_run_parent_cases(cli, tmp), f, indent=1, sort_keys=True)
        f.write("\n")


def test_cli_without_adm_is_byte_identical_with_the_parents(tmp_path):
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(PARENT_CASES)
    got = _run_parent_cases(CLI, tmp_path)
    for name in PARENT_CASES:
        assert got[name] == want[name], name
        assert "adm" not in got[name].lower()
