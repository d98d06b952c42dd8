"""GPU tier of scene-cut detection (libturbometrics_scene.so on the MI355X): every histogram equal to the CPU restatement
(tests/scene_ref.py) in all 256 bins -- the hand-derived pictures, four contents at sizes from 1 x 1 to 2160p, all layouts, the three
memory kinds with odd pitches and an unaligned device base, batches, repeated computes, the state errors; the CLI's --scenes in every
output format; and the CLI without --scenes against a recorded run of the parent commit's binary on the same inputs
(tests/golden/scene_parent_cli.json).  No tolerance anywhere: the definition is integer."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import scene_ref as R
from tests import scene_util as U
from tests.test_gpu_motion import _hand_over, _y4m
from tm_pkg import tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_parent_cli.json")


@pytest.fixture(scope="module", autouse=True)
def _hip():
    tm.init_hip(0)


def one_bin(b, n):
    h = np.zeros(256, np.uint32)
    h[b] = n
    return h


def _compute(s, layout, bits, pics, mem="host", aligned=True, pad=0, dirty=True):
    """the pictures as slots 0 .. n-1 of one compute -> their histograms"""
    keep = [_hand_over(U.luma_plane(layout, Y, bits, pad=pad, dirty=(i + 1 if dirty else None)), mem, aligned) for i, Y in enumerate(pics)]
    for i, p in enumerate(keep):
        s.set_frame(i, p)
    s.compute(len(pics))
    return [f.hist for f in s.frames(len(pics))]


def _same(got, pics, bits):
    assert len(got) == len(pics)
    for g, Y in zip(got, pics):
        want = R.hist(Y, bits)
        assert g.dtype == np.uint32 and g.shape == (256,) and int(g.astype(np.uint64).sum()) == Y.size
        assert (g == want).all(), np.flatnonzero(g != want)[:8]
    return True


def test_hand_derived_pictures():
    for layout, bits in U.CASES:
        w, h = 37, 5
        vals = [0, (1 << bits) - 1, 0x5A5A % (1 << bits)]
        with tm.Scene(w, h, layout, bits, batch=3) as s:
            got = _compute(s, layout, bits, [np.full((h, w), v, np.int64) for v in vals])
            assert all((g == one_bin(v >> (bits - 8), w * h)).all() for v, g in zip(vals, got))
            assert s.mem_usage() > 0
    for layout, bits in (("y8", 8), ("y16_msb", 10), ("y10_packed", 10)):
        w, h = 1 << bits, 3
        Y = np.tile(np.arange(w, dtype=np.int64), (h, 1))
        with tm.Scene(w, h, layout, bits) as s:
            assert (_compute(s, layout, bits, [Y])[0] == w * h // 256).all()
    w, h = 257, 6
    Y = np.tile(np.arange(w, dtype=np.int64) % 256, (h, 1))
    want = np.full(256, h, np.uint32)
    want[0] = 2 * h
    with tm.Scene(w, h, "y8", 8) as s:
        assert (_compute(s, "y8", 8, [Y])[0] == want).all()
    # nothing in bin 0: a lane beyond the width that is counted shows there
    for layout, bits in U.CASES:
        for w in (1, 2, 3, 5, 7):
            Y = (np.indices((3, w)).sum(axis=0) % 3 + 1) * (((1 << bits) - 1) // 4)
            with tm.Scene(w, 3, layout, bits) as s:
                for mem, aligned in (("host", True), ("device", True), ("device", False)):
                    g = _compute(s, layout, bits, [Y], mem, aligned)[0]
                    assert g[0] == 0 and (g == R.hist(Y, bits)).all(), (layout, bits, w, mem, aligned)


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (65, 33), (257, 9), (33, 517), (256, 256)])
def test_four_contents_equal_the_restatement(w, h):
    for layout, bits in (("y8", 8), ("y16_msb", 10), ("y16_low", 12), ("y10_packed", 10)):
        pics = [U.picture(w, h, bits, k, seed=w + h) for k in U.KINDS]
        with tm.Scene(w, h, layout, bits, batch=4) as s:
            assert _same(_compute(s, layout, bits, pics, pad=3 if layout != "y10_packed" else 0), pics, bits)
            assert _same(_compute(s, layout, bits, pics, "device"), pics, bits)


@pytest.mark.parametrize("w,h,layout,bits", [(1920, 1080, "y8", 8), (3840, 2160, "y16_msb", 10)])
def test_large_pictures_equal_the_restatement(w, h, layout, bits):
    pics = [U.picture(w, h, bits, "noise", seed=1), U.picture(w, h, bits, "flat", seed=2)]
    with tm.Scene(w, h, layout, bits, batch=2) as s:
        assert _same(_compute(s, layout, bits, pics, "device", dirty=False), pics, bits)


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_memory_kinds_pitches_and_dirty_bytes(layout, bits):
    w, h = 65, 33
    pics = [U.picture(w, h, bits, k, seed=5) for k in U.KINDS]
    with tm.Scene(w, h, layout, bits, batch=4) as s:
        for mem, aligned in (("host", True), ("pinned", True), ("pinned", False), ("device", True), ("device", False)):
            assert _same(_compute(s, layout, bits, pics, mem, aligned, pad=0 if mem != "host" else 7), pics, bits), (mem, aligned)


def test_batches_repeats_and_state_errors():
    w, h, layout, bits = 65, 33, "y16_msb", 10
    pics = [U.picture(w, h, bits, U.KINDS[i % 4], seed=100 + i) for i in range(8)]
    assert len({R.hist(p, bits).tobytes() for p in pics}) == 8
    with tm.Scene(w, h, layout, bits, batch=8) as s:
        first = _compute(s, layout, bits, pics, "device")
        assert _same(first, pics, bits)
        # the same slots again with other content: nothing of the first compute is left
        other = pics[::-1]
        assert _same(_compute(s, layout, bits, other, "device"), other, bits)
        assert _same(_compute(s, layout, bits, other[:3]), other[:3], bits)
        # the same input twice: the same answer twice
        again = _compute(s, layout, bits, pics, "device")
        assert all((a == b).all() for a, b in zip(first, again))
        # a slot that was not set again is an error, not a stale picture
        with pytest.raises(tm.scene.SceneError) as e:
            s.compute(1)
        assert e.value.code == tm.ffi.TM_ERR_STATE
        # one compute at a time
        L = tm.scene.lib()
        keep = [_hand_over(U.luma_plane(layout, p, bits), "device", True) for p in pics]
        for i, p in enumerate(keep):
            s.set_frame(i, p)
        assert L.tm_scene_compute_async(s._h, 8) == tm.ffi.TM_OK
        assert L.tm_scene_compute_async(s._h, 8) == tm.ffi.TM_ERR_STATE
        assert L.tm_scene_sync(s._h) == tm.ffi.TM_OK
        assert _same([f.hist for f in s.frames(8)], pics, bits)
        assert _same([f.hist for f in s.frames(2, first=5)], pics[5:7], bits)


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def _cli(*args, cli=CLI, env=None):
    out = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300, env=None if env is None else {**os.environ, **env})
    assert out.returncode == 0, out.stderr
    return out.stdout


W, H = 64, 48
SCENES = [(10, 4), (120, 3), (230, 5)]  # three flat "scenes": (bin, pictures)


def _scene_files(d, bits=8, lumas=None):
    if lumas is None:
        lumas = [np.full((H, W), b << (bits - 8), np.int64) for b, n in SCENES for _ in range(n)]
    a, b = os.path.join(str(d), "a.y4m"), os.path.join(str(d), "b.y4m")
    _y4m(a, W, H, lumas, bits, 1)
    _y4m(b, W, H, [(p + 1) % (1 << bits) for p in lumas], bits, 2)
    return a, b


WANT_SCORES = [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
WANT_CUTS = [0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0]


@pytest.mark.parametrize("bits,batch", [(8, "5"), (10, "12"), (12, "1")])
def test_cli_scenes_in_every_output_format(tmp_path, bits, batch):
    a, b = _scene_files(tmp_path, bits)
    n = len(WANT_SCORES)
    base = (a, b, "--scenes", "--batch", batch)
    lines = [json.loads(x) for x in _cli(*base, "--output", "json-lines").splitlines() if x.strip()]
    frames, agg = [d for d in lines if "frame_count" not in d], [d for d in lines if "frame_count" in d][0]
    assert [f["scene_score"] for f in frames] == WANT_SCORES and [f["scene_cut"] for f in frames] == WANT_CUTS
    assert all(list(f) == ["scene_score", "scene_cut"] for f in frames)
    assert agg["frame_count"] == n and agg["scene_starts"] == [0, 4, 7] and agg["scene_score"]["max"] == 1.0 and agg["scene_score"]["min"] == 0.0
    js = json.loads(_cli(*base, "--output", "json"))
    assert js["scene_score"]["scores"] == WANT_SCORES and js["scene_starts"] == [0, 4, 7] and js["frame_count"] == n
    assert js["scene_score"]["stats"]["mean"] == agg["scene_score"]["mean"] and abs(agg["scene_score"]["mean"] - 2.0 / 12.0) < 1e-15
    rows = _cli(*base, "--output", "csv").splitlines()
    # the rows as they are computed, then the whole table once more behind them
    assert rows[0] == "scene_score,scene_cut" == rows[1 + n] and len(rows) == 2 * (1 + n)
    for part in (rows[1:1 + n], rows[2 + n:]):
        assert [(float(r.split(",")[0]), r.split(",")[1]) for r in part] == [(s, str(c)) for s, c in zip(WANT_SCORES, WANT_CUTS)]
    txt = _cli(*base)
    assert "SCENE_SCORE: Stats {" in txt and "SCENE_STARTS: [0, 4, 7]" in txt


def test_cli_scenes_beside_psnr_and_motion(tmp_path):
    a, b = _scene_files(tmp_path)
    for sel in (["-m", "psnr"], ["--motion"]):
        for fmt in ("json-lines", "csv"):
            plain = _cli(a, b, *sel, "--batch", "5", "--output", fmt).splitlines()
            with_s = _cli(a, b, *sel, "--scenes", "--batch", "5", "--output", fmt).splitlines()
            assert len(plain) == len(with_s)
            if fmt == "csv":
                ncol = len(plain[0].split(","))
                assert [r.split(",")[:ncol] for r in with_s] == [r.split(",") for r in plain]
                assert with_s[0].split(",")[ncol:] == ["scene_score", "scene_cut"]
                assert [int(r.split(",")[ncol + 1]) for r in with_s[1:13]] == WANT_CUTS
            else:
                for p, q in zip(plain, with_s):
                    p, q = json.loads(p), json.loads(q)
                    assert {k: v for k, v in q.items() if not k.startswith("scene_")} == p
                    assert list(q)[:len(p)] == list(p)  # the scene columns come after every other column
                assert [json.loads(q)["scene_score"] for q in with_s[:12]] == WANT_SCORES
                assert json.loads(with_s[12])["scene_starts"] == [0, 4, 7]
    assert "scene" not in _cli(a, b, "-m", "psnr", "--motion", "--output", "json").lower()


def test_cli_bins_threshold_and_every(tmp_path):
    # pictures that differ by one code: bins 100, 101, 101, 104 -- 100 | 101 share a merged bin of 64, 101 | 104 do not
    lumas = [np.full((H, W), v, np.int64) for v in (100, 101, 101, 104)]
    a, b = _scene_files(tmp_path, 8, lumas)

    def run(*extra):
        return json.loads(_cli(a, b, "--scenes", "--output", "json", *extra))
    js = run()
    assert js["scene_score"]["scores"] == [0.0, 0.0, 0.0, 1.0] and js["scene_starts"] == [0, 3]
    js = run("--scene-bins", "256", "--scene-threshold", "1")
    assert js["scene_score"]["scores"] == [0.0, 1.0, 0.0, 1.0] and js["scene_starts"] == [0, 1, 3]
    js = run("--scene-bins=16")
    assert js["scene_score"]["scores"] == [0.0, 0.0, 0.0, 0.0] and js["scene_starts"] == [0]
    # half of the samples leave their bin: score 0.5, a cut at 0.5 (the >=) and none above it
    half = np.full((H, W), 100, np.int64)
    half[: H // 2] = 200
    a, b = _scene_files(tmp_path, 8, [np.full((H, W), 100, np.int64), half, half])
    assert run()["scene_starts"] == [0, 1] and run()["scene_score"]["scores"] == [0.0, 0.5, 0.0]
    assert run("--scene-threshold", "0.5000001")["scene_starts"] == [0]
    # --every: the score is that against the previous KEPT picture
    a, b = _scene_files(tmp_path)
    js = run("--every", "2")  # frames 0, 2, 4, 6, 8, 10: bins 10, 10, 120, 120, 230, 230
    assert js["scene_score"]["scores"] == [0.0, 0.0, 1.0, 0.0, 1.0, 0.0] and js["scene_starts"] == [0, 2, 4]


def test_cli_scenes_refuses_rgb_images(tmp_path):
    a = str(tmp_path / "a.ppm")
    with open(a, "wb") as f:
        f.write(b"P6\n16 16\n255\n" + bytes(16 * 16 * 3))
    out = subprocess.run([CLI, a, a, "--scenes"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "scenes" in out.stderr, (out.returncode, out.stderr)


# what the parent commit's binary printed for these arguments on the inputs of _parent_files(dir, bits): recorded once with
# record_parent_cli(<the parent's turbo-metrics>, GOLDEN, <a scratch directory>) on an MI355X
PARENT_CASES = {
    "psnr_jsonl_8": (8, ["-m", "psnr", "--output", "json-lines"]),
    "psnr_ssimu_json_8": (8, ["-m", "psnr", "-m", "ssimulacra2", "--output", "json"]),
    "vif_motion_psnr_csv_8": (8, ["-m", "vif", "--motion", "-m", "psnr", "--batch", "3", "--output", "csv"]),
    "adm_default_8": (8, ["-m", "adm"]),
    "vif_default_10": (10, ["-m", "vif"]),
    "xpsnr_ssim_csv_10": (10, ["-m", "xpsnr", "-m", "ssim", "--output", "csv"]),
    "motion_adm_jsonl_10": (10, ["--motion", "-m", "adm", "--output", "json-lines"]),
}


def _parent_files(d, bits):
    from tests import motion_util
    seq = motion_util.sequence(160, 96, 4, bits, "smooth")
    a, b = os.path.join(d, "a.y4m"), os.path.join(d, "b.y4m")
    _y4m(a, 160, 96, seq, bits, 1)
    _y4m(b, 160, 96, [(p + 1) % (1 << bits) for p in seq], bits, 2)
    return a, b


def _run_parent_cases(cli, tmp):
    out = {}
    for bits in (8, 10):
        d = os.path.join(str(tmp), f"in{bits}")
        os.makedirs(d, exist_ok=True)
        a, b = _parent_files(d, bits)
        for name, (bb, args) in PARENT_CASES.items():
            if bb == bits:
                out[name] = _cli(a, b, *args, cli=cli)
    return out


def record_parent_cli(cli, dest, tmp):
    with open(dest, "w") as f:
        json.dump(_run_parent_cases(cli, tmp), f, indent=1, sort_keys=True)
        f.write("\n")


def test_cli_without_scenes_is_byte_identical_with_the_parents(tmp_path):
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(PARENT_CASES)
    got = _run_parent_cases(CLI, tmp_path)
    for name in PARENT_CASES:
        assert got[name] == want[name], name
        assert "scene" not in got[name].lower()
