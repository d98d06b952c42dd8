"""GPU tier of CAMBI (libturbometrics_cambi.so on the MI355X) against the CPU restatement (tests/cambi_ref.py): heat maps equal at all
five scales, t, n_gt and k equal, sum_gt within the bound of a naive f64 sum, cambi within 1e-9 relative -- small sizes, windows and
contents, all layouts, the three memory kinds with an unaligned device base, batches, repeated computes, the state errors; 1080p and
2160p through the derived window at scales 2 - 4; the CLI's -m cambi in every output format; and the CLI without -m cambi against a
recorded run of the parent commit's binary on the same inputs (tests/golden/cambi_parent_cli.json)."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import cambi_ref as R
from tests import cambi_util as U
from tests.test_gpu_motion import _hand_over, _y4m
from tm_pkg import tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cambi_parent_cli.json")


@pytest.fixture(scope="module", autouse=True)
def _hip():
    tm.init_hip(0)


def _compute(c, layout, bits, pics, mem="host", aligned=True, pad=0, dirty=True):
    """the pictures as slots 0 .. n-1 of one compute -> per picture a namespace like the restatement's (no mask / plane)"""
    keep = [_hand_over(U.luma_plane(layout, Y, bits, pad=pad, dirty=(i + 1 if dirty else None)), mem, aligned) for i, Y in enumerate(pics)]
    for i, p in enumerate(keep):
        c.set_frame(i, p)
    c.compute(len(pics))
    out = []
    for i, f in enumerate(c.frames(len(pics))):
        out.append(type("Got", (), dict(cmap=[c.heatmap(i, s) for s in range(5)], t=list(f.t), n_gt=list(f.n_gt), k=list(f.k), sum_gt=list(f.sum_gt),
                                        cambi=f.cambi, scales=f.scales)))
    return out


def _same(got, want):
    assert U.same(got, want)
    assert abs(got.cambi - want.cambi) <= 1e-9 * abs(want.cambi)
    assert all(abs(a - b) <= 1e-9 * abs(b) for a, b in zip(got.scales, want.scores))
    return True


@pytest.mark.parametrize("w,h", U.SIZES)
def test_library_equals_the_restatement(w, h):
    layouts = (("y8", 8), ("y16_msb", 10), ("y16_low", 12), ("y10_packed", 10))
    for wi, window in enumerate(U.WINDOWS):
        layout, bits = layouts[(wi + w) % 4]
        pics = [U.picture(w, h, bits, kind, seed=w + window) for kind in U.KINDS]
        want = [R.compute(Y, bits, window, fast=True) for Y in pics]
        with tm.Cambi(w, h, layout, bits, window=window, batch=len(pics)) as c:
            assert c.window == window and c.mem_usage() > 0
            for g, r in zip(_compute(c, layout, bits, pics, "device" if wi % 2 else "host", pad=0 if layout == "y10_packed" else 3), want):
                assert _same(g, r), (layout, window)
    assert any(r.cambi > 0 for r in want)


@pytest.mark.parametrize("w,h,layout,bits,window", [(1920, 1080, "y8", 8, 31), (3840, 2160, "y16_msb", 10, 63)])
def test_large_pictures_through_the_derived_window(w, h, layout, bits, window):
    # a dark staircase of one-code steps 40 pixels wide, with some noise in a corner so that the mask is not full
    x = np.indices((h, w))[1]
    # D = 8: codes 100, 104, ... with the anti-dither filter's half step between them; D = 10: codes 100, 101, ... on either side of 178
    Y = ((25 if bits == 8 else 100) + x // 40).astype(np.int64)
    Y[: h // 8, : w // 8] = np.random.default_rng(1).integers(0, 1 << bits, (h // 8, w // 8))
    want = R.compute(Y, bits, 0, fast=True, scales=(2, 3, 4))
    assert want.window == window
    with tm.Cambi(w, h, layout, bits) as c:
        assert c.window == window
        got = _compute(c, layout, bits, [Y], "device", dirty=False)[0]
    assert U.same(got, want, scales=(2, 3, 4))
    assert max(float(m.max()) for m in got.cmap) > 0 and got.cambi > 0
    assert got.k[0] == int(0.6 * w * h) and got.n_gt[0] < got.k[0]


@pytest.mark.parametrize("layout,bits", U.CASES)
def test_memory_kinds_pitches_and_dirty_bytes(layout, bits):
    w, h, window = 65, 33, 7
    pics = [U.picture(w, h, bits, k, seed=5) for k in ("stairs_lo", "mixed", "stairs_hi")]
    want = [R.compute(Y, bits, window, fast=True) for Y in pics]
    with tm.Cambi(w, h, layout, bits, window=window, batch=3) as c:
        for mem, aligned in (("host", True), ("pinned", True), ("pinned", False), ("device", True), ("device", False)):
            got = _compute(c, layout, bits, pics, mem, aligned, pad=0 if mem != "host" or layout == "y10_packed" else 7)
            assert all(_same(g, r) for g, r in zip(got, want)), (mem, aligned)


def test_batches_repeats_and_state_errors():
    w, h, layout, bits, window = 65, 40, "y16_msb", 10, 7
    pics = [U.picture(w, h, bits, U.KINDS[i % 5], seed=100 + i) for i in range(6)]
    want = [R.compute(Y, bits, window, fast=True) for Y in pics]
    with tm.Cambi(w, h, layout, bits, window=window, batch=6) as c:
        first = _compute(c, layout, bits, pics, "device")
        assert all(_same(g, r) for g, r in zip(first, want))
        # the same slots again with other content: nothing of the first compute is left
        assert all(_same(g, r) for g, r in zip(_compute(c, layout, bits, pics[::-1], "device"), want[::-1]))
        assert all(_same(g, r) for g, r in zip(_compute(c, layout, bits, pics[2:4]), want[2:4]))
        # the same input twice: identical bytes in every field
        again = _compute(c, layout, bits, pics, "device")
        for a, b in zip(first, again):
            assert (a.t, a.n_gt, a.k) == (b.t, b.n_gt, b.k) and np.array(a.sum_gt).tobytes() == np.array(b.sum_gt).tobytes()
            assert a.cambi == b.cambi and all(x.tobytes() == y.tobytes() for x, y in zip(a.cmap, b.cmap))
        # a slot that was not set again is an error, not a stale picture
        with pytest.raises(tm.cambi.CambiError) as e:
            c.compute(1)
        assert e.value.code == tm.ffi.TM_ERR_STATE
        # a heat map of a slot the last compute did not cover
        keep = _hand_over(U.luma_plane(layout, pics[0], bits), "device", True)
        c.set_frame(0, keep)
        c.compute(1)
        with pytest.raises(tm.cambi.CambiError) as e:
            c.heatmap(1, 0)
        assert e.value.code == tm.ffi.TM_ERR_STATE
        # one compute at a time
        L = tm.cambi.lib()
        keep = [_hand_over(U.luma_plane(layout, p, bits), "device", True) for p in pics]
        for i, p in enumerate(keep):
            c.set_frame(i, p)
        assert L.tm_cambi_compute_async(c._h, 6) == tm.ffi.TM_OK
        assert L.tm_cambi_compute_async(c._h, 6) == tm.ffi.TM_ERR_STATE
        assert L.tm_cambi_sync(c._h) == tm.ffi.TM_OK
        fr = c.frames(2, first=3)
        assert [list(f.t) for f in fr] == [want[3].t, want[4].t] and [list(f.n_gt) for f in fr] == [want[3].n_gt, want[4].n_gt]


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def _cli(*args, cli=CLI):
    out = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


W, H = 96, 64
NAMES = ["cambi"] + [f"cambi_scale{s}" for s in range(5)]


def _cambi_files(d, bits):
    dis = [U.picture(W, H, bits, k, seed=i) for i, k in enumerate(("stairs_lo", "mixed", "flat", "stairs_lo", "noise"))]
    ref = [U.picture(W, H, bits, "stairs_lo", seed=7 + i) for i in range(5)]
    a, b = os.path.join(str(d), "a.y4m"), os.path.join(str(d), "b.y4m")
    _y4m(a, W, H, ref, bits, 1)
    _y4m(b, W, H, dis, bits, 2)
    return a, b, ref, dis


def _binding(pics, bits, window=0, topk=0.6):
    layout = "y8" if bits == 8 else "y16_low"
    with tm.Cambi(W, H, layout, bits, window=window, topk=topk, batch=len(pics)) as c:
        for i, Y in enumerate(pics):
            c.set_frame(i, U.luma_plane(layout, Y, bits))
        c.compute(len(pics))
        return [[f.cambi, *f.scales] for f in c.frames(len(pics))]


@pytest.mark.parametrize("bits,batch", [(8, "2"), (10, "5"), (12, "1")])
def test_cli_cambi_in_every_output_format(tmp_path, bits, batch):
    a, b, ref, dis = _cambi_files(tmp_path, bits)
    want = _binding(dis, bits)
    assert any(r[0] > 0 for r in want)
    n = len(want)
    base = (a, b, "-m", "cambi", "--batch", batch)
    lines = [json.loads(x) for x in _cli(*base, "--output", "json-lines").splitlines() if x.strip()]
    frames, agg = [d for d in lines if "frame_count" not in d], [d for d in lines if "frame_count" in d][0]
    assert all(list(f) == NAMES for f in frames) and [[f[k] for k in NAMES] for f in frames] == want
    assert agg["frame_count"] == n and all(abs(agg[k]["mean"] - np.mean([r[i] for r in want])) <= 1e-12 * (1 + agg[k]["mean"]) for i, k in enumerate(NAMES))
    js = json.loads(_cli(*base, "--output", "json"))
    assert [js[k]["scores"] for k in NAMES] == [[r[i] for r in want] for i in range(6)] and js["frame_count"] == n
    assert js["cambi"]["stats"]["mean"] == agg["cambi"]["mean"]
    rows = _cli(*base, "--output", "csv").splitlines()
    # the rows as they are computed, then the whole table once more behind them
    assert rows[0] == ",".join(NAMES) == rows[1 + n] and len(rows) == 2 * (1 + n)
    for part in (rows[1:1 + n], rows[2 + n:]):
        assert [[float(x) for x in r.split(",")] for r in part] == want
    txt = _cli(*base)
    assert "CAMBI: Stats {" in txt and all(f"CAMBI_SCALE{s}: Stats {{" in txt for s in range(5)) and "CAMBI_REF" not in txt


def test_cli_cambi_parameters_ref_and_other_metrics(tmp_path):
    a, b, ref, dis = _cambi_files(tmp_path, 8)
    js = json.loads(_cli(a, b, "-m", "cambi", "--cambi-window", "7", "--cambi-topk", "0.25", "--cambi-ref", "--output", "json"))
    want_d, want_r = _binding(dis, 8, 7, 0.25), _binding(ref, 8, 7, 0.25)
    assert want_d != _binding(dis, 8)
    assert [js[k]["scores"] for k in NAMES] == [[r[i] for r in want_d] for i in range(6)]
    assert [js[k.replace("cambi", "cambi_ref")]["scores"] for k in NAMES] == [[r[i] for r in want_r] for i in range(6)]
    # beside other metrics: their columns are unchanged and come first
    for sel in (["-m", "psnr"], ["--motion", "-m", "vif"], ["--scenes"]):
        for fmt in ("json-lines", "csv"):
            plain = _cli(a, b, *sel, "--batch", "2", "--output", fmt).splitlines()
            with_c = _cli(a, b, *sel, "-m", "cambi", "--batch", "2", "--output", fmt).splitlines()
            assert len(plain) == len(with_c)
            if fmt == "csv":
                ncol = len(plain[0].split(","))
                assert [r.split(",")[:ncol] for r in with_c] == [r.split(",") for r in plain]
                assert with_c[0].split(",")[ncol:] == NAMES
            else:
                for p, q in zip(plain, with_c):
                    p, q = json.loads(p), json.loads(q)
                    assert {k: v for k, v in q.items() if not k.startswith("cambi")} == p and list(q)[:len(p)] == list(p)
                assert [json.loads(q)["cambi"] for q in with_c[:5]] == [r[0] for r in _binding(dis, 8)]


def test_cli_every_feature_library_at_once_equals_each_alone(tmp_path):
    """7 pictures of 160 x 96 in batches of 3 (a partial last batch) with all six feature libraries and the engine in flight for every
    batch: each column is the column of a run that selects that metric alone; and with --every 2 for the metrics that keep no history"""
    from tests import vif_util
    w, h, n = 160, 96, 7
    pairs = [vif_util.pair(w, h, 8, "blurred", seed=i) for i in range(n)]
    a, b = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    _y4m(a, w, h, [p[0] for p in pairs], 8, 1)
    # pictures 1, 2, 5 and 6 band (CAMBI above 0); --every 2 keeps 0, 2, 4, 6: both kinds are in either run
    _y4m(b, w, h, [U.picture(w, h, 8, "mixed", seed=i) if i % 4 in (1, 2) else p[1] for i, p in enumerate(pairs)], 8, 2)

    def run(sel, *extra):
        return [json.loads(x) for x in _cli(a, b, *sel, "--batch", "3", *extra, "--output", "json-lines").splitlines() if x.strip()]
    alone = {"psnr": ["-m", "psnr"], "xpsnr": ["-m", "xpsnr"], "vif": ["-m", "vif"], "adm": ["-m", "adm"], "cambi": ["-m", "cambi"],
             "motion": ["--motion"], "scenes": ["--scenes"]}
    for extra, names in (((), list(alone)), (("--every", "2"), ["psnr", "vif", "adm", "cambi"])):
        together = run([x for k in names for x in alone[k]], *extra)
        assert len(together) == (n if not extra else (n + 1) // 2) + 1
        seen = set()
        for k in names:
            one = run(alone[k], *extra)
            assert len(one) == len(together)
            for p, q in zip(one, together):
                assert p and all(q[c] == v for c, v in p.items()), (k, extra, p, q)  # the per-picture lines and the summary line
                seen |= set(p)
        assert all(set(q) <= seen for q in together)  # and nothing besides
        frames = [q for q in together if "frame_count" not in q]
        assert any(q["cambi"] > 0 for q in frames) and any(q["cambi"] == 0 for q in frames)  # the banded pictures band, the others do not


def test_cli_cambi_refuses_rgb_images(tmp_path):
    a = str(tmp_path / "a.ppm")
    with open(a, "wb") as f:
        f.write(b"P6\n64 64\n255\n" + bytes(64 * 64 * 3))
    out = subprocess.run([CLI, a, a, "-m", "cambi"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "cambi" in out.stderr, (out.returncode, out.stderr)


# what the parent commit's binary printed for these arguments on the inputs of _parent_files(dir, bits): recorded once with
# record_parent_cli(<the parent's turbo-metrics>, GOLDEN, <a scratch directory>) on an MI355X
PARENT_CASES = {
    "psnr_jsonl_8": (8, ["-m", "psnr", "--output", "json-lines"]),
    "psnr_ssimu_json_8": (8, ["-m", "psnr", "-m", "ssimulacra2", "--output", "json"]),
    "vif_motion_scenes_csv_8": (8, ["-m", "vif", "--motion", "--scenes", "--batch", "3", "--output", "csv"]),
    "adm_scenes_default_8": (8, ["-m", "adm", "--scenes"]),
    "vif_default_10": (10, ["-m", "vif"]),
    "xpsnr_ssim_csv_10": (10, ["-m", "xpsnr", "-m", "ssim", "--output", "csv"]),
    "motion_adm_scenes_jsonl_10": (10, ["--motion", "-m", "adm", "--scenes", "--output", "json-lines"]),
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


def test_cli_without_cambi_is_byte_identical_with_the_parents(tmp_path):
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(PARENT_CASES)
    got = _run_parent_cases(CLI, tmp_path)
    for name in PARENT_CASES:
        assert got[name] == want[name], name
        assert "cambi" not in got[name].lower()
