"""LDR-FLIP throughput of libturbometrics_flip.so from HBM-resident packed RGB8 pictures (torch device tensors, TM_MEM_DEVICE), batch
128, at 1080p and 2160p: a smooth picture against a copy with noise on a tenth of its pixels.  Prints one JSON line per case: pairs/s
(wall clock over whole computes, results on the host; the median and the spread of --repeats windows), and the tile kernel's time per
batch from a `rocprofv3 --kernel-trace --stats` run of this script in a child process of its own, with the COMPULSORY HBM traffic that
time stands for (6 bytes read and 12 written per pixel; the halo re-reads -- 84 x 36 pixels loaded per 64 x 16 tile, about three times
the RGB bytes, served by the caches or by HBM -- are not counted) as a fraction of 8 TB/s.

    python tools/flip_bench.py [--iters N] [--repeats R] [--batch B] [--no-prof]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch  # noqa: F401  (torch's HIP runtime first, like bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tm_pkg import tm  # noqa: E402

CASES = [("1080p_rgb8", 1920, 1080), ("2160p_rgb8", 3840, 2160)]
KERNELS = ("k_flip_tile", "k_flip_finish")
DISTINCT = 8  # distinct device pairs a batch cycles through
HBM_BYTES_PER_S = 8e12


def surfaces(w, h, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.arange(w, dtype=torch.int32, device="cuda").repeat(h, 1)
    y = torch.arange(h, dtype=torch.int32, device="cuda").unsqueeze(1).repeat(1, w)
    out = []
    for i in range(n):
        a = torch.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), ((x // 16 + y // 16 + i) % 2) * 200], -1)
        noise = torch.randint(-20, 21, (h, w, 3), dtype=torch.int32, device="cuda", generator=g)
        hit = (torch.rand((h, w, 1), device="cuda", generator=g) < 0.1).to(torch.int32)
        b = (a + noise * hit).clamp(0, 255)
        out.append((a.to(torch.uint8).contiguous(), b.to(torch.uint8).contiguous()))
    return out


def run(iters, repeats, batch):
    tm.init_hip(0)
    res = {}
    for name, w, h in CASES:
        pairs = surfaces(w, h, DISTINCT, 1)
        torch.cuda.synchronize()
        with tm.Flip(w, h, "rgb8", batch=batch) as f:
            def step():  # every compute takes its slots' pairs anew (device tensors: descriptors only, no copy)
                for k in range(batch):
                    f.set_pair(k, *pairs[(k * 3) % DISTINCT])
                f.compute(batch)
            step()  # warm-up
            step()
            fr = f.frames(1)[0]
            assert 0 < fr.mean < 1, fr
            rates = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _ in range(iters):
                    step()
                rates.append(batch * iters / (time.perf_counter() - t0))
            res[name] = {"pairs_per_s": statistics.median(rates), "pairs_per_s_min": min(rates), "pairs_per_s_max": max(rates), "repeats": repeats,
                         "iters": iters, "w": w, "h": h, "batch": batch, "ppd": f.ppd, "flip_of_slot_0": fr.mean, "mem_mib": f.mem_usage() >> 20}
    return res


def kernel_times(iters, batch):
    """calls and total / min / max ns of the two kernels per case, from rocprofv3 over a child run of this script (one case per child)"""
    out = {}
    for name, *_ in CASES:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "fb", "--",
                   sys.executable, os.path.abspath(__file__), "--child", name, "--iters", str(iters), "--repeats", "1", "--batch", str(batch), "--no-prof"]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                raise RuntimeError(f"rocprofv3 failed ({p.returncode}): {p.stderr[-2000:]}")
            stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not stats:
                raise RuntimeError("rocprofv3 wrote no kernel_stats.csv: " + " ".join(glob.glob(os.path.join(d, "**"), recursive=True)[:20]))
            for row in csv.DictReader(open(stats[0])):
                for k in KERNELS:
                    if k in row["Name"]:
                        e = out.setdefault(name, {}).setdefault(k, {"calls": 0, "total_ns": 0.0, "min_ns": float("inf"), "max_ns": 0.0})
                        e["calls"] += int(row["Calls"])
                        e["total_ns"] += float(row["TotalDurationNs"])
                        e["min_ns"] = min(e["min_ns"], float(row["MinNs"]))
                        e["max_ns"] = max(e["max_ns"], float(row["MaxNs"]))
            out.setdefault(name, {})["computes"] = iters + 2  # (the child's two warm-up computes included)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        global CASES
        CASES = [c for c in CASES if c[0] == a.child]
        run(a.iters, a.repeats, a.batch)
        return
    res = run(a.iters, a.repeats, a.batch)
    for name, r in res.items():
        print(json.dumps({"case": name, "wall_clock_only": True, **r}), flush=True)
    prof = {} if a.no_prof else kernel_times(2, a.batch)
    for name, r in res.items():
        k = prof.get(name, {})
        n = k.get("computes", 1)
        for kn in KERNELS:
            if kn in k:
                r[kn + "_ms_per_batch"] = k[kn]["total_ns"] / n / 1e6
        if "k_flip_tile" in k:
            s = k["k_flip_tile"]["total_ns"] / n * 1e-9
            r["kernel_pairs_per_s"] = r["batch"] / s
            r["compulsory_hbm_fraction_of_8TBps"] = r["batch"] * r["w"] * r["h"] * 18 / s / HBM_BYTES_PER_S
        print(json.dumps({"case": name, **r}), flush=True)


if __name__ == "__main__":
    main()
