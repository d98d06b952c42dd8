"""ADM throughput of libturbometrics_adm.so from HBM-resident luma planes (torch device tensors, TM_MEM_DEVICE), batch 128, at 1080p
8-bit and 2160p high-aligned 10-bit.  Prints one JSON line per case: pairs/s (wall clock over whole computes, results on the host;
the median and the spread of --repeats windows), the mean time of every kernel from a `rocprofv3 --kernel-trace --stats` run of this
script in a child process of its own, and the fraction of 8 TB/s that the algorithmic bytes of a batch -- both lumas read once, plus
the f32 a bands of scales 0 .. 2 written and read once -- make of the summed kernel time.

    python tools/adm_bench.py [--iters N] [--repeats R] [--no-prof]
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

CASES = [("1080p_y8", 1920, 1080, "y8", 8), ("2160p_y16_msb", 3840, 2160, "y16_msb", 10)]
HBM_PEAK = 8e12
DISTINCT = 16  # distinct device pairs a batch cycles through


def surfaces(w, h, bits, n, seed):
    """n (ref, dis) pairs: noise and a noisier copy of it"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for _ in range(n):
        lo, hi = (16, 236) if bits == 8 else (64, 941)
        ref = torch.randint(lo, hi, (h, w), dtype=torch.int32, device="cuda", generator=g)
        dis = (ref + torch.randint(-(hi - lo) // 16, (hi - lo) // 16 + 1, (h, w), dtype=torch.int32, device="cuda", generator=g)).clamp(0, (1 << bits) - 1)
        out.append(tuple(p.to(torch.uint8) if bits == 8 else (p << (16 - bits)).to(torch.int16) for p in (ref, dis)))
    return out


def algorithmic_bytes(w, h, bits, batch):
    """both lumas read once + the f32 a bands of scales 0 .. 2 (both sides) written and read once, per pair"""
    small, ws, hs = 0, w, h
    for _ in range(3):
        ws, hs = (ws + 1) // 2, (hs + 1) // 2
        small += ws * hs
    return batch * (2 * w * h * (1 if bits == 8 else 2) + 2 * 2 * 4 * small)


def run(iters, repeats, batch=128):
    tm.init_hip(0)
    res = {}
    for name, w, h, layout, bits in CASES:
        pairs = surfaces(w, h, bits, DISTINCT, 1)
        torch.cuda.synchronize()
        with tm.Adm(w, h, layout, bits, batch=batch) as v:
            def step():  # every compute takes its slots' pairs anew (device tensors: descriptors only, no copy)
                for s in range(batch):
                    v.set_pair(s, *pairs[(s * 5) % DISTINCT])
                v.compute(batch)
            step()  # warm-up
            step()
            rates = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _ in range(iters):
                    step()
                rates.append(batch * iters / (time.perf_counter() - t0))
            res[name] = {"pairs_per_s": statistics.median(rates), "pairs_per_s_min": min(rates), "pairs_per_s_max": max(rates),
                         "repeats": repeats, "iters": iters, "w": w, "h": h, "layout": layout, "bits": bits, "batch": batch,
                         "bytes_per_batch": algorithmic_bytes(w, h, bits, batch), "mem_mib": v.mem_usage() >> 20,
                         "adm2_of_slot0": v.frames(1)[0].adm2}
    return res


def kernel_times(iters):
    """per case: {kernel: calls, mean / min / max ns} of every k_adm* kernel, from rocprofv3 over a child run of this script (one case
    per child; tracing only, no counters beside it)"""
    out = {}
    for name, *_ in CASES:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ad", "--",
                   sys.executable, os.path.abspath(__file__), "--child", name, "--iters", str(iters), "--repeats", "1", "--no-prof"]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                raise RuntimeError(f"rocprofv3 failed ({p.returncode}): {p.stderr[-2000:]}")
            stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not stats:
                raise RuntimeError("rocprofv3 wrote no kernel_stats.csv: " + " ".join(glob.glob(os.path.join(d, "**"), recursive=True)[:20]))
            out[name] = {}
            for row in csv.DictReader(open(stats[0])):
                if "k_adm" in row["Name"]:
                    short = row["Name"].split("(")[0].replace("void ", "")
                    out[name][short] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                                        "max_us": float(row["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        global CASES
        CASES = [c for c in CASES if c[0] == a.child]
        run(a.iters, a.repeats)
        return
    res = run(a.iters, a.repeats)
    for name, r in res.items():
        print(json.dumps({"case": name, "wall_clock_only": True, **r}), flush=True)
    prof = {} if a.no_prof else kernel_times(4)
    for name, r in res.items():
        k = prof.get(name)
        if k:
            r["kernels"] = k
            r["kernel_us_per_batch"] = sum(x["mean_us"] for x in k.values())  # one launch of each per batch
            r["kernel_fraction_of_8TBps"] = r["bytes_per_batch"] / (r["kernel_us_per_batch"] * 1e-6) / HBM_PEAK
        print(json.dumps({"case": name, **r}), flush=True)


if __name__ == "__main__":
    main()
