"""SI / TI throughput of libturbometrics_siti.so from HBM-resident luma planes (torch device tensors, TM_MEM_DEVICE), batch 128, at
1080p 8-bit and 2160p high-aligned 10-bit, on noise and on a flat picture.  Prints one JSON line per case: pictures/s (wall clock over whole computes, results on
the host; the median and the spread of --repeats windows), the kernel's mean time from a `rocprofv3 --kernel-trace --stats` run of
this script in a child process of its own, and the fraction of 8 TB/s that the algorithmic bytes of a launch -- one luma read per
picture plus the uint16 history plane read and written once -- make of that kernel time.

    python tools/siti_bench.py [--iters N] [--repeats R] [--no-prof]
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

CASES = [("1080p_y8_noise", 1920, 1080, "y8", 8, "noise"), ("1080p_y8_flat", 1920, 1080, "y8", 8, "flat"),
         ("2160p_y16_msb_noise", 3840, 2160, "y16_msb", 10, "noise"), ("2160p_y16_msb_flat", 3840, 2160, "y16_msb", 10, "flat")]
HBM_PEAK = 8e12
DISTINCT = 32  # distinct device pictures a batch cycles through


def surfaces(w, h, bits, n, seed, content):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for i in range(n):
        if content == "flat":  # every sample of a picture the same value: no magnitude, no atomics beyond T1 / T2
            out.append(torch.full((h, w), 16 + i, dtype=torch.uint8 if bits == 8 else torch.int16, device="cuda") * (1 if bits == 8 else 1 << (16 - bits)))
        elif bits == 8:
            out.append(torch.randint(16, 236, (h, w), dtype=torch.int32, device="cuda", generator=g).to(torch.uint8))
        else:
            out.append((torch.randint(64, 941, (h, w), dtype=torch.int32, device="cuda", generator=g) << (16 - bits)).to(torch.int16))
    return out


def algorithmic_bytes(w, h, bits, batch):
    """one luma read per picture + the history plane read and written once per batch"""
    return batch * w * h * (1 if bits == 8 else 2) + 2 * w * h * 2


def run(iters, repeats, batch=128):
    tm.init_hip(0)
    res = {}
    for name, w, h, layout, bits, content in CASES:
        pics = surfaces(w, h, bits, DISTINCT, 1, content)
        torch.cuda.synchronize()
        with tm.Siti(w, h, layout, bits, batch=batch) as m:
            def step():  # every compute takes its slots' pictures anew (device tensors: descriptors only, no copy)
                for s in range(batch):
                    m.set_frame(s, pics[(s * 5) % DISTINCT])
                m.compute(batch)
            step()  # warm-up
            step()
            rates = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _ in range(iters):
                    step()
                rates.append(batch * iters / (time.perf_counter() - t0))
            res[name] = {"pictures_per_s": statistics.median(rates), "pictures_per_s_min": min(rates), "pictures_per_s_max": max(rates),
                         "repeats": repeats, "iters": iters, "w": w, "h": h, "layout": layout, "bits": bits, "content": content, "batch": batch,
                         "bytes_per_batch": algorithmic_bytes(w, h, bits, batch), "mem_mib": m.mem_usage() >> 20}
    return res


def kernel_times(iters):
    """calls, mean / min / max ns of k_siti per case, from rocprofv3 over a child run of this script (one case per child)"""
    out = {}
    for name, *_ in CASES:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "si", "--",
                   sys.executable, os.path.abspath(__file__), "--child", name, "--iters", str(iters), "--repeats", "1", "--no-prof"]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                raise RuntimeError(f"rocprofv3 failed ({p.returncode}): {p.stderr[-2000:]}")
            stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not stats:
                raise RuntimeError("rocprofv3 wrote no kernel_stats.csv: " + " ".join(glob.glob(os.path.join(d, "**"), recursive=True)[:20]))
            for row in csv.DictReader(open(stats[0])):
                if "k_siti" in row["Name"]:
                    out[name] = {"calls": int(row["Calls"]), "mean_ns": float(row["AverageNs"]), "min_ns": float(row["MinNs"]),
                                 "max_ns": float(row["MaxNs"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
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
    prof = {} if a.no_prof else kernel_times(10)
    for name, r in res.items():
        k = prof.get(name)
        if k:
            r["kernel_us"] = k["mean_ns"] / 1e3
            r["kernel_us_min"] = k["min_ns"] / 1e3
            r["kernel_us_max"] = k["max_ns"] / 1e3
            r["kernel_calls"] = k["calls"]
            r["kernel_fraction_of_8TBps"] = r["bytes_per_batch"] / (k["mean_ns"] * 1e-9) / HBM_PEAK
        print(json.dumps({"case": name, **r}), flush=True)


if __name__ == "__main__":
    main()
