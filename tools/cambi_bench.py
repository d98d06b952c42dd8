"""CAMBI throughput of libturbometrics_cambi.so from HBM-resident luma planes (torch device tensors, TM_MEM_DEVICE), batch 128, at 1080p
8-bit and 2160p high-aligned 10-bit, each on NOISE (the mask is almost empty: the c-value kernel skips nearly every window) and on a
dark STAIRCASE of one-code steps 40 pixels wide with a per-picture offset (the mask is full and every pixel is below the visibility
thresholds: the c-value kernel at its worst).  Prints one JSON line per case: pictures/s (wall clock over whole computes, results on
the host; the median and the spread of --repeats windows) and every kernel's time per batch from a `rocprofv3 --kernel-trace --stats`
run of this script in a child process of its own.

    python tools/cambi_bench.py [--iters N] [--repeats R] [--batch B] [--no-prof]
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

SHAPES = [("1080p_y8", 1920, 1080, "y8", 8), ("2160p_y16_msb", 3840, 2160, "y16_msb", 10)]
CASES = [(f"{n}_{c}", w, h, lay, b, c) for n, w, h, lay, b in SHAPES for c in ("noise", "stairs")]
KERNELS = ("k_cambi_ingest", "k_cambi_mask", "k_cambi_mode", "k_cambi_cvalues", "k_cambi_pool")
DISTINCT = 16  # distinct device pictures a batch cycles through


def surfaces(w, h, bits, content, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.arange(w, dtype=torch.int32, device="cuda").repeat(h, 1)
    out = []
    for i in range(n):
        if content == "stairs":  # 10-bit codes 100 + i + x / 40, all at or below 178 + 40: dark, one code per step
            v = (100 + i + x // 40) if bits == 10 else (25 + i + x // 40)
        else:
            v = torch.randint(0, 1 << bits, (h, w), dtype=torch.int32, device="cuda", generator=g)
        out.append(v.to(torch.uint8) if bits == 8 else (v << (16 - bits)).to(torch.int16))
    return out


def run(iters, repeats, batch):
    tm.init_hip(0)
    res = {}
    for name, w, h, layout, bits, content in CASES:
        pics = surfaces(w, h, bits, content, DISTINCT, 1)
        torch.cuda.synchronize()
        with tm.Cambi(w, h, layout, bits, batch=batch) as c:
            def step():  # every compute takes its slots' pictures anew (device tensors: descriptors only, no copy)
                for k in range(batch):
                    c.set_frame(k, pics[(k * 5) % DISTINCT])
                c.compute(batch)
            step()  # warm-up
            step()
            f = c.frames(1)[0]
            assert (f.cambi > 0) == (content == "stairs"), f
            rates = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _ in range(iters):
                    step()
                rates.append(batch * iters / (time.perf_counter() - t0))
            res[name] = {"pictures_per_s": statistics.median(rates), "pictures_per_s_min": min(rates), "pictures_per_s_max": max(rates),
                         "repeats": repeats, "iters": iters, "w": w, "h": h, "layout": layout, "bits": bits, "content": content, "batch": batch,
                         "window": c.window, "cambi_of_slot_0": f.cambi, "mem_mib": c.mem_usage() >> 20}
    return res


def kernel_times(iters, batch):
    """calls and total / mean / min / max ns of every CAMBI kernel per case, from rocprofv3 over a child run of this script (one case
    per child)"""
    out = {}
    for name, *_ in CASES:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "cb", "--",
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
            if kn in k:  # time per batch: all launches of the kernel in one compute (five scales; four layouts of the ingest)
                r[kn + "_ms_per_batch"] = k[kn]["total_ns"] / n / 1e6
                r[kn + "_launch_ms_min"] = k[kn]["min_ns"] / 1e6
                r[kn + "_launch_ms_max"] = k[kn]["max_ns"] / 1e6
        if "k_cambi_cvalues" in k:
            r["cvalues_pictures_per_s"] = r["batch"] / (k["k_cambi_cvalues"]["total_ns"] / n * 1e-9)
        print(json.dumps({"case": name, **r}), flush=True)


if __name__ == "__main__":
    main()
