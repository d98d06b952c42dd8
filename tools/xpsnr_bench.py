"""XPSNR throughput of libturbometrics_xpsnr.so from HBM-resident inputs (torch device tensors, TM_MEM_DEVICE), batch 128, at 1080p NV12
and 2160p P016.  Prints one JSON line per case: pairs/s (wall clock over whole computes, results on the host), the block kernel's mean
time from a `rocprofv3 --kernel-trace --stats` run of this script in a child process, and the fraction of 8 TB/s that the algorithmic
bytes of a launch -- reference and distorted luma + chroma, plus the m1 (and, second order, m2) luma the history adds -- make of that
kernel time.

    python tools/xpsnr_bench.py [--iters N] [--no-prof]
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import torch  # noqa: F401  (torch's HIP runtime first, like bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tm_pkg import tm  # noqa: E402

CASES = [("1080p_nv12", 1920, 1080, "nv12", 8), ("2160p_p016", 3840, 2160, "p016", 10)]
HBM_PEAK = 8e12


def surfaces(w, h, layout, bits, n, seed):
    """n distinct device pictures (Y, CbCr) of random samples"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    out = []
    for _ in range(n):
        if layout == "nv12":
            y = torch.randint(16, 236, (h, w), dtype=torch.int32, device="cuda", generator=g).to(torch.uint8)
            c = torch.randint(16, 241, (ch, 2 * cw), dtype=torch.int32, device="cuda", generator=g).to(torch.uint8)
        else:
            sh = 16 - bits
            y = (torch.randint(64, 941, (h, w), dtype=torch.int32, device="cuda", generator=g) << sh).to(torch.int16)
            c = (torch.randint(64, 961, (ch, 2 * cw), dtype=torch.int32, device="cuda", generator=g) << sh).to(torch.int16)
        out.append((y, c))
    return out


def algorithmic_bytes(w, h, bits, second):
    bps = 1 if bits == 8 else 2
    pic = (w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)) * bps
    return 2 * pic + w * h * bps * (2 if second else 1)


def run(iters, batch=128, fps=(30, 1)):
    tm.init_hip(0)
    res = {}
    for name, w, h, layout, bits in CASES:
        refs, diss = surfaces(w, h, layout, bits, 8, 1), surfaces(w, h, layout, bits, 8, 2)
        torch.cuda.synchronize()
        with tm.Xpsnr(w, h, layout, bits, fps=fps, batch=batch) as x:
            def step():  # every compute takes its slots' pictures anew (device tensors: descriptors only, no copy)
                for s in range(batch):
                    x.set_pair(s, refs[s % 8], diss[(s * 3) % 8])
                x.compute(batch)
            step()  # warm-up
            t0 = time.perf_counter()
            for _ in range(iters):
                step()
            dt = time.perf_counter() - t0
            res[name] = {"pairs_per_s": batch * iters / dt, "w": w, "h": h, "layout": layout, "bits": bits, "batch": batch,
                         "bytes_per_pair": algorithmic_bytes(w, h, bits, False), "mem_mib": x.mem_usage() >> 20}
    return res


def kernel_times(iters):
    """mean ns of k_xpsnr_blocks / k_xpsnr_finish per case, from rocprofv3 over a child run of this script (one case per child)"""
    out = {}
    for name, *_ in CASES:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "xp", "--", sys.executable, os.path.abspath(__file__),
                   "--child", name, "--iters", str(iters), "--no-prof"]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"rocprofv3 failed ({p.returncode}): {p.stderr[-2000:]}")
            stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not stats:
                raise RuntimeError("rocprofv3 wrote no kernel_stats.csv: " + " ".join(glob.glob(os.path.join(d, "**"), recursive=True)[:20]))
            import csv
            k = {}
            for row in csv.DictReader(open(stats[0])):
                if "xpsnr" in row["Name"]:
                    k["blocks" if "blocks" in row["Name"] else "finish"] = {"calls": int(row["Calls"]), "mean_ns": float(row["AverageNs"])}
            out[name] = k
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        global CASES
        CASES = [c for c in CASES if c[0] == a.child]
        run(a.iters)
        return
    res = run(a.iters)
    for name, r in res.items():
        print(json.dumps({"case": name, "wall_clock_only": True, **r}), flush=True)
    prof = {} if a.no_prof else kernel_times(5)
    for name, r in res.items():
        k = prof.get(name, {}).get("blocks")
        if k:
            bytes_launch = r["bytes_per_pair"] * r["batch"]
            r["block_kernel_us"] = k["mean_ns"] / 1e3
            r["finish_kernel_us"] = prof[name].get("finish", {}).get("mean_ns", float("nan")) / 1e3
            r["block_kernel_fraction_of_8TBps"] = bytes_launch / (k["mean_ns"] * 1e-9) / HBM_PEAK
        print(json.dumps({"case": name, **r}))


if __name__ == "__main__":
    main()
