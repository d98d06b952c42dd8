"""Histogram throughput of libturbometrics_scene.so from HBM-resident luma planes (torch device tensors, TM_MEM_DEVICE), batch 128, at
1080p 8-bit and 2160p high-aligned 10-bit, each on NOISE and on a FLAT picture (every sample in one bin: the worst case of a
histogram's atomics).  Prints one JSON line per case: pictures/s (wall clock over whole computes, results on the host; the median and
the spread of --repeats windows), the kernels' mean times from a `rocprofv3 --kernel-trace --stats` run of this script in a child
process of its own, and the fraction of 8 TB/s that the luma bytes of a launch, each counted once, make of the k_scene_hist time.

    python tools/scene_bench.py [--iters N] [--repeats R] [--no-prof]
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
CASES = [(f"{n}_{c}", w, h, lay, b, c) for n, w, h, lay, b in SHAPES for c in ("noise", "flat")]
HBM_PEAK = 8e12
DISTINCT = 32  # distinct device pictures a batch cycles through


def surfaces(w, h, bits, content, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for i in range(n):
        if content == "flat":  # one value per picture, another one for the next picture
            v = torch.full((h, w), 16 + (i * 37) % 220, dtype=torch.int32, device="cuda") << (bits - 8)
        else:
            v = torch.randint(0, 1 << bits, (h, w), dtype=torch.int32, device="cuda", generator=g)
        out.append(v.to(torch.uint8) if bits == 8 else (v << (16 - bits)).to(torch.int16))
    return out


def run(iters, repeats, batch=128):
    tm.init_hip(0)
    res = {}
    for name, w, h, layout, bits, content in CASES:
        pics = surfaces(w, h, bits, content, DISTINCT, 1)
        torch.cuda.synchronize()
        with tm.Scene(w, h, layout, bits, batch=batch) as s:
            def step():  # every compute takes its slots' pictures anew (device tensors: descriptors only, no copy)
                for k in range(batch):
                    s.set_frame(k, pics[(k * 5) % DISTINCT])
                s.compute(batch)
            step()  # warm-up
            step()
            hist = s.frames(1)[0].hist
            assert int(hist.astype("uint64").sum()) == w * h and (content != "flat" or int(hist.max()) == w * h)
            rates = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _ in range(iters):
                    step()
                rates.append(batch * iters / (time.perf_counter() - t0))
            res[name] = {"pictures_per_s": statistics.median(rates), "pictures_per_s_min": min(rates), "pictures_per_s_max": max(rates),
                         "repeats": repeats, "iters": iters, "w": w, "h": h, "layout": layout, "bits": bits, "content": content, "batch": batch,
                         "bytes_per_batch": batch * w * h * (1 if bits == 8 else 2), "mem_mib": s.mem_usage() >> 20}
    return res


def kernel_times(iters):
    """calls, mean / min / max ns of k_scene_hist and k_scene_finish per case, from rocprofv3 over a child run of this script (one
    case per child)"""
    out = {}
    for name, *_ in CASES:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "sc", "--",
                   sys.executable, os.path.abspath(__file__), "--child", name, "--iters", str(iters), "--repeats", "1", "--no-prof"]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                raise RuntimeError(f"rocprofv3 failed ({p.returncode}): {p.stderr[-2000:]}")
            stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not stats:
                raise RuntimeError("rocprofv3 wrote no kernel_stats.csv: " + " ".join(glob.glob(os.path.join(d, "**"), recursive=True)[:20]))
            for row in csv.DictReader(open(stats[0])):
                for k in ("k_scene_hist", "k_scene_finish"):
                    if k in row["Name"]:
                        out.setdefault(name, {})[k] = {"calls": int(row["Calls"]), "mean_ns": float(row["AverageNs"]), "min_ns": float(row["MinNs"]),
                                                      "max_ns": float(row["MaxNs"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
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
        k = prof.get(name, {})
        if "k_scene_hist" in k:
            hk = k["k_scene_hist"]
            r["kernel_us"] = hk["mean_ns"] / 1e3
            r["kernel_us_min"] = hk["min_ns"] / 1e3
            r["kernel_us_max"] = hk["max_ns"] / 1e3
            r["kernel_calls"] = hk["calls"]
            r["kernel_fraction_of_8TBps"] = r["bytes_per_batch"] / (hk["mean_ns"] * 1e-9) / HBM_PEAK
        if "k_scene_finish" in k:
            r["finish_us"] = k["k_scene_finish"]["mean_ns"] / 1e3
        print(json.dumps({"case": name, **r}), flush=True)
    for shape, *_ in SHAPES:
        a_, b_ = res.get(shape + "_flat", {}), res.get(shape + "_noise", {})
        if "kernel_us" in a_ and "kernel_us" in b_:
            print(json.dumps({"shape": shape, "flat_over_noise_kernel_time": a_["kernel_us"] / b_["kernel_us"]}), flush=True)


if __name__ == "__main__":
    main()
