"""MDSI throughput of libturbometrics_mdsi.so from HBM-resident inputs (torch device tensors, TM_MEM_DEVICE), batch 128, at 1080p NV12
(8-bit, factor 4) and 2160p P016 (10-bit, factor 8), with the map read-back off and on (TM_MDSI_MAPS: the kernels form the map either
way).  Prints one JSON line per case and appends it to profiles/mdsi_bench.log: pairs/s (wall clock over whole computes, results on the
host: the median of 3 windows of --iters steps, min and max beside it), the mean times of k_mdsi, k_mdsi_dev and the finish kernel from a
`rocprofv3 --kernel-trace --stats` run of this script in a child process (no counters in that run; the cases with maps off), and the
fraction of 8 TB/s that the bytes a launch MUST move -- the luma and chroma samples of both pictures once, the map written once and
read once, the cells -- make of the kernels' time.

    python tools/mdsi_bench.py [--iters N] [--no-prof]
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

SIZES = [("1080p_nv12", 1920, 1080, "nv12", 8), ("2160p_p016", 3840, 2160, "p016", 10)]
CASES = [(f"{n}{'_map' if m else ''}", w, h, layout, bits, m) for n, w, h, layout, bits in SIZES for m in (False, True)]
HBM_PEAK = 8e12


def surfaces(w, h, layout, bits, n, seed):
    """n distinct device pictures (Y, CbCr) of random limited-range samples"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    s_ = 1 << (bits - 8)
    out = []
    for _ in range(n):
        y = torch.randint(16 * s_, 236 * s_, (h, w), dtype=torch.int32, device="cuda", generator=g)
        c = torch.randint(16 * s_, 241 * s_, ((h + 1) // 2, 2 * ((w + 1) // 2)), dtype=torch.int32, device="cuda", generator=g)
        if layout == "nv12":
            out.append((y.to(torch.uint8), c.to(torch.uint8)))
        else:
            out.append(((y << (16 - bits)).to(torch.int16), (c << (16 - bits)).to(torch.int16)))
    return out


def algorithmic_bytes(w, h, bits):
    """the luma and the interleaved chroma plane of both pictures read once; the f32 map written once and read once; the cells (24 bytes
    per tile of 32 x 16 decimated positions and per chunk of 2048 map values)"""
    bps = 1 if bits == 8 else 2
    f = tm.mdsi.factor(w, h)
    wd, hd = -(-w // f), -(-h // f)
    return 2 * (w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)) * bps + 2 * 4 * wd * hd + 24 * (-(-wd // 32) * -(-hd // 16) + -(-wd * hd // 2048))


def run(iters, batch=128, windows=3):
    tm.init_hip(0)
    res = {}
    for name, w, h, layout, bits, maps in CASES:
        refs, diss = surfaces(w, h, layout, bits, 8, 1), surfaces(w, h, layout, bits, 8, 2)
        torch.cuda.synchronize()
        with tm.Mdsi(w, h, layout, bits, matrix="bt709", factor=0, batch=batch, maps=maps) as x:
            def step():  # every compute takes its slots' pairs anew (device tensors: descriptors only, no copy)
                for s in range(batch):
                    x.set_pair(s, refs[s % 8], diss[(s * 3) % 8])
                x.compute(batch)
            step()  # warm-up
            rates = []
            for _ in range(windows):
                t0 = time.perf_counter()
                for _ in range(iters):
                    step()
                rates.append(batch * iters / (time.perf_counter() - t0))
            rates.sort()
            res[name] = {"pairs_per_s": rates[len(rates) // 2], "pairs_per_s_min": rates[0], "pairs_per_s_max": rates[-1], "windows": windows, "steps": iters, "w": w, "h": h, "layout": layout, "bits": bits,
                         "factor": x.factor, "maps": maps, "batch": batch, "bytes_per_pair": algorithmic_bytes(w, h, bits), "mem_mib": x.mem_usage() >> 20}
    return res


def kernel_times(iters):
    """mean ns of k_mdsi / k_mdsi_dev / the finish kernel per case with maps off, from rocprofv3 over a child run of this script (one case per
    child)"""
    out = {}
    for name, *_, maps in CASES:
        if maps:
            continue
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "mdsi", "--", sys.executable, os.path.abspath(__file__),
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
                if "k_mdsi_finish" in row["Name"]:
                    k["finish"] = {"calls": int(row["Calls"]), "mean_ns": float(row["AverageNs"])}
                elif "k_mdsi_dev" in row["Name"]:
                    k["dev"] = {"calls": int(row["Calls"]), "mean_ns": float(row["AverageNs"])}
                elif "k_mdsi" in row["Name"]:
                    k["blocks"] = {"calls": int(row["Calls"]), "mean_ns": float(row["AverageNs"])}
            out[name] = k
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        global CASES
        CASES = [c for c in CASES if c[0] == a.child]
        run(a.iters, windows=1)
        return
    res = run(a.iters)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    log = open(os.path.join(ROOT, "profiles", "mdsi_bench.log"), "a")
    for name, r in res.items():
        print(json.dumps({"case": name, "wall_clock_only": True, **r}), flush=True)
    prof = {} if a.no_prof else kernel_times(2)
    for name, r in res.items():
        k = prof.get(name, {}).get("blocks")
        if k:
            bytes_launch = r["bytes_per_pair"] * r["batch"]
            r["tile_kernel_us"] = k["mean_ns"] / 1e3
            r["finish_kernel_us"] = prof[name].get("finish", {}).get("mean_ns", float("nan")) / 1e3
            r["dev_kernel_us"] = prof[name].get("dev", {}).get("mean_ns", float("nan")) / 1e3
            r["kernels_fraction_of_8TBps"] = bytes_launch / ((k["mean_ns"] + prof[name].get("dev", {}).get("mean_ns", 0.0)) * 1e-9) / HBM_PEAK
        line = json.dumps({"case": name, **r})
        print(line)
        log.write(line + "\n")
    log.close()


if __name__ == "__main__":
    main()
