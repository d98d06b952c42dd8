"""HaarPSI throughput of libturbometrics_haarpsi.so from HBM-resident inputs (torch device tensors, TM_MEM_DEVICE), batch 128, at 1080p
8-bit and 2160p high-aligned 10-bit, with the local similarity maps off and on.  Prints one JSON line per case and appends it to
profiles/haarpsi_bench.log: pairs/s (wall clock over whole computes, results on the host: the median of 3 windows of --iters steps, min
and max beside it), the mean time of k_haarpsi and k_haarpsi_finish from a `rocprofv3 --kernel-trace --stats` run of this script in a
child process (no counters in that run), and the fraction of 8 TB/s that the bytes a launch MUST move -- both lumas once, the tiles'
cells written once, with maps on the f32 map of the decimated plane written once -- make of k_haarpsi's time.  GMSD reads the same
bytes: profiles/gmsd_bench.log is the figure to set beside these.

    python tools/haarpsi_bench.py [--iters N] [--no-prof]
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

CASES = [("1080p_y8", 1920, 1080, "y8", 8, False), ("1080p_y8_maps", 1920, 1080, "y8", 8, True),
         ("2160p_y16_msb", 3840, 2160, "y16_msb", 10, False), ("2160p_y16_msb_maps", 3840, 2160, "y16_msb", 10, True)]
HBM_PEAK = 8e12


def surfaces(w, h, layout, bits, n, seed):
    """n distinct device luma planes of random samples"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for _ in range(n):
        if layout == "y8":
            out.append(torch.randint(16, 236, (h, w), dtype=torch.int32, device="cuda", generator=g).to(torch.uint8))
        else:
            out.append((torch.randint(64, 941, (h, w), dtype=torch.int32, device="cuda", generator=g) << (16 - bits)).to(torch.int16))
    return out


def algorithmic_bytes(w, h, bits, maps):
    """both lumas read once; the cells (16 bytes per tile of 64 x 32 decimated positions) written once; with maps, 4 bytes per position"""
    bps = 1 if bits == 8 else 2
    w2, h2 = (w + 1) // 2, (h + 1) // 2
    return 2 * w * h * bps + 16 * -(-w2 // 64) * -(-h2 // 32) + (4 * w2 * h2 if maps else 0)


def run(iters, batch=128, windows=3):
    tm.init_hip(0)
    res = {}
    for name, w, h, layout, bits, maps in CASES:
        refs, diss = surfaces(w, h, layout, bits, 8, 1), surfaces(w, h, layout, bits, 8, 2)
        torch.cuda.synchronize()
        with tm.HaarPsi(w, h, layout, bits, batch=batch, maps=maps) as x:
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
            res[name] = {"pairs_per_s": rates[len(rates) // 2], "pairs_per_s_min": rates[0], "pairs_per_s_max": rates[-1], "windows": windows, "steps": iters, "w": w, "h": h, "layout": layout, "bits": bits, "maps": maps, "batch": batch,
                         "bytes_per_pair": algorithmic_bytes(w, h, bits, maps), "mem_mib": x.mem_usage() >> 20}
    return res


def kernel_times(iters):
    """mean ns of k_haarpsi / k_haarpsi_finish per case, from rocprofv3 over a child run of this script (one case per child)"""
    out = {}
    for name, *_ in CASES:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "haarpsi", "--", sys.executable, os.path.abspath(__file__),
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
                if "k_haarpsi" in row["Name"]:
                    k["finish" if "finish" in row["Name"] else "tiles"] = {"calls": int(row["Calls"]), "mean_ns": float(row["AverageNs"])}
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
        run(a.iters, windows=1)
        return
    res = run(a.iters)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    log = open(os.path.join(ROOT, "profiles", "haarpsi_bench.log"), "a")
    for name, r in res.items():
        print(json.dumps({"case": name, "wall_clock_only": True, **r}), flush=True)
    prof = {} if a.no_prof else kernel_times(5)
    for name, r in res.items():
        k = prof.get(name, {}).get("tiles")
        if k:
            bytes_launch = r["bytes_per_pair"] * r["batch"]
            r["tile_kernel_us"] = k["mean_ns"] / 1e3
            r["finish_kernel_us"] = prof[name].get("finish", {}).get("mean_ns", float("nan")) / 1e3
            r["tile_kernel_fraction_of_8TBps"] = bytes_launch / (k["mean_ns"] * 1e-9) / HBM_PEAK
        line = json.dumps({"case": name, **r})
        print(line)
        log.write(line + "\n")
    log.close()


if __name__ == "__main__":
    main()
