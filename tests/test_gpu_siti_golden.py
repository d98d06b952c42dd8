"""Without --siti the CLI prints what the parent commit's binary printed, byte for byte: tests/golden/siti_parent_cli.json holds the
parent's stdout for the invocations below on a synthetic Y4M pair, recorded once on an MI355X with
record_parent_cli(<the parent's turbo-metrics>, GOLDEN, <a scratch directory>)."""
import json
import os
import subprocess

import pytest

from tests import siti_util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "turbo-metrics_amd", "bin", "turbo-metrics")
GOLDEN = os.path.join(ROOT, "tests", "golden", "siti_parent_cli.json")
W, H, N = 162, 94, 5

PARENT_CASES = {
    "y4m8_psnr_csv": (8, ["-m", "psnr", "--output", "csv"]),
    "y4m8_psnr_ssim_json": (8, ["-m", "psnr", "-m", "ssim", "--output", "json"]),
    "y4m8_ssimu_jsonl": (8, ["-m", "ssimulacra2", "--batch", "2", "--output", "json-lines"]),
    "y4m8_psnr_motion_csv": (8, ["-m", "psnr", "--motion", "--output", "csv"]),
    "y4m10_motion_scenes_json": (10, ["--motion", "--scenes", "--batch", "3", "--output", "json"]),
    "y4m10_psnr_motion_jsonl": (10, ["-m", "psnr", "--motion", "--output", "json-lines"]),
    "y4m10_xpsnr_default": (10, ["-m", "xpsnr", "-m", "psnr"]),
}


def _cli(*args, cli=CLI):
    out = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def _run_parent_cases(cli, tmp):
    out = {}
    for bits in (8, 10):
        seq = U.sequence(W, H, N, bits, "smooth", seed=bits)
        a, b = os.path.join(str(tmp), f"a{bits}.y4m"), os.path.join(str(tmp), f"b{bits}.y4m")
        U.y4m(a, seq, bits)
        U.y4m(b, [(p * 7 // 8 + 3) % (1 << bits) for p in seq], bits)
        for name, (k, args) in PARENT_CASES.items():
            if k == bits:
                out[name] = _cli(a, b, *args, cli=cli)
    return out


def record_parent_cli(cli, golden, tmp):
    with open(golden, "w") as f:
        json.dump(_run_parent_cases(cli, tmp), f, indent=1, sort_keys=True)
        f.write("\n")


def test_cli_without_siti_is_byte_identical_with_the_parents(tmp_path):
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(PARENT_CASES)
    got = _run_parent_cases(CLI, tmp_path)
    for name in PARENT_CASES:
        assert got[name] == want[name], name
        assert '"si"' not in got[name] and "SI:" not in got[name], name
