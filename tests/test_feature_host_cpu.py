"""The host core the ten feature libraries share (turbo-metrics_amd/csrc/tm_feature_host.h), without a GPU: tests/host/feature_host_test.cpp
compiles the header with g++ against the fake hip_runtime.h under tests/host/fake_hip and runs as a stand-alone program under
AddressSanitizer and UBSan (nothing is loaded into Python).  What it asserts is listed at the top of the .cpp."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "turbo-metrics_amd", "csrc")
NAMES = ("xpsnr", "motion", "vif", "adm", "scene", "cambi", "flip", "yuv", "hvs", "ciede")


def test_the_shared_host_core_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "feature_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "tests", "host", "fake_hip"), "-o", exe, os.path.join(ROOT, "tests", "host", "feature_host_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout == "feature host ok\n", (out.stdout, out.stderr)


def test_every_feature_library_uses_it_and_keeps_no_copy():
    for name in NAMES:
        src = open(os.path.join(CSRC, f"tm_{name}.hip")).read()
        assert '#include "tm_feature_host.h"' in src and "TmFeatureHost c;" in src, name
        assert not re.search(r"#define\s+\w*(CHK|QUEUED)\b", src), name  # the private ?CHK / ?QUEUED macros are gone
        for call in ("hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree(", "hipStreamCreateWithFlags(", "hipStreamDestroy(", "hipGetDevice("):
            assert call not in src, (name, call)
        # compute_async: the first queued operation is checked plainly, everything behind it through the drain
        body = src[src.index(f"int tm_{name}_compute_async("):]
        body = body[:body.index("\n}\n")]
        assert body.count("TMFH_CHK(") == 1 and body.count("TMFH_CHK_QUEUED(") >= 3, name
        assert body.index("TMFH_CHK(") < body.index("TMFH_CHK_QUEUED("), name
    core = open(os.path.join(CSRC, "tm_feature_host.h")).read()
    assert "__global__" not in core and "<<<" not in core and 'extern "C"' not in core  # host code only, no entry points
    assert re.findall(r'#include "([^"]+)"', core) == ["../../include/turbo_metrics_hip.h"]
