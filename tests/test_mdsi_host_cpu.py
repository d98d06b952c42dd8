"""The host file of libturbometrics_mdsi.so (turbo-metrics_amd/csrc/tm_mdsi.hip), without a GPU: tests/host/mdsi_host_test.cpp compiles
it with g++ against the fake hip_runtime.h under tests/host/fake_hip and runs as a stand-alone program under AddressSanitizer and UBSan
(nothing is loaded into Python).  What it asserts is listed at the top of the .cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_mdsi_host_file_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "mdsi_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-enum-compare", "-x", "c++",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "tests", "host", "fake_hip"), "-I" + os.path.join(ROOT, "tests", "emul"),
                           "-o", exe, os.path.join(ROOT, "tests", "host", "mdsi_host_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout == "mdsi host ok\n", (out.stdout, out.stderr)


def test_the_library_uses_the_shared_host_core_like_the_other_fourteen():
    src = open(os.path.join(ROOT, "turbo-metrics_amd", "csrc", "tm_mdsi.hip")).read()
    assert '#include "tm_feature_host.h"' in src and "TmFeatureHost c;" in src
    for call in ("hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree(", "hipStreamCreateWithFlags(", "hipStreamDestroy(", "hipGetDevice("):
        assert call not in src, call
    body = src[src.index("int tm_mdsi_compute_async("):]
    body = body[:body.index("\n}\n")]
    assert body.count("TMFH_CHK(") == 1 and body.count("TMFH_CHK_QUEUED(") == 5 and body.index("TMFH_CHK(") < body.index("TMFH_CHK_QUEUED(")
    wait = src[src.index("int tm_mdsi_set_frame("):]
    wait = wait[:wait.index("\n}\n")]
    assert wait.index("tmfh_sync(&x->c)") < wait.index("tmfh_upload_420(")  # a host picture waits for a pending compute first
