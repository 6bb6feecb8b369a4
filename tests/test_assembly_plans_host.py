"""The assembly planners of slepc_amd/csrc/ks_csr.cpp under a sanitizer: tests/host/assembly_plans.cpp, a program of its own built together with
ks_csr.cpp with -fsanitize=address,undefined, makes the split and the halo plan of small worlds (ranks with no rows, one row, no ghosts) rank by rank
and checks them by brute force, and walks the binned plan of two integer matrices against a plain CSR product. One build and one run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHECKS = ["4 ranks, 5 0 3 8 rows", "8 ranks with a 0-row and a 1-row rank", "3 ranks, one without ghosts", "rejections",
          "binned n 4096 on 4 CUs", "binned n 4500 on 256 CUs"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("assembly_plans") / "assembly_plans")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-Wall", "-Wno-unknown-pragmas", "-pthread", os.path.join(ROOT, "tests", "host", "assembly_plans.cpp"),
                           os.path.join(ROOT, "slepc_amd", "csrc", "ks_csr.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout.splitlines()


@pytest.mark.parametrize("name", CHECKS)
def test_assembly_plans_under_asan_ubsan(report, name):
    assert any(line == "ok " + name or line.startswith("ok " + name + ":") for line in report), (name, report)
    assert report[-1] == "all ok"
