"""The pair form of the dictionary row walk (slepc_amd/csrc/ks_dict_pairs.h) on the host: tests/host/dict_pairs_walk.cpp, a program of its own built
with -fsanitize=address,undefined, emulates waves of 64 lanes over x and y of exactly n elements, compares every row bit for bit with the one-row
walk and asks the eligibility rule about matrices it must refuse. One build and one run serve both tests."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WALKS = ["lap3d 4x4x4", "lap3d 6x6x6", "lap3d 4x6x10", "lap3d 2x2x2", "lap2d 4x4", "lap2d 10x12", "27-point 4x4x4", "lap3d 6x6x6 without its last row",
         "lap2d 10x30 (three waves)", "offsets 0, +-1, +-2 (bases 2 apart)", "18 offsets, W 32, n 1001", "W 16 with an odd n",
         "underflow, rows with padding", "underflow, full rows", "underflow, lap3d 6x6x6"]
REFUSED = ["odd stride (lap2d 5x4)", "odd stride (lap3d 5x4x4)", "an offset two past a base's pair", "10 bases", "random values (no pattern form)", "unsorted row"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dict_pairs") / "dict_pairs_walk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", os.path.join(ROOT, "tests", "host", "dict_pairs_walk.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout.splitlines()


def test_pair_walk_stays_inside_x_and_gives_the_row_walks_bits(report):
    for name in WALKS:
        assert any(line.startswith("ok " + name + ":") for line in report), (name, report)
    assert report[-1] == "all ok"
    # the underflow case with full rows does produce results of -0.0, the sign the one-row walk gives them
    assert any("underflow, full rows:" in line and "rows with a result of -0.0" in line and not line.strip().endswith(": 0 rows with a result of -0.0") for line in report)


def test_pair_form_eligibility(report):
    """The issue's case "an offset of +-2 refused" is kept as far as the issue's own rule can refuse it: an offset of exactly +-2 is b = +-2 with d = 0
    (the 2x2x2 Laplacian, which the issue wants accepted, has such offsets), so offsets 0, +-1, +-2 are accepted and walked (WALKS); refused is an entry
    two past a base's pair, offsets 0, +-1, +-3, whose pair at +-2 no row of the matrix reads."""
    for name in REFUSED:
        assert any(line.startswith("ok " + name + " refused:") for line in report), (name, report)
    # what the accepted ones were given: the 7-point stencil five bases with only the centre wide, the 27-point one nine, all wide
    assert any(line.startswith("ok lap3d 6x6x6:") and "5 bases, wide mask 0x4" in line for line in report)
    assert any(line.startswith("ok 27-point 4x4x4:") and "9 bases, wide mask 0x1ff" in line for line in report)
