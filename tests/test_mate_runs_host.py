"""The walk of a mate's M runs that depth_mark, callcov_mark and depthw_mark share (csrc/gk_materuns.h) and the draw that
boot_resample and callboot_draw share (csrc/gk_draw.h), on the host: tests/asan/mate_runs.cpp, a stand-alone program that
builds records in both forms in heap blocks of exactly their size, walks every mate with both walkers and compares the
marks with a restatement of its own, is built for the host with AddressSanitizer and UBSan and run.  Its cases: n_cig 0,
1, 13, 14 and beyond the record (clamped); M / D / I / S mixed; runs that end at, straddle, start at and start beyond the
gene's length; pos0 = 0; wide pairs with n_cig 0, 128 and 200 (clamped), with and without a wide array, in the last slot
and one past it; pair_src of -1, n_pairs - 1 and n_pairs; and a compact mate that ends with its last CIGAR word as the last
record of the buffer.  The draws the program prints are held against tests/boot_reference.py.  Both headers are also
compiled into a gfx950 code object (tests/asan/mate_runs_device.hip; nothing runs): they must stay device code."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import boot_reference  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kir_graph_amd", "csrc")
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the shared walk has no other host-side check"
    exe = str(tmp_path_factory.mktemp("mate_runs") / "mate_runs")
    # the sanitizer runtimes are linked into the executable: compiler and program run in the environment as it is
    cmd = [hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", f"-I{ROOT}/include", f"-I{CSRC}", "-x", "hip",
           f"{ROOT}/tests/asan/mate_runs.cpp", f"{CSRC}/gk_sampack.cpp", "-o", exe, "-lz", "-ldl", "-lpthread"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-3000:], res.stderr[-3000:])
    return res.stdout


def test_both_walkers_mark_what_the_restatement_marks(program_output):
    assert "FAIL" not in program_output, program_output[-3000:]
    assert "mate runs: ok" in program_output


def drawByTheFormula(seed, i, b, g, n):
    """The module docstring of boot_reference in Python integers: for the n that ``boot_reference.draws`` does not take."""
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15 + (b + 1) * 0xBF58476D1CE4E5B9 + (g + 1) * 0x94D049BB133111EB) & M64
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    z ^= z >> 31
    return ((z >> 32) * n) >> 32


def test_shared_draw_gives_the_reference_draws(program_output):
    lines = [tuple(int(x) for x in ln.split()[1:]) for ln in program_output.splitlines() if ln.startswith("draw ")]
    assert len(lines) >= 300
    assert {1, (1 << 32) - 1} <= {n for _, _, _, _, n, _ in lines}
    by_reference = 0
    replicate = {}      # boot_reference.draws makes all n draws of a replicate at once
    for seed, i, b, g, n, j in lines:
        assert 0 <= j < n
        assert j == drawByTheFormula(seed, i, b, g, n), (seed, i, b, g, n)
        if i < n <= 1 << 20:      # ... and takes n < 2^31
            if (seed, g, b, n) not in replicate:
                replicate[seed, g, b, n] = boot_reference.draws(seed, g, b, n)
            assert j == int(replicate[seed, g, b, n][i]), (seed, i, b, g, n)
            by_reference += 1
    assert by_reference >= 100
    # the formula above and the reference are the same numbers where both apply
    ref = boot_reference.draws(12345, 2, 7, 1000)
    assert [drawByTheFormula(12345, i, 7, 2, 1000) for i in range(1000)] == [int(x) for x in ref]
    assert ref.dtype == np.uint64


def test_shared_headers_compile_for_the_device(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-O3", f"-I{ROOT}/include", f"-I{CSRC}", "-c",
           f"{ROOT}/tests/asan/mate_runs_device.hip", "-o", str(tmp_path / "mate_runs_device.co")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    assert os.path.getsize(tmp_path / "mate_runs_device.co") > 0
