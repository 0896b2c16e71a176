"""The call record of the two-phase device calls (csrc/gk_calls.h: GkCall) owns what it took: tests/asan/call_record.cpp,
a stand-alone program with its own pool, transfers and result ring, is built for the host with AddressSanitizer and
UBSan and run.  It fails an enqueue at every step and lets the record go out of scope (no block out, no delivery left
pointing into it, the next wait clean), runs the good path on a reused and on a moved record (no cancel, no wait of the
record's own), and both sides of the limit above which a result, or a parameter block, does not go through a ring.  The
shape of a blocking entry point -- the record on its stack, deliveries into the caller's arrays and into a local declared
before it -- is failed at every step in the same way."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kir_graph_amd", "csrc")


def test_call_record_owns_its_blocks_and_its_delivery(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the ownership rules of the call record have no other check"
    exe = str(tmp_path / "call_record")
    # the sanitizer runtimes are linked into the executable: compiler and program run in the environment as it is
    cmd = [hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", f"-I{ROOT}/include", f"-I{CSRC}", "-x", "hip",
           f"{ROOT}/tests/asan/call_record.cpp", "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.stdout[-3000:], res.stderr[-3000:])
    assert "call record: ok" in res.stdout
