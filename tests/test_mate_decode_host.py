"""The decoder of a plain mate pair that host and device share (csrc/gk_mate_decode.h) against the host decoder it restates
(csrc/gk_bamread.cpp, csrc/gk_sampack.cpp): tests/asan/mate_decode.cpp, a stand-alone program that builds BAM records in
memory and runs both decoders on every pair, is built for the host with AddressSanitizer and UBSan and run.  DONE implies
the host's bytes, without error, spill or strings; every plain class is DONE and every non-plain class HOST; and the
implication holds over a few thousand single-byte mutations and truncations of plain records on a fixed seed.  The header
is also compiled into a gfx950 code object (tests/asan/mate_decode_device.hip; nothing runs): it must stay device code."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kir_graph_amd", "csrc")


def test_shared_decoder_agrees_with_the_host_decoder(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the shared decoder has no other host-side check"
    exe = str(tmp_path / "mate_decode")
    # the sanitizer runtimes are linked into the executable: compiler and program run in the environment as it is
    cmd = [hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", f"-I{ROOT}/include", f"-I{CSRC}", "-x", "hip",
           f"{ROOT}/tests/asan/mate_decode.cpp", f"{CSRC}/gk_sampack.cpp", "-o", exe, "-lz", "-ldl", "-lpthread"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-3000:], res.stderr[-3000:])
    assert "mate decode: ok" in res.stdout


def test_shared_decoder_compiles_for_the_device(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-O3", f"-I{ROOT}/include", f"-I{CSRC}", "-c",
           f"{ROOT}/tests/asan/mate_decode_device.hip", "-o", str(tmp_path / "mate_decode_device.co")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    assert os.path.getsize(tmp_path / "mate_decode_device.co") > 0
