"""The split route of the ingest -- a decoder of plain pairs between pairing and decoding, the packer decoding the
rest (csrc/gk_ingest.h: gk_bam_pack_with; csrc/gk_sampack.cpp: gk_packer_decode_subset) -- against gk_bam_pack:
tests/asan/ingest_split.cpp, a stand-alone program that builds BAM records in memory, is built for the host with
AddressSanitizer and UBSan and run.  Whatever the split of the verdicts, the packer holds the host route's records,
pair_lines, counts, strings, spill and error; the empty subset is passed as a null pointer and as a pointer, each with
count 0; a subset that is not strictly ascending is refused."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kir_graph_amd", "csrc")


def test_split_route_leaves_what_the_host_route_leaves(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the split route has no other host-side check"
    exe = str(tmp_path / "ingest_split")
    # the sanitizer runtimes are linked into the executable: compiler and program run in the environment as it is
    cmd = [hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", f"-I{ROOT}/include", f"-I{CSRC}", "-x", "hip",
           f"{ROOT}/tests/asan/ingest_split.cpp", f"{CSRC}/gk_sampack.cpp", "-o", exe, "-lz", "-ldl", "-lpthread"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-3000:], res.stderr[-3000:])
    assert "ingest split: ok" in res.stdout
