"""pkt_off / pkt_len and the host models that call them under AddressSanitizer + UndefinedBehaviorSanitizer
(no GPU).

tests/cpp/batch_helpers_san.cpp is a stand-alone program that drives the offset rule and the length clamp of
packet-rs_amd/csrc/pktgpu_batch.hpp on the stride form and the indexed form (an offset at and past the slab
end, a length crossing it, a length above 65535, slab_len 0), then pkt_compare_host, pkt_pcap_write_host and
pkt_edit_host on a 3-packet batch whose last packet the slab end cuts, every slab and dst a heap block of
exactly its length and every expected byte written out in the program.  Built here with
g++ -fsanitize=address,undefined, the way test_edit_sanitizers.py builds edit_host_san.cpp, and run directly;
any report fails the run.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "cpp", "build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g"]


def build():
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "batch_helpers_asan")
    subprocess.run(["g++", "-std=c++17", "-Wall", *SAN, "-static-libasan", "-o", exe,
                    os.path.join(REPO, "tests", "cpp", "batch_helpers_san.cpp"),
                    os.path.join(REPO, "packet-rs_amd", "csrc", "pktgpu_host.cpp"), "-lpthread"], check=True)
    return exe


def test_batch_helpers_under_asan_ubsan():
    exe = build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "batch helpers OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
