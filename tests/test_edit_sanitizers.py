"""pkt_edit_host under AddressSanitizer + UndefinedBehaviorSanitizer (no GPU).

tests/cpp/edit_host_san.cpp is a stand-alone program that drives pkt_edit_host
(packet-rs_amd/csrc/pktgpu_host.cpp) over the strip and the insert at every pair of source and
destination alignments, rooms one byte short and exact, destination offsets past dst_len, the
16-header list, and chain columns that are no parse of the batch, every slab, dst and hdr_data a heap
block of exactly its length.  Built here with g++ -fsanitize=address,undefined, the way
test_compare_sanitizers.py builds compare_host_san.cpp, and run directly; any report fails the run.
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
    exe = os.path.join(OUT, "edit_host_asan")
    subprocess.run(["g++", "-std=c++17", "-Wall", *SAN, "-static-libasan", "-o", exe,
                    os.path.join(REPO, "tests", "cpp", "edit_host_san.cpp"),
                    os.path.join(REPO, "packet-rs_amd", "csrc", "pktgpu_host.cpp"), "-lpthread"], check=True)
    return exe


def test_edit_host_under_asan_ubsan():
    exe = build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "edit OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
