"""The host handle of pkt_meter_* under AddressSanitizer + UndefinedBehaviorSanitizer (no GPU).

tests/cpp/meter_host_san.cpp is a stand-alone program that drives pkt_meter_create_host / pkt_meter_batch / _reset /
_export (packet-rs_amd/csrc/pktgpu_host.cpp with pktgpu_meter.hpp: the refill, the decision, the DSCP stores and the
refusals the kernels share), every array a heap block of its exact size, packets at every alignment 0..15 with the last
packet ending at the slab's last byte, forged chain columns (an offset past the packet, n_hdrs of 255), every
NULL-output combination with and without PKT_METER_MARK, the largest and the smallest adjust, and the refusals.  Built
here with g++ -fsanitize=address,undefined, the way test_nat_sanitizers.py builds its program, and run directly; any
report fails the run.
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
    exe = os.path.join(OUT, "meter_host_asan")
    subprocess.run(["g++", "-std=c++17", "-Wall", *SAN, "-static-libasan", "-o", exe,
                    os.path.join(REPO, "tests", "cpp", "meter_host_san.cpp"),
                    os.path.join(REPO, "packet-rs_amd", "csrc", "pktgpu_host.cpp"), "-lpthread"], check=True)
    return exe


def test_meter_host_under_asan_ubsan():
    exe = build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "meter OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
