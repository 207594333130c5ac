"""rewrite_cases' yardstick (Python integers) against the C oracle (oracle/pkt_oracle.c): two independent readings
of the reference's getters, setters and IPv4 checksum, checked against each other on every case that
test_rewrite_device.py runs on the GPU; and every case's floor: the check that the case reaches the path it is
built for.  No GPU."""
import numpy as np
import pytest

import oracle

import rewrite_cases as R


def test_yardstick_pins():
    R.pin_yardstick()


def test_table_is_what_the_device_file_runs():
    assert len(R.TABLE) == 6 * 8 + 3 + 2 + 3 + 2 * 10 + 4 + 2 + 2 * 6 + 2
    assert all(set(calls) <= {R.GET, R.SET, R.SET0, R.SET1, R.UPD0, R.UPD1} for _, calls in R.TABLE.values())


@pytest.mark.parametrize("name", list(R.TABLE))
def test_floor(name):
    c = R.case(name)
    assert c["floor"] is not None
    c["floor"]()


@pytest.mark.parametrize("name,call", R.CALLS)
def test_yardstick_equals_oracle(name, call):
    c = R.case(name)
    b, ch = c["batch"], c["chain"]
    kw = R.batch_kw(b)
    want = R.expected(name, call)
    if call == R.GET:
        vals, found = oracle.extract_fields(b["slab"], b["n"], ch, c["specs"], **kw)
        for k, sp in enumerate(c["specs"]):
            assert np.array_equal(vals[k], want[0][k]), (k, sp)
            assert np.array_equal(found[k], want[1][k]), (k, sp)
        return
    slab = b["slab"].copy()
    if call.startswith("set"):
        oracle.set_fields(slab, b["n"], ch, c["specs"], c["values"], **kw)
    if call[-1] in "01":
        oracle.ipv4_update_checksum(slab, b["n"], ch, int(call[-1]), **kw)
    bad = np.flatnonzero(slab != want)
    assert bad.size == 0, (bad[:8], slab[bad[:8]], want[bad[:8]])
    assert not np.array_equal(want, b["slab"]), "the call changes nothing"


@pytest.mark.parametrize("stride", R.CSUM_STRIDES)
@pytest.mark.parametrize("n", R.CSUM_N)
def test_checksum_batch_cases(n, stride):
    buf, want, differ, hs = R.csum_case(n, stride)
    assert buf.size == n * stride and [oracle.ipv4_checksum(h) for h in hs] == want.tolist()
    if n >= 63:
        assert differ >= n / 8 and differ < n   # Q1 and RFC 1071 differ on some headers and agree on others


def test_broadcast_cases():
    for length, stride in R.BCAST:
        src, want = R.bcast_case(length, stride, 3)
        assert want.size == 3 * stride and want[stride:stride + length].tobytes() == src and not want[2 * stride + length:].any()
    length, stride, n = R.BCAST_BIG
    assert n * stride // 16 > 256 * 64 * 256 and stride % 16 == 0
