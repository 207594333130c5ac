"""Host-side arithmetic of bench.py's roofline objects (no GPU): the line-granular floor."""
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("bench", os.path.join(REPO, "bench.py"))
bench = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bench)


def brute_lines(starts, spans):
    lines = set()
    for s, n in zip(starts, spans):
        n = max(int(n), 1)
        lines.update(range(int(s) // 128, (int(s) + n - 1) // 128 + 1))
    return 128 * len(lines)


def test_line_bytes_fixed_stride():
    n = 1000
    # C2: 42-byte header spans at a 64-byte stride: two packets per line
    assert bench.line_bytes(n, 64, None, np.full(n, 42)) == 64 * n
    # C3: 128-byte slots, headers inside the slot: one line each
    assert bench.line_bytes(n, 128, None, np.full(n, 58)) == 128 * n
    # failed parses (span 0) still count the packet's first line
    assert bench.line_bytes(n, 128, None, np.zeros(n)) == 128 * n


def test_line_bytes_indexed_vs_brute_force():
    rng = np.random.default_rng(7)
    for _ in range(20):
        n = int(rng.integers(1, 300))
        lens = rng.integers(0, 400, n)
        gaps = rng.integers(0, 40, n)
        offs = np.cumsum(lens + gaps) - lens - gaps + 24
        span = np.minimum(lens, rng.integers(0, 200, n))
        perm = rng.permutation(n) if rng.integers(0, 2) else np.arange(n)  # any record order
        assert bench.line_bytes(n, None, offs[perm].astype(np.uint64), span[perm]) == brute_lines(offs, span)


def test_dump_outputs_files(tmp_path, monkeypatch):
    """--dump-outputs: one exact float .npy per column, unused slot rows as 0, and above the budget the
    same seeded sample of packets from every column, identical from run to run."""
    import pytest
    torch = pytest.importorskip("torch")
    from pktgpu import schema
    n = 1000
    rng = np.random.default_rng(3)
    nh = rng.integers(0, 5, n).astype(np.uint8)
    cols = {"n_hdrs": nh,
            "hdr_off": rng.integers(0, 1 << 16, (schema.MAX_HDRS, n)).astype(np.uint16),
            "eth_src": rng.integers(0, 1 << 48, n).astype(np.uint64),
            "ipv4_src": rng.integers(0, 1 << 32, n).astype(np.uint32),
            "ipv6_src": rng.integers(0, 256, (n, 16)).astype(np.uint8)}
    views = {c: torch.from_numpy(a) for c, a in cols.items()}
    used = np.arange(schema.MAX_HDRS)[:, None] < nh[None, :]

    bench.dump_outputs(str(tmp_path / "all"), [views], n)
    got = {c: np.load(tmp_path / "all" / f"{c}.npy") for c in cols}
    assert sorted(p.name for p in (tmp_path / "all").iterdir()) == sorted(f"{c}.npy" for c in cols)
    assert got["n_hdrs"].dtype == np.float32 and got["hdr_off"].dtype == np.float32
    assert got["eth_src"].dtype == np.float64 and got["ipv4_src"].dtype == np.float64
    for c in ("n_hdrs", "eth_src", "ipv4_src", "ipv6_src"):
        assert np.array_equal(got[c].astype(cols[c].dtype), cols[c]), c
    assert np.array_equal(got["hdr_off"], np.where(used, cols["hdr_off"], 0))

    monkeypatch.setattr(bench, "DUMP_BUDGET", 20000)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), [views], n)
    idx = np.load(tmp_path / "s1" / "sample_index.npy").astype(np.int64)
    assert 0 < len(idx) < n and np.all(np.diff(idx) > 0) and idx[-1] < n
    total = 0
    for p in sorted((tmp_path / "s1").iterdir()):
        a = np.load(p)
        total += a.nbytes
        assert np.array_equal(a, np.load(tmp_path / "s2" / p.name)), p.name
    assert total <= 20000
    assert np.array_equal(np.load(tmp_path / "s1" / "eth_src.npy"), cols["eth_src"][idx].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "s1" / "hdr_off.npy"), np.where(used, cols["hdr_off"], 0)[:, idx])
    assert np.array_equal(np.load(tmp_path / "s1" / "ipv6_src.npy"), cols["ipv6_src"][idx])


def test_gpus_beyond_visible_devices_exits_nonzero():
    """`bench.py --gpus N` with fewer visible devices must fail.  This container has
    no GPU."""
    import subprocess
    import sys
    import pytest
    torch = pytest.importorskip("torch")
    if torch.cuda.device_count() >= 2:
        pytest.skip("two or more devices visible")
    for extra in ([],):
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2",
                            "--warmup", "1", "--no-cpu-baseline"] + extra,
                           capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "")))
        assert r.returncode != 0, (extra, r.stdout[-500:], r.stderr[-500:])
        assert "device" in r.stderr, r.stderr[-500:]
        assert not r.stdout.strip(), r.stdout[-500:]
