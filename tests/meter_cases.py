"""pkt_meter_*: the sequential model of include/pktgpu.h in Python integers, and the cases the host handle
(test_meter_host.py) and the device handle (test_meter_device.py) are both held to, exactly.

A SCENARIO is dict(cfgs=[...], adjust=int, calls=[dict(b=batch, chain=None | chain, **kwargs of Meters.run)]): the calls
are made in order on one handle and on one Model, and everything is compared after each: colour, passed, marked, hits,
bytes, the slab and the exported state.  Metering never looks at packet bytes, so most batches are `plain`: every
packet starts at offset 0 of one small slab and only its length differs."""
import numpy as np

import pktgpu
from pktgpu import schema

import compare_cases as C
import fwd_cases as W
import nat_cases as N

UNIT = 10 ** 9
GREEN, YELLOW, RED, UNMETERED = range(4)
PASS, DROP, REMARK = range(3)
T_IPV4, T_IPV6 = schema.HDR_ID["IPv4"], schema.HDR_ID["IPv6"]
LAST = 0xFF
NAMES = ("color", "passed", "marked")
NONE = 0xFFFFFFFF


def cfg(cir, cbs, xbs=0, pir=0, mode="srtcm", aware=False, action=(PASS, PASS, DROP), dscp=(0, 0, 0)):
    return dict(cir=cir, pir=pir, cbs=cbs, xbs=xbs, mode=mode, color_aware=aware, action=action, dscp=dscp)


# ------------------------------------------------------------------ the model
def find_ip(chain, i, which):
    """pkt_fwd_batch step 2: (type, offset) of the IP entry `which` names among the first min(n_hdrs, 16), or None."""
    nh = min(int(chain["n_hdrs"][i]), schema.MAX_HDRS)
    seen, got = 0, None
    for j in range(nh):
        t = int(chain["hdr_type"][j, i])
        if t in (T_IPV4, T_IPV6):
            if which == LAST or seen == which:
                got = (t, int(chain["hdr_off"][j, i]))
            seen += 1
    return got


def remark(slab, at, v4, dscp):
    """Step 6's stores on the numpy slab, the IP header at `at`."""
    b0, b1 = int(slab[at]), int(slab[at + 1])
    if v4:
        n1 = dscp << 2 | (b1 & 3)
        m, m2 = b0 << 8 | b1, b0 << 8 | n1
        hc = int(slab[at + 10]) << 8 | int(slab[at + 11])
        s = (~hc & 0xFFFF) + (~m & 0xFFFF) + m2
        while s >> 16:
            s = (s & 0xFFFF) + (s >> 16)
        s = ~s & 0xFFFF
        slab[at + 1], slab[at + 10], slab[at + 11] = n1, s >> 8, s & 0xFF
    else:
        slab[at] = (b0 & 0xF0) | dscp >> 2
        slab[at + 1] = (b1 & 0x3F) | (dscp & 3) << 6


class Model:
    def __init__(self, cfgs, adjust=0):
        self.g = pktgpu.meter_cfgs(cfgs)
        self.n = self.g.size
        self.adjust = adjust
        self.reset()

    def reset(self):
        self.c = [int(x) * UNIT for x in self.g["cbs"]]
        self.x = [int(x) * UNIT for x in self.g["xbs"]]
        self.last = [0] * self.n
        self.pk = np.zeros((self.n, 3), np.uint64)
        self.by = np.zeros((self.n, 3), np.uint64)

    def run(self, b, chain=None, meter=0, now=0, time=None, in_color=None, select=None, mark=False, which_ip=0,
            hits=None, nbytes=None):
        n = b["n"]
        slab = b["slab"].copy()
        out = {k: np.zeros(n, np.uint8) for k in NAMES}
        hits = np.zeros(4, np.uint64) if hits is None else hits.copy()
        nbytes = np.zeros(4, np.uint64) if nbytes is None else nbytes.copy()
        g = self.g
        for i, (off, ln) in enumerate(C.extents(b)):
            k = int(meter[i]) if isinstance(meter, np.ndarray) else int(meter) & NONE
            if (select is not None and not select[i]) or k >= self.n:
                out["color"][i], out["passed"][i] = UNMETERED, 1
                hits[3] += 1
                nbytes[3] += ln
                continue
            t = int(time[i]) if time is not None else int(now)
            B = max(0, ln + self.adjust) * UNIT
            cir, pir, cap, xcap = int(g["cir"][k]), int(g["pir"][k]), int(g["cbs"][k]) * UNIT, int(g["xbs"][k]) * UNIT
            tr = g["mode"][k] == schema.METER_TRTCM
            if t > self.last[k]:
                dt = t - self.last[k]
                self.last[k] = t
                if tr:
                    self.c[k] = min(cap, self.c[k] + cir * dt)
                    self.x[k] = min(xcap, self.x[k] + pir * dt)
                else:
                    a = cir * dt
                    c2 = min(cap, self.c[k] + a)
                    self.x[k] = min(xcap, self.x[k] + (self.c[k] + a - c2))
                    self.c[k] = c2
            ic = int(in_color[i]) if in_color is not None and g["flags"][k] & schema.METER_F_COLOR_AWARE else GREEN
            ic = min(ic, RED)
            if tr:
                if ic == RED or self.x[k] < B:
                    col = RED
                elif ic == YELLOW or self.c[k] < B:
                    col = YELLOW
                    self.x[k] -= B
                else:
                    col = GREEN
                    self.c[k] -= B
                    self.x[k] -= B
            elif ic == GREEN and self.c[k] >= B:
                col = GREEN
                self.c[k] -= B
            elif ic <= YELLOW and self.x[k] >= B:
                col = YELLOW
                self.x[k] -= B
            else:
                col = RED
            act = int(g["action"][k][col])
            out["color"][i], out["passed"][i] = col, act != DROP
            self.pk[k, col] += 1
            self.by[k, col] += ln
            hits[col] += 1
            nbytes[col] += ln
            if mark and act == REMARK:
                ipe = find_ip(chain, i, which_ip)
                if ipe and ipe[1] + (20 if ipe[0] == T_IPV4 else 40) <= ln:
                    remark(slab, off + ipe[1], ipe[0] == T_IPV4, int(g["dscp"][k][col]))
                    out["marked"][i] = 1
        out.update(hits=hits, bytes=nbytes, slab=slab)
        return out

    def export(self):
        st = np.zeros(self.n, schema.METER_STATE_DTYPE)
        st["c"], st["x"], st["last"] = self.c, self.x, self.last
        st["packets"], st["bytes"] = self.pk, self.by
        return st


def check(got, want, label=""):
    for k in NAMES + ("hits", "bytes", "slab"):
        if k in got and got[k] is not None:
            bad = np.flatnonzero(np.asarray(got[k]) != want[k])
            assert bad.size == 0, f"{label}: {k} differs at {bad[:8]}: {np.asarray(got[k])[bad[:8]]} != {want[k][bad[:8]]}"


def same_state(got, want, label=""):
    for f in schema.METER_STATE_DTYPE.names:
        bad = np.flatnonzero((got[f] != want[f]).reshape(got.size, -1).any(axis=1))
        assert bad.size == 0, f"{label}: state.{f} differs at meters {bad[:8]}: {got[f][bad[:8]]} != {want[f][bad[:8]]}"


H0 = np.arange(4, dtype=np.uint64) + 5        # what hits / bytes hold before a call: they are added to
Y0 = np.arange(4, dtype=np.uint64) * 1000


def play(m, model, calls, put, get, label="", put_slab=None):
    """Make the calls on the handle `m` and on the model and compare everything after each -> the handle's results.
    put / get move a numpy array to what the handle takes and back; put_slab likewise for the slab."""
    outs = []
    for j, call in enumerate(calls):
        b, chain = call["b"], call.get("chain")
        kw = {k: v for k, v in call.items() if k not in ("b", "chain") and v is not None}
        want = model.run(b, chain, hits=H0, nbytes=Y0, **kw)
        slab = (put_slab or put)(b["slab"])
        db = dict(slab=slab, n=b["n"], stride=b["stride"], offsets=None if b["offsets"] is None else put(b["offsets"]),
                  lens=None if b["lens"] is None else put(b["lens"]))
        dch = None if chain is None else {k: put(v) for k, v in chain.items()}
        dkw = {k: put(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
        hits, nb = put(H0), put(Y0)
        r = m.run(db, dch, counters=(hits, nb), **dkw)
        got = {k: get(getattr(r, k)) for k in NAMES}
        got.update(hits=get(hits), bytes=get(nb), slab=get(slab))
        check(got, want, f"{label} call {j}")
        assert int(got["hits"].sum() - H0.sum()) == b["n"], label
        same_state(m.export(), model.export(), f"{label} call {j}")
        outs.append(got)
    return outs


# ------------------------------------------------------------------ batches
_SLAB =np.random.default_rng(5).integers(0, 256, 65535 + 1, dtype=np.uint8)


def plain(lens):
    """A batch whose packets all start at offset 0 of one 64 KiB slab: only the lengths matter."""
    lens = np.asarray(lens, np.uint32)
    return C.batch(_SLAB, offsets=np.zeros(lens.size, np.uint64), lens=lens)


def head(call, lo, hi):
    """Packets [lo, hi) of a call as a call of its own."""
    b = call["b"]
    out = dict(call)
    out["b"] = C.batch(b["slab"], offsets=b["offsets"][lo:hi], lens=b["lens"][lo:hi])
    for k in ("meter", "time", "in_color", "select"):
        if isinstance(call.get(k), np.ndarray):
            out[k] = call[k][lo:hi]
    if call.get("chain") is not None:
        out["chain"] = {k: np.ascontiguousarray(v[..., lo:hi]) for k, v in call["chain"].items()}
    return out


def mixed_cfgs(nmeters, rng):
    """Both modes, colour-aware or not, every action, bursts of a few packets, rates of a packet per 1..100 us."""
    out = []
    for k in range(min(nmeters, 512)):
        out.append(cfg(cir=int(rng.integers(0, 4)) * 10 ** 7 + (k % 3) * 12345, cbs=int(rng.integers(0, 5000)),
                       xbs=int(rng.integers(0, 5000)), pir=int(rng.integers(0, 6)) * 10 ** 7,
                       mode=("srtcm", "trtcm")[k & 1], aware=bool(k & 2),
                       action=tuple(int(a) for a in rng.integers(0, 3, 3)), dscp=tuple(int(d) for d in rng.integers(0, 64, 3))))
    arr = pktgpu.meter_cfgs(out)
    return arr[np.arange(nmeters) % arr.size].copy()  # the table repeats past 512 meters


def mixed(n, nmeters, seed=1, stray=True, spread=None):
    """A call of n packets over `nmeters` meters: ids drawn from `spread` (default: all, at most 40 distinct so that
    runs form), ids at or above nmeters and 0xFFFFFFFF and unselected packets mixed in, times that mostly advance and
    sometimes run backwards, every in_color 0..3."""
    rng = np.random.default_rng(seed * 1000003 + n * 31 + nmeters)
    ids = rng.choice(nmeters, size=min(nmeters, spread or 40), replace=False).astype(np.uint32)
    meter = ids[rng.integers(0, ids.size, n)].astype(np.uint32)
    select = np.ones(n, np.uint8)
    if stray and n:
        r = rng.random(n)
        meter[r < 0.05] = nmeters
        meter[(r >= 0.05) & (r < 0.08)] = NONE
        meter[(r >= 0.08) & (r < 0.1)] = nmeters + int(rng.integers(1, 1 << 20))
        select[rng.random(n) < 0.07] = 0
    step = rng.integers(0, 40000, n).astype(np.int64)
    step[rng.random(n) < 0.1] = 0
    time = (10 ** 6 + np.cumsum(step)).astype(np.int64)
    back = rng.random(n) < 0.05
    time[back] -= rng.integers(1, 10 ** 5, int(back.sum()))
    return dict(b=plain(rng.integers(0, 1600, n)), meter=meter, time=time.astype(np.uint64),
                in_color=rng.integers(0, 4, n).astype(np.uint8), select=select)


def scenario(cfgs, calls, adjust=0):
    return dict(cfgs=cfgs, adjust=adjust, calls=calls if isinstance(calls, list) else [calls])


SIZES_N = [0, 1, 63, 64, 65, 2047, 2048, 2049, 4097]
SIZES_M = [1, 2, 255, 256, 257, 65537]


def sizes(n, nmeters):
    rng = np.random.default_rng(nmeters)
    return scenario(mixed_cfgs(nmeters, rng), mixed(n, nmeters), adjust=(20, -14, 0)[n % 3])


def one_meter(n, c=None, lens=None, gap=1000, in_color=None, **kw):
    """n packets on meter 0, `gap` ns apart."""
    lens = np.full(n, 100) if lens is None else lens
    return scenario([c or cfg(cir=5 * 10 ** 7, cbs=3000, xbs=3000)],
                    dict(b=plain(lens), meter=0, time=(1000 + gap * np.arange(n)).astype(np.uint64), in_color=in_color, **kw))


def runs_side_by_side():
    """Runs of 63, 64 and 65 packets (and one of 200), interleaved in index order."""
    ids = np.repeat(np.arange(4, dtype=np.uint32), [63, 64, 65, 200])
    np.random.default_rng(9).shuffle(ids)
    n = ids.size
    cfgs = [cfg(cir=10 ** 7, cbs=2000, xbs=1500), cfg(cir=10 ** 7, cbs=2000, xbs=1500, pir=3 * 10 ** 7, mode="trtcm")] * 2
    return scenario(cfgs, dict(b=plain(np.full(n, 200)), meter=ids, time=(5000 * np.arange(n)).astype(np.uint64)))


def distinct(n=300):
    rng = np.random.default_rng(4)
    return scenario(mixed_cfgs(n, rng), dict(b=plain(rng.integers(0, 1600, n)), meter=rng.permutation(n).astype(np.uint32),
                                             now=10 ** 6, in_color=rng.integers(0, 4, n).astype(np.uint8)))


def step_with_one_bad(pos, aware):
    """Three wave steps of one meter, green but for the packet at `pos` of the middle step: red on its in_color
    (aware), or too long for either bucket."""
    n, lens, ic = 192, np.full(192, 100), np.zeros(192, np.uint8)
    if aware:
        ic[64 + pos] = RED
    else:
        lens[64 + pos] = 1600
    return one_meter(n, cfg(cir=10 ** 9, cbs=1500, xbs=1000, aware=aware), lens, gap=1000, in_color=ic)


def overload(mode):
    """Twice the committed rate, a packet of the bucket's size at a time: green and red interleave."""
    # (trTCM: a peak burst of one packet too, refilled at the same rate, so that every second packet finds x < B)
    c = cfg(cir=10 ** 9, cbs=1000, xbs=1000, mode=mode, pir=10 ** 9) if mode == "trtcm" else cfg(cir=10 ** 9, cbs=1000, xbs=0)
    return one_meter(1025, c, np.full(1025, 1000), gap=500)


def all_red(n=321):
    return one_meter(n, cfg(cir=0, cbs=0, xbs=0), np.full(n, 64))


def edges():
    """name -> scenario: the bucket and time edges, one meter each, several calls where `last` has to carry."""
    t = lambda *a: np.asarray(a, np.uint64)  # noqa: E731
    big = cfg(cir=1 << 40, cbs=1 << 26, xbs=1 << 26, pir=1 << 40)
    out = {
        # a 1000-byte bucket refilled by 1 byte per second: 10^12 ns give exactly 1000 bytes, one ns less one unit less
        "cost_equals_level": scenario([cfg(1, 1000)], dict(b=plain([1000, 1000]), time=t(0, 10 ** 12))),
        "cost_one_unit_above": scenario([cfg(1, 1000)], dict(b=plain([1000, 1000]), time=t(0, 10 ** 12 - 1))),
        "refill_lands_on_cap": scenario([cfg(1, 1000, 7)], dict(b=plain([1000, 0, 1000, 1]), time=t(5, 10 ** 12 + 5, 10 ** 12 + 5, 10 ** 12 + 5))),
        # both buckets drained, then a refill of exactly cbs + xbs, and of one unit less
        "spill_fills_x": scenario([cfg(3, 1000, 500)], dict(b=plain([1000, 500, 0, 1000, 500, 1]), time=t(1, 1, 1 + 5 * 10 ** 11, 1 + 5 * 10 ** 11, 1 + 5 * 10 ** 11, 1 + 5 * 10 ** 11))),
        "spill_one_unit_short": scenario([cfg(1, 1000, 500)], dict(b=plain([1000, 500, 0, 1000, 500]), time=t(1, 1, 15 * 10 ** 11, 15 * 10 ** 11, 15 * 10 ** 11))),
        "cbs_0": scenario([cfg(10 ** 6, 0, 800)], dict(b=plain([0, 1, 700, 100, 1]), now=7)),
        "xbs_0": scenario([cfg(10 ** 6, 800, 0)], dict(b=plain([0, 1, 700, 99, 1]), now=7)),
        "cir_0": scenario([cfg(0, 500, 500), cfg(0, 500, 500, pir=0, mode="trtcm")],
                          dict(b=plain([400] * 8), meter=np.asarray([0, 1] * 4, np.uint32), time=t(*range(0, 8 * 10 ** 12, 10 ** 12)))),
        "cost_0": scenario([cfg(0, 0, 0)], dict(b=plain([0, 14, 1999, 2000, 2001]), now=1), adjust=-2000),
        "adjust_min": scenario([cfg(0, 0, 0)], dict(b=plain([0, 65535]), now=1), adjust=-(1 << 31)),
        "largest": scenario([big, dict(big, mode="trtcm")],
                            [dict(b=plain([65535] * 6), meter=np.asarray([0, 1] * 3, np.uint32), time=t(0, 0, 1, 1, 1 << 63, 1 << 63)),
                             dict(b=plain([65535] * 4), meter=np.asarray([0, 1] * 2, np.uint32), time=t((1 << 64) - 1, (1 << 64) - 1, 5, 5))],
                            adjust=(1 << 31) - 1),
        "largest_fits": scenario([big, dict(big, mode="trtcm")],
                                 [dict(b=plain([65535] * 2100), meter=np.asarray([0, 1] * 1050, np.uint32), now=0),
                                  dict(b=plain([65535] * 4), meter=np.asarray([0, 1] * 2, np.uint32), now=1 << 63)], adjust=20),
        # 130 packets a meter (two whole wave steps and a rest) at the largest burst and rate, the stamps 2^55 ns apart:
        # every lane's gain is at its clamp, which is what the wave scans' sums have to hold.  With adjust = 20 every
        # packet is green (the scan is accepted); with the largest adjust no cost can be paid (the scan fails, the walk)
        "wave_max_gain": scenario([big, dict(big, mode="trtcm")],
                                  dict(b=plain([65535] * 260), meter=np.asarray([0, 1] * 130, np.uint32),
                                       time=(np.arange(1, 261, dtype=np.uint64) << np.uint64(55))), adjust=20),
        "wave_max_gain_drained": scenario([big, dict(big, mode="trtcm")],
                                          [dict(b=plain([65535] * 2100), meter=np.asarray([0, 1] * 1050, np.uint32), now=0),
                                           dict(b=plain([65535] * 260), meter=np.asarray([0, 1] * 130, np.uint32),
                                                time=(np.arange(1, 261, dtype=np.uint64) << np.uint64(55)))], adjust=20),
        "wave_max_gain_cost": scenario([big, dict(big, mode="trtcm")],
                                       dict(b=plain([65535] * 260), meter=np.asarray([0, 1] * 130, np.uint32),
                                            time=(np.arange(1, 261, dtype=np.uint64) << np.uint64(55))), adjust=(1 << 31) - 1),
        "dt_2_63": scenario([cfg(1, 1000, 1000), cfg(1 << 40, 1000, 1000, pir=1, mode="trtcm")],
                            [dict(b=plain([1000] * 4), meter=np.asarray([0, 0, 1, 1], np.uint32), now=0),
                             dict(b=plain([1000] * 4), meter=np.asarray([0, 0, 1, 1], np.uint32), now=1 << 63)]),
        "now_alone": scenario([cfg(10 ** 9, 1000, 1000)], [dict(b=plain([600] * 5), now=10), dict(b=plain([600] * 5), now=1210)]),
        "equal_stamps": scenario([cfg(10 ** 9, 1000, 1000)], dict(b=plain([300] * 9), time=t(*([50] * 9)))),
        "backwards": scenario([cfg(10 ** 9, 1000, 1000)], dict(b=plain([500] * 8), time=t(1000, 900, 1100, 1000, 1050, 1300, 1, 1301))),
        "below_carried_last": scenario([cfg(10 ** 9, 1000, 1000)], [dict(b=plain([900] * 3), now=10 ** 6), dict(b=plain([900] * 3), now=10 ** 5),
                                                                    dict(b=plain([900] * 3), now=10 ** 6 + 400)]),
    }
    return out


def color_aware():
    """Every in_color 0..3 against every bucket situation (each bucket enough or not), both modes, aware or not."""
    cfgs, meter, ic = [], [], []
    for mode in ("srtcm", "trtcm"):
        for aware in (True, False):
            for cbs in (0, 1000):
                for xbs in (0, 1000):
                    for c in range(4):
                        meter.append(len(cfgs))
                        ic.append(c)
                        cfgs.append(cfg(0, cbs, xbs, mode=mode, aware=aware, action=(PASS, REMARK, DROP)))
    n = len(cfgs)
    return scenario(cfgs, dict(b=plain([500] * n), meter=np.asarray(meter, np.uint32), in_color=np.asarray(ic, np.uint8), now=3))


def named():
    out = {f"edge_{k}": v for k, v in edges().items()}
    for k in (1, 2, 5):
        out[f"one_meter_{64 * k + 1}"] = one_meter(64 * k + 1, lens=np.random.default_rng(k).integers(0, 400, 64 * k + 1))
    out["runs_63_64_65"] = runs_side_by_side()
    out["distinct"] = distinct()
    for pos in (0, 32, 63):
        out[f"step_bad_{pos}_aware"] = step_with_one_bad(pos, True)
        out[f"step_bad_{pos}_long"] = step_with_one_bad(pos, False)
    out["overload_srtcm"] = overload("srtcm")
    out["overload_trtcm"] = overload("trtcm")
    out["all_red"] = all_red()
    out["color_aware"] = color_aware()
    return out


_CACHE = {}


def cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def named_cached():
    return cached("named", named)


NAMED = sorted(named_cached())
SPLITS = [1, 64, 2048, 4096]


def split_case():
    rng = np.random.default_rng(77)
    return mixed_cfgs(300, rng), mixed(4097, 300, seed=7)


# ------------------------------------------------------------------ remark
MARK_ALL = dict(action=(REMARK, REMARK, REMARK))


def ecn(item, bits, good=True):
    """The item with its first IP header's ECN bits and some DSCP set (IPv4: the checksum valid, or off by 5)."""
    p, hdrs = item
    t, o = [(t, o) for t, o in hdrs if t in (T_IPV4, T_IPV6)][0]
    q = bytearray(p)
    if t == T_IPV4:
        q[o + 1] = 0x54 | bits
        q = bytearray(W.fix_csum(bytes(q), o))
        if not good:
            q[o + 11] = (q[o + 11] + 5) & 0xFF
    else:
        q[o], q[o + 1] = (q[o] & 0xF0) | 0x5, (q[o + 1] & 0x0F) | 0x40 | bits << 4
    return bytes(q), hdrs


def remark_items():
    """IPv4 and IPv6 under 0..2 VLAN tags, valid and wrong checksums, every ECN value, enough of them for every
    alignment 0..15; then a tunnel packet, a packet with no IP entry, cut headers and forged chain columns."""
    items = []
    for k in range(36):
        vl, bits = k % 3, k % 4
        items.append(ecn(W.v4(vlans=vl, payload=b"m" * (k % 7)), bits, good=k % 5 != 0))
        items.append(ecn(W.v6(vlans=vl, payload=b"m" * (k % 5)), bits))
    items.append(N.vxlan())
    v4, v6 = W.v4(), W.v6()
    items += [W.without(v4, T_IPV4), W.cut_ip(v4, 1), W.cut_ip(v6, 1), W.cut_ip(v4, 19), (v4[0][:14], v4[1])]
    forged = [(T_IPV4, 0xFFF0)], [(T_IPV6, len(v6[0]) - 39)], [(T_IPV4, len(v4[0]) - 20)] * 40
    items += [(v4[0], h) for h in forged]
    return items


def remark_call(which_ip=0, kind="indexed", seed=2):
    items = remark_items()
    b, chain = N.layout(items, kind)
    n = b["n"]
    rng = np.random.default_rng(seed)
    cfgs = [cfg(0, 0, 0, dscp=(10, 20, 46), **MARK_ALL), cfg(0, 1 << 20, 0, dscp=(63, 1, 2), **MARK_ALL),
            cfg(0, 0, 1 << 20, dscp=(0, 0, 0), **MARK_ALL), cfg(0, 1 << 20, 0, dscp=(33, 0, 0), action=(REMARK, PASS, DROP)),
            cfg(0, 0, 0, dscp=(1, 2, 3), action=(PASS, PASS, DROP))]
    return cfgs, dict(b=b, chain=chain, meter=rng.integers(0, 6, n).astype(np.uint32), now=1, mark=True, which_ip=which_ip)
