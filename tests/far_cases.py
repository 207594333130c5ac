"""Far layouts: the packets of any compact batch placed past 2^31 and 2^32 bytes into a slab of more than 4 GiB
(tests/test_far_offsets_host.py, test_far_offsets_device.py).  numpy only.

place(plan, b) takes a compact batch (the dict(slab, offsets, lens, stride, n) of compare_cases.batch / C.indexed / the
layout() functions) whose n is N[plan] and returns a Placement: new offsets (or a stride) for the same packets and the
byte regions to write.  It allocates nothing: the caller owns the allocation (numpy here, torch on the device) and
writes the regions, so one plan serves both.  Expected values never come from here: they are the call's own model
run over the COMPACT batch, since no output of any call depends on where a source packet lies.

The slab is a view that begins FRONT = 2^31 + 4096 bytes into the allocation, 16-byte aligned when the allocation is.
Every packet at or above 2^31 has a decoy where a wrong offset would land, a well-formed packet of the same length
with other addresses, ports, ttl, MAC and payload (decoy()):
    off >= 2^32          -> off mod 2^32                (a lost high half)
    2^31 <= off < 2^32   -> off - 2^32, a negative position inside the front area (a sign-extended low half)
so a truncated or sign-extended offset reads or rewrites a different packet inside the allocation: a wrong answer or
a touched decoy, never a fault.  Around every packet and decoy lie 64-byte guard bands (the bytes within 64 of a
region that belong to no region); regions are pairwise disjoint, which place() asserts.

Plans:
  indexed_ascending  n = 200, offsets ascending with i, >= 16 bytes of fill between neighbours, slot s at s % 16 mod 16
                     unless its role fixes it:
                         0..29    a control group near 2^20
                         30..89   around 2^31: 59 ends exactly at 2^31, 60 starts exactly on it
                         90..109  from 3 * 2^30
                         110..135 around 2^32: 122 starts at 2^32 - 9 and straddles it at an odd alignment
                         136..199 above 2^32, every alignment 0..15 four times, 199 ending at the slab's last byte
                     so wave 0 (0..63) holds both sides of 2^31, wave 1 (64..127) both sides of 2^32, and wave 2
                     (128..191) lies wholly above 2^32.
                     One boundary cannot carry "ends exactly at it", "straddles it" and "starts exactly on it" at once
                     (the straddler overlaps both others), so 2^31 has the first and the last, touching (the one pair
                     of neighbours with no fill between them), and 2^32 the straddler; stride_1MiB starts slots
                     exactly on both boundaries.
  indexed_shuffled   the same slots, the batch order permuted by a fixed seed: batch packet j lies in slot PERM[j], so
                     every wave mixes low, middle and far packets.  Offsets need not be ordered (include/pktgpu.h,
                     pkt_batch_t), and no call's header comment asks for order: no call is left out of this plan.
  stride_1MiB        stride 2^20, lens given, n = 4096 + 65: slots from 2048 on lie past 2^31, from 4096 on past 2^32,
                     and slab_len = (n - 1) * stride + lens[n - 1].  Slot k >= 4096 aliases slot k - 4096, which holds
                     a packet of its own: cycle() shifts the items there so that the two differ, and that packet is
                     the decoy.  Slots 2048..4095 get decoys in the front area.
"""
import struct

import numpy as np

import pyref
from pktgpu import schema

FRONT = (1 << 31) + 4096
GUARD = 64
FILL = 0xA5
B31, B32 = 1 << 31, 1 << 32
PLANS = ("indexed_ascending", "indexed_shuffled", "stride_1MiB")
STRIDE = 1 << 20
N = {"indexed_ascending": 200, "indexed_shuffled": 200, "stride_1MiB": 4096 + 65}
PERM = np.random.default_rng(0xFA2).permutation(200)
ENDS_AT_31, STARTS_ON_31, STRADDLES_32 = 59, 60, 122


def cycle(items, plan):
    """The case's items cycled to the plan's n.  In stride_1MiB slot k >= 4096 takes another item than slot k - 4096,
    the slot a lost high half reads."""
    m, n = len(items), N[plan]
    if plan != "stride_1MiB":
        return [items[k % m] for k in range(n)]
    assert m >= 2
    shift = 1 if (4096 + 1) % m else 2
    return [items[(k + (shift if k >= 4096 else 0)) % m] for k in range(n)]


def extents(b):
    """pkt_batch_t's rules: (offset, clamped length) of every packet of a compact batch."""
    size = b["slab"].size
    out = []
    for i in range(b["n"]):
        off = int(b["offsets"][i]) if b.get("offsets") is not None else i * b["stride"]
        ln = int(b["lens"][i]) if b.get("lens") is not None else b["stride"]
        out.append((off, min(ln, max(0, size - off), 65535)))
    return out


# ------------------------------------------------------------------ decoys
def _ones_sum(data):
    s = sum(struct.unpack(f">{len(data) // 2}H", bytes(data)))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def decoy(p):
    """Packet `p` as another host pair would have sent it: the same length and the same header chain, the last byte of
    every Ether / Dot3 source MAC, of every IP source and destination (IPv4: the last two) and of every ARP sender
    address changed, every
    ttl / hop limit, both ports of every TCP / UDP header (the destination of a UDP header in front of a Vxlan one
    stays: the chain depends on it) and every payload byte.  An IPv4 header checksum that was valid is valid again;
    L4 checksums are left as they were, so they no longer verify: l4_checksum tells the two apart as well."""
    q = bytearray(p)
    n = len(q)

    def flip(at, mask):
        if at < n:
            q[at] ^= mask

    status, hdrs, pay, _ = pyref.parse(bytes(p))
    if status != "OK":  # cut inside its headers: no chain to follow
        flip(11, 0x01)
        flip(22, 0x10)
        for at in range(26, n):
            q[at] ^= 0x5A
    else:
        for j, (name, o) in enumerate(hdrs):
            if name in ("Ether", "Dot3"):
                flip(o + 11, 0x01)
            elif name == "IPv4":
                valid = o + 20 <= n and q[o] == 0x45 and _ones_sum(q[o:o + 20]) == 0xFFFF
                flip(o + 8, 0x10)
                flip(o + 14, 0x01)
                flip(o + 15, 0x55)
                flip(o + 18, 0x01)
                flip(o + 19, 0x2A)
                if valid:
                    q[o + 10:o + 12] = b"\0\0"
                    q[o + 10:o + 12] = struct.pack(">H", 0xFFFF - _ones_sum(q[o:o + 20]))
            elif name == "IPv6":
                flip(o + 7, 0x10)
                flip(o + 23, 0x55)
                flip(o + 39, 0x2A)
            elif name in ("TCP", "UDP"):
                flip(o + 1, 0x11)
                if not (j + 1 < len(hdrs) and hdrs[j + 1][0] == "Vxlan"):
                    flip(o + 3, 0x22)
            elif name == "ARP":
                flip(o + 17, 0x55)
        for at in range(pay, n):
            q[at] ^= 0xFF
    if n and bytes(q) == bytes(p):
        q[n - 1] ^= 0xFF
    return bytes(q)


# ------------------------------------------------------------------ placements
def _pack(lens, slots, start):
    """Offsets of `slots` one after the other from `start` (a multiple of 16): slot s at s % 16 mod 16, at least 16
    bytes behind its predecessor's end.  -> ({slot: offset}, end of the last)."""
    at, pos, first = {}, start, True
    for s in slots:
        pos = (pos + (0 if first else 16) + 15) // 16 * 16 + s % 16
        at[s] = pos
        pos += lens[s]
        first = False
    return at, pos


def _below(lens, slots, top):
    """The same run shifted by a multiple of 16 so that it ends at least 64 bytes below `top`."""
    at, end = _pack(lens, slots, 0)
    shift = (top - 64 - end) // 16 * 16
    return {s: o + shift for s, o in at.items()}


def _indexed_slots(lens):
    """Slot -> offset for the 200 slots of the indexed plans, and slab_len."""
    x = STRADDLES_32
    if lens[x] <= 9:  # the straddler must reach past 2^32: take the nearest slot that does
        x = min((s for s in range(112, 127) if lens[s] > 9), key=lambda s: abs(s - STRADDLES_32))
    at = {}
    # around 2^31
    at[ENDS_AT_31] = B31 - lens[ENDS_AT_31]
    at[STARTS_ON_31] = B31
    at.update(_below(lens, range(30, ENDS_AT_31), at[ENDS_AT_31]))
    up, _ = _pack(lens, range(STARTS_ON_31 + 1, 90), B31 + (lens[STARTS_ON_31] + 16 + 15) // 16 * 16)
    at.update(up)
    # from 3 * 2^30
    at.update(_pack(lens, range(90, 110), 3 << 30)[0])
    # around 2^32, and on to the slab's end
    at[x] = B32 - 9
    at.update(_below(lens, range(110, x), at[x]))
    up, end = _pack(lens, range(x + 1, 200), (B32 - 9 + lens[x] + 16 + 15) // 16 * 16)
    at.update(up)
    # the control group, clear of where the far packets' decoys land
    far = end - B32
    base = max(1, -(-(far + 65536) // (1 << 20))) << 20
    at.update(_pack(lens, range(0, 30), base)[0])
    assert end > B32 and at[29] + lens[29] + 65536 < at[30] and end < B32 + B31
    return [at[s] for s in range(200)], end, x


class Placement:
    """plan, n, slab_len, offsets (uint64 or None), lens (uint32), stride (or None); packets / decoys: [(position
    relative to the slab's first byte, bytes)], decoy positions may be negative; offs: the packets' offsets as ints;
    decoy_of: the packet index of each decoy; alloc_len = FRONT + slab_len rounded up to 16."""

    def batch(self, slab):
        """The far batch over `slab`, the caller's view of alloc[FRONT : FRONT + slab_len]."""
        return dict(slab=slab, offsets=self.offsets, lens=self.lens, stride=self.stride, n=self.n)

    def guards(self):
        """[(position, length)] of the guard bands: every byte within GUARD of a region and inside none."""
        lo, hi = -FRONT, self.alloc_len - FRONT
        content = sorted((p, p + len(d)) for p, d in self.packets + self.decoys if len(d))
        near, out = [], []
        for a, e in content:
            a, e = max(lo, a - GUARD), min(hi, e + GUARD)
            if near and a <= near[-1][1]:
                near[-1][1] = max(near[-1][1], e)
            else:
                near.append([a, e])
        k = 0
        for a, e in near:
            pos = a
            while k < len(content) and content[k][0] < e:
                if content[k][0] > pos:
                    out.append((pos, content[k][0] - pos))
                pos = max(pos, content[k][1])
                k += 1
            if pos < e:
                out.append((pos, e - pos))
        return out

    def index(self):
        """(positions int64 relative to the ALLOCATION's first byte, bytes uint8, packet bounds, decoy bounds): every
        region's bytes flattened, packets first; bounds[i] : bounds[i + 1] are region i's."""
        pos, val, pb, db = [], [], [0], [0]
        for regions, bounds in ((self.packets, pb), (self.decoys, db)):
            for p, d in regions:
                pos.append(np.arange(p + FRONT, p + FRONT + len(d), dtype=np.int64))
                val.append(np.frombuffer(d, np.uint8))
                bounds.append(bounds[-1] + len(d))
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)  # noqa: E731
        return cat(pos, np.int64), cat(val, np.uint8), np.array(pb), np.array(db) + pb[-1]


def place(plan, b, distinct=True):
    ext = extents(b)
    n = b["n"]
    assert n == N[plan], (plan, n, N[plan])
    data = [b["slab"][o:o + ln].tobytes() for o, ln in ext]
    lens = [ln for _, ln in ext]
    pl = Placement()
    pl.plan, pl.n, pl.lens = plan, n, np.array(lens, np.uint32)
    pl.decoys, pl.decoy_of = [], []
    if plan == "stride_1MiB":
        assert max(lens) <= STRIDE - 2 * GUARD
        offs = [i * STRIDE for i in range(n)]
        pl.offsets, pl.stride = None, STRIDE
        pl.slab_len = offs[-1] + lens[-1]
        assert offs[2048] == B31 and offs[4096] == B32 and n == 4096 + 65
        for i in range(4096, n if distinct else 0):  # the packet a lost high half reads must be another one
            assert data[i] != data[i - 4096] or not lens[i], i
    else:
        slot_of = np.arange(n) if plan == "indexed_ascending" else PERM
        inv = np.argsort(slot_of)
        slot_at, pl.slab_len, pl.straddler = _indexed_slots([lens[int(inv[s])] for s in range(n)])
        offs = [slot_at[int(slot_of[i])] for i in range(n)]
        pl.offsets, pl.stride = np.array(offs, np.uint64), None
        order = sorted(range(n), key=lambda i: offs[i])
        for a, c in zip(order, order[1:]):
            gap = offs[c] - offs[a] - lens[a]
            assert gap >= 16 or (offs[c] == B31 and gap == 0), (a, c, gap)
        assert max(o + ln for o, ln in zip(offs, lens)) == pl.slab_len
        assert {o % 16 for o in offs if o > B32} == set(range(16))
        at = sorted(offs)  # by slot
        x = pl.straddler
        assert at[ENDS_AT_31] + sorted(zip(offs, lens))[ENDS_AT_31][1] == B31 == at[STARTS_ON_31]
        assert at[x] == B32 - 9 and sorted(zip(offs, lens))[x][1] > 9
        assert at[29] < 1 << 22 and at[30] > 1 << 30 and at[63] > B31 > at[0]  # slots 0..63: both sides of 2^31
        assert at[64] < B32 < at[127] and at[128] > B32                         # 64..127: both sides of 2^32; 128..: above
        assert abs(at[90] - (3 << 30)) < 16
        if plan == "indexed_shuffled":  # every wave of the batch mixes low, middle and far packets
            for w in range(0, n, 64):
                o = offs[w:w + 64]
                assert min(o) < B31 and max(o) > B32 and any(B31 <= v < B32 for v in o), w
    assert pl.slab_len > B32
    pl.alloc_len = (FRONT + pl.slab_len + 15) // 16 * 16
    pl.offs = offs
    pl.packets = list(zip(offs, data))
    for i, (o, d) in enumerate(pl.packets):
        if o >= B32 and plan == "stride_1MiB":
            continue  # slot i - 4096's packet lies there
        if o >= B31:
            pl.decoys.append((o % B32 if o >= B32 else o - B32, decoy(d)))
            pl.decoy_of.append(i)
    # pairwise disjoint, inside the allocation; the guard bands are disjoint from them by construction
    regions = sorted((p, p + len(d)) for p, d in pl.packets + pl.decoys if len(d))
    assert regions[0][0] - GUARD >= -FRONT and regions[-1][1] <= pl.slab_len
    for (a0, a1), (c0, c1) in zip(regions, regions[1:]):
        assert a1 <= c0, ("regions overlap", a0, a1, c0, c1)
    return pl


# ------------------------------------------------------------------ numpy allocations (the host twins)
def host_alloc(pl):
    """(keep, alloc): alloc_len bytes of untouched anonymous memory as a uint8 array, 16-byte aligned.  Pages come
    into being when written: write() touches the regions and their guard bands alone."""
    import mmap
    mm = mmap.mmap(-1, pl.alloc_len)
    if hasattr(mmap, "MADV_NOHUGEPAGE"):
        mm.madvise(mmap.MADV_NOHUGEPAGE)  # a 2 MiB page per touched slot would make the whole slab resident
    alloc = np.frombuffer(mm, np.uint8)
    assert alloc.ctypes.data % 16 == 0
    return mm, alloc


def touched_bytes(pl, page=4096):
    pages = set()
    for p, ln in [(p, len(d)) for p, d in pl.packets + pl.decoys if len(d)] + pl.guards():
        pages.update(range((p + FRONT) // page, (p + FRONT + ln - 1) // page + 1))
    return len(pages) * page


def write(pl, alloc):
    """The guard bands as FILL, then every packet and decoy; -> the slab view."""
    for p, ln in pl.guards():
        alloc[p + FRONT:p + FRONT + ln] = FILL
    for p, d in pl.packets + pl.decoys:
        alloc[p + FRONT:p + FRONT + len(d)] = np.frombuffer(d, np.uint8)
    return alloc[FRONT:FRONT + pl.slab_len]


def check(pl, alloc, after=None, label=""):
    """Every packet's bytes are after[i] (default: as written), every decoy and every guard band is untouched."""
    for i, (p, d) in enumerate(pl.packets):
        want = d if after is None else after[i]
        got = alloc[p + FRONT:p + FRONT + len(d)].tobytes()
        assert got == bytes(want), (label, pl.plan, "packet", i, "at", p)
    for k, (p, d) in enumerate(pl.decoys):
        assert alloc[p + FRONT:p + FRONT + len(d)].tobytes() == d, (label, pl.plan, "the decoy of packet", pl.decoy_of[k], "at", p)
    for p, ln in pl.guards():
        assert (alloc[p + FRONT:p + FRONT + ln] == FILL).all(), (label, pl.plan, "guard band at", p)


def packets_of(b, slab=None):
    """The packets' bytes of a compact batch, read from `slab` (the model's rewritten copy) or its own."""
    s = b["slab"] if slab is None else slab
    return [bytes(s[o:o + ln]) for o, ln in extents(b)]


# ------------------------------------------------------------------ the calls' cases, built compact
# build(call, plan) -> a dict with the compact batch "b" (n = N[plan]), its "chain" where the call takes one, the
# call's own arguments and "want", the call's model over the compact batch; "pl" = place(plan, b).  Built once per
# (call, plan) and left unchanged.  The case modules are imported here, not at the top: the placements need none.
_BUILT = {}
PORTS = (40000, 40999)


def _repack(pkts, chain, plan, seed=9):
    """(batch, chain) of the small case's packets cycled to the plan's n, in compare_cases' indexed layout, the chain
    columns following their packets."""
    import compare_cases as C
    idx = cycle(list(range(len(pkts))), plan)
    b = C.indexed([pkts[k] for k in idx], np.random.default_rng(seed), align=[i % 16 for i in range(len(idx))])
    return b, (None if chain is None else {k: np.ascontiguousarray(v[..., idx]) for k, v in chain.items()}), idx


def _build(call, plan):
    import compare_cases as C
    n = N[plan]
    rng = np.random.default_rng(41)
    if call == "pcap_write":
        import l4_cases as L4
        import pcap_write_cases as PW
        c0 = L4.all_cases()["protocols"][0]
        b, _, _ = _repack(C.packets(c0["batch"]), None, plan)
        c = PW.case(b["slab"], b["offsets"], b["lens"], select=np.arange(n) % 5 != 2, snaplen=0,
                    ts=(rng.integers(0, 1 << 32, n, dtype=np.uint32), rng.integers(0, 10 ** 6, n, dtype=np.uint32)))
        return dict(b=b, c=c, want=PW.expect(c))
    if call == "compare":
        c0 = C.all_cases()["straddle"][0]
        a, ch, idx = _repack(C.packets(c0["a"]), c0["chain"], plan, 9)
        b2, _, _ = _repack(C.packets(c0["b"]), None, plan, 10)
        c = C.case(a, b2, c0["ignore"], ch)
        return dict(b=a, b2=b2, chain=ch, ignore=c0["ignore"], want=C.expect(c))
    if call == "edit":
        import edit_cases as E
        import match_cases as M
        src, _, _ = _repack(C.packets(M.ref22_batch()), None, plan)
        ops = [("remove", 1), ("insert", "MPLS", E.MPLS, 2)]
        c = E.case(src, ops, slot=EDIT_SLOT, select=np.arange(n) % 7 != 3)
        return dict(b=src, c=c, parsed=E.parsed_of(src), want=E.expect(c))
    if call == "l4_checksum":
        import l4_cases as L4
        c0 = L4.all_cases()["protocols"][0]
        pk = C.packets(c0["batch"])  # every other one with a changed last byte: its checksum is wrong, UPDATE stores
        pk = [p[:-1] + bytes([p[-1] ^ 0x5A]) if k % 2 and p else p for k, p in enumerate(pk)]
        b, ch, _ = _repack(pk, c0["chain"], plan)
        c = dict(batch=b, chain=ch, which=c0["which"])
        return dict(b=b, chain=ch, which=c0["which"], want=L4.expect(c), want_update=L4.expect(c, update=True))
    if call == "flow_keys":
        import flow_cases as F
        c0 = F.all_cases()["protocols"][0]
        b, ch, _ = _repack(C.packets(c0["batch"]), c0["chain"], plan)
        c = dict(batch=b, chain=ch, opt=c0["opt"])
        return dict(b=b, chain=ch, opt=c0["opt"], want=F.expect(c))
    if call == "match":
        import match_cases as M
        b0, ch0, prog, _ = M.all_cases()["random_rules64"]
        b, ch, _ = _repack(C.packets(b0)[:400], {k: v[..., :400] for k, v in ch0.items()}, plan)
        want = M.Evaluator(b, ch).run(prog)
        want.pop("cover")
        return dict(b=b, chain=ch, prog=prog, want=want)
    if call == "reorder":
        import dispatch_cases as D
        b0, cols0 = D.sources()["mix"]
        b, cols, _ = _repack(C.packets(b0), {k: cols0[k] for k in ("n_hdrs", "hdr_type", "hdr_off", "eth_dst")}, plan)
        perm = rng.permutation(n + 3).astype(np.uint32)  # three empty positions
        return dict(b=b, cols=cols, perm=perm, slot=REORDER_SLOT, want=D.expect_reorder(b, perm, cols, None, 0, REORDER_SLOT))
    if call == "lpm":
        import lpm_cases as X
        routes, probes, model, _ = X.cached("random")
        b, ch = X.batch_case(cycle(X.mixed_items(probes[:400]), plan))
        return dict(b=b, chain=ch, routes=routes, want=X.expect_batch(model, b, ch))
    if call in ("fwd", "fwd_lpm"):
        import fwd_cases as W
        c = W.mix(n=n) if call == "fwd" else W.fused("random")
        if call == "fwd_lpm":
            c = dict(c, items=cycle(c["items"], plan))
        b, ch = W.layout(c, "indexed")
        return dict(b=b, chain=ch, c=c, want=W.expect(c, b, ch))
    if call == "frag":
        import frag_cases as G
        items, mtu, sel = G.mix(n, big=False)
        b, ch = G.layout(items)
        return dict(b=b, chain=ch, mtu=mtu, select=sel, want=G.expect(b, ch, mtu, sel))
    if call == "reasm":
        import reasm_cases as R
        for seed in range(17, 49):  # the first mix with a datagram joined from members on both sides of 2^32
            items, sel = R.mix(n, seed)
            b, ch = R.layout(items)
            want, pl = R.expect(b, ch, sel), place(plan, b)
            sides = {}
            for i in np.flatnonzero(want["status"] == R.JOINED):
                sides.setdefault(int(want["out_index"][i]), set()).add(pl.offs[i] >= B32)
            if any(len(s) == 2 for s in sides.values()):
                break
        return dict(b=b, chain=ch, select=sel, want=want)
    if call == "icmp_err":
        import icmp_cases as I
        items, code, mtu, sel = I.mix(n)
        b, ch = I.layout(items)
        cf = I.cfg(ident=65000)
        cmap = np.array(schema.ICMP_MAP_FWD, np.uint8)  # (Parser.icmp_errors(fwd_status=...) reads the codes through it)
        return dict(b=b, chain=ch, code=code, mtu=mtu, select=sel, cf=cf, cmap=cmap,
                    want=I.expect(b, ch, code, cf, mtu, cmap, sel, 0))
    if call in ("scan_packet", "scan_payload"):
        import scan_cases as S
        c0 = S.all_cases()["every_alignment"]
        b, _, _ = _repack(C.packets(c0["batch"]), None, plan)
        region = call[5:]
        c = S.case(c0["pats"], b, region, S.ether_chain(n) if region == "payload" else None, default=4)
        return dict(b=b, c=c, chain=c["chain"], want=S.expect(c))
    if call == "nat":
        import nat_cases as NA
        st = NA.statuses_items()
        items = [s[0] for s in st] + [NA.flow_item(k, vlans=k % 3) for k in range(31)]
        dirs = [s[1] for s in st] + [NA.OUT] * 31
        sels = [s[2] for s in st] + [1] * 31
        idx = cycle(list(range(len(items))), plan)
        b, ch = NA.layout([items[k] for k in idx])
        dirs, sels = np.array([dirs[k] for k in idx], np.uint8), np.array([sels[k] for k in idx], np.uint8)
        m = NA.Model(NA.POOL1, PORTS)
        want = m.run(b, ch, dir=dirs, select=sels, now=5)
        # the way back: the replies to the translated packets, against the sessions the first call made
        ok = np.flatnonzero((want["status"] == NA.OK) & (dirs == NA.OUT))
        back = [NA.reply((NA.packet_after(b, want["slab"], int(i)), items[idx[int(i)]][1])) for i in ok]
        b_in, ch_in = NA.layout(cycle(back, plan))
        want_in = m.run(b_in, ch_in, dir=NA.IN, now=9)
        assert (want_in["status"] == NA.OK).all() and want["created"].sum() == 32  # (the statuses' OK packet is a flow too)
        return dict(b=b, chain=ch, dir=dirs, select=sels, want=want, b_in=b_in, chain_in=ch_in, want_in=want_in,
                    sessions=m.sessions())
    if call == "parse":  # the ref22 packets; the caller runs the oracle over `b` (parse, to_vec)
        import edit_cases as E
        import match_cases as M
        b, _, idx = _repack(C.packets(M.ref22_batch()), None, plan)
        return dict(b=b, parsed=E.parsed_of(b))
    if call == "rewrite":  # extract_fields / set_fields / set_fields_csum / ipv4_update_checksum over the ref22 packets
        import match_cases as M
        import rewrite_cases as RW
        b, _, _ = _repack(C.packets(M.ref22_batch()), None, plan)
        c = RW.make(b, RW.SHAPE_SPECS, rng)
        return dict(b=b, chain=c["chain"], specs=c["specs"], values=c["values"], want_get=RW.expect_get(c),
                    want_set=RW.expect_set(c), want_csum=RW.expect_set(c, csum=0), want_update=RW.expect_update(c, 0))
    raise KeyError(call)


EDIT_SLOT = 512
REORDER_SLOT = 1536


def build(call, plan):
    key = (call, plan)
    if key not in _BUILT:
        c = _build(call, plan)
        c["pl"] = place(plan, c["b"])
        for k in ("b2", "b_in"):
            if k in c:
                c["pl_" + k] = place(plan, c[k])
        _BUILT[key] = c
    return _BUILT[key]


def slots(plan, slot):
    """A Placement for n destination slots of `slot` bytes each (edit's dst_offsets, far): its offsets are where the
    outputs go; it has no bytes of its own to write."""
    n = N[plan]
    b = dict(slab=np.zeros(n * slot, np.uint8), offsets=None, lens=None, stride=slot, n=n)
    return place(plan, b, distinct=False)


def check_reorder(c, dst, out_len, cols, label):
    """Every position's bytes with their zero padding, the lengths, and the columns by dispatch_cases' rule."""
    import dispatch_cases as D
    want, slot = c["want"], c["slot"]
    assert np.array_equal(np.asarray(out_len), want["out_len"]), label
    dst = np.asarray(dst)
    for k, ln in enumerate(want["out_len"]):
        r = (int(ln) + 15) // 16 * 16
        assert dst[k * slot:k * slot + r].tobytes() == want["dst"][k * slot:k * slot + r].tobytes(), (label, "position", k)
    D.check_reorder(None, None, cols, dict(want, dst=None), label)
