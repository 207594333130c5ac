"""Output schema of the batched parser — the Python mirror of include/pktgpu.h.

Everything here is metadata: header ids/names (reference src/headers.rs:529-827), the
parser entry points (src/parser/fast.rs), and the struct-of-arrays column layout of
`pkt_out_t`.  The order of OUT_COLUMNS is the field order of `pkt_out_t` and must not
change without bumping PKTGPU_ABI_VERSION.
"""
import numpy as np

MAX_HDRS = 16
ABI_VERSION = 5

# pkt_status_t
OK, TRUNCATED, DEPTH_LIMIT = 0, 1, 2
STATUS_NAMES = ["OK", "TRUNCATED", "DEPTH_LIMIT"]

# pkt_l4_status_t (pkt_l4_checksum_batch)
L4_OK, L4_BAD, L4_UNCHECKED, L4_ABSENT, L4_NO_IP, L4_SPAN, L4_FRAGMENT = range(7)
L4_STATUS = ["OK", "BAD", "UNCHECKED", "ABSENT", "NO_IP", "SPAN", "FRAGMENT"]
L4_LAST = 0xFF
L4_UPDATE, L4_KEEP_ZERO_UDP = 1, 2

# pkt_flow_status_t, the flags and which_ip of pkt_flow_key_batch; pkt_flow_upd_t (pkt_flow_table_update)
FLOW_OK, FLOW_NO_IP, FLOW_SPAN = range(3)
FLOW_STATUS = ["OK", "NO_IP", "SPAN"]
FLOW_LAST = 0xFF
FLOW_SYMMETRIC, FLOW_NO_PORTS = 1, 2
FLOW_UPD_OK, FLOW_UPD_SKIPPED, FLOW_UPD_COLLISION, FLOW_UPD_FULL = range(4)
FLOW_UPD_STATUS = ["OK", "SKIPPED", "COLLISION", "FULL"]
FLOW_NONE = 0xFFFFFFFF  # flow_id of a packet that is not FLOW_UPD_OK

# pkt_match_* (first-match rule tables)
MATCH_MAX_RULES, MATCH_MAX_TERMS = 64, 256
MATCH_NONE = 0xFF  # rule[i] when no rule matched
MATCH_NOT = 1      # term flag: invert the term
MATCH_HAS, MATCH_EQ, MATCH_RANGE, MATCH_LEN = range(4)
MATCH_OPS = ["HAS", "EQ", "RANGE", "LEN"]

# pkt_dispatch_* / pkt_reorder_batch (per-queue batches)
DISPATCH_MAX_BUCKETS, DISPATCH_MAX_TABLE = 256, 4096
DISPATCH_DROP = 0xFFFF  # bucket[i] of a packet no queue takes; a table entry that drops
REORDER_MAX_SEGS = 257

# pkt_lpm_* (longest-prefix-match route tables)
LPM_OK, LPM_NO_ROUTE, LPM_NO_IP, LPM_SPAN, LPM_SKIPPED = range(5)
LPM_STATUS = ["OK", "NO_ROUTE", "NO_IP", "SPAN", "SKIPPED"]
LPM_NONE = 0xFFFFFFFF  # route[i] when status != LPM_OK
LPM_SRC = 1            # flags: look up the source address
LPM_MAX_ROUTES = 1 << 24

# pkt_fwd_* (L3 forwarding rewrite)
(FWD_OK, FWD_SKIPPED, FWD_NO_IP, FWD_SPAN, FWD_NO_ETHER, FWD_TTL, FWD_NO_ADJ, FWD_DROP, FWD_PUNT,
 FWD_MTU) = range(10)
FWD_STATUS = ["OK", "SKIPPED", "NO_IP", "SPAN", "NO_ETHER", "TTL", "NO_ADJ", "DROP", "PUNT", "MTU"]
FWD_STATUS_COUNT = 10
FWD_ACT_FORWARD, FWD_ACT_DROP, FWD_ACT_PUNT = range(3)
FWD_NONE = 0xFFFFFFFF  # port[i] / adj_index[i] when there is none
FWD_KEEP_L2 = 1        # flags: no Ether entry is looked for, no MAC is written
FWD_NO_WRITE = 2       # flags: decide everything, store nothing into the slab
FWD_MAX_ADJ = 1 << 20

# pkt_nat_* (NAPT44 sessions and translation)
(NAT_OK, NAT_SKIPPED, NAT_NO_IP, NAT_SPAN, NAT_IPV6, NAT_BAD_HDR, NAT_FRAGMENT, NAT_NO_L4, NAT_NO_SESSION, NAT_NOT_OURS,
 NAT_EXHAUSTED, NAT_TABLE_FULL) = range(12)
NAT_STATUS = ["OK", "SKIPPED", "NO_IP", "SPAN", "IPV6", "BAD_HDR", "FRAGMENT", "NO_L4", "NO_SESSION", "NOT_OURS",
              "EXHAUSTED", "TABLE_FULL"]
NAT_STATUS_COUNT = 12
NAT_OUT, NAT_IN = 0, 1
NAT_NO_WRITE = 1         # flags: create, refresh and decide, store nothing into the slab
NAT_NONE = 0xFFFFFFFF    # entry[i] of a packet that is not OK
NAT_STATIC = 0x80000000  # entry[i] = NAT_STATIC | the static's index
NAT_REC_STATIC = 1
NAT_MAX_ADDR, NAT_MAX_STATIC = 64, 4096
NAT_PROTOS = (6, 17, 1)  # protocol index p -> IP protocol

# pkt_meter_* (srTCM / trTCM policers): colours, modes, the cfg flag, actions, the call flag, limits
METER_GREEN, METER_YELLOW, METER_RED, METER_UNMETERED = range(4)
METER_COLOR = ["GREEN", "YELLOW", "RED", "UNMETERED"]
METER_COLORS = 4
METER_SRTCM, METER_TRTCM = 0, 1
METER_MODE = {"srtcm": METER_SRTCM, "trtcm": METER_TRTCM}
METER_F_COLOR_AWARE = 1
METER_PASS, METER_DROP, METER_REMARK = range(3)
METER_ACTION = {"pass": METER_PASS, "drop": METER_DROP, "remark": METER_REMARK}
METER_MARK = 1           # call flags: do the REMARK stores
METER_MAX_METERS, METER_MAX_RATE, METER_MAX_BURST = 1 << 24, 1 << 40, 1 << 26
METER_UNIT = 10 ** 9     # bucket units per byte

# pkt_frag_* (IPv4 fragmentation to a per-packet MTU)
(FRAG_FITS, FRAG_SPLIT, FRAG_SKIPPED, FRAG_NO_IP, FRAG_SPAN, FRAG_IPV6, FRAG_BAD_HDR, FRAG_TRUNC, FRAG_DF,
 FRAG_MTU) = range(10)
FRAG_STATUS = ["FITS", "SPLIT", "SKIPPED", "NO_IP", "SPAN", "IPV6", "BAD_HDR", "TRUNC", "DF", "MTU"]
FRAG_STATUS_COUNT = 10
FRAG_ONLY_SPLIT = 1      # flags: a FITS packet gives no output
FRAG_NO_WRITE = 2        # flags: decide and total everything, store no packet byte and no per-output array
FRAG_NONE = 0xFFFFFFFF   # first[i] / src_index[q] when there is none
# pkt_reasm_* (IPv4 reassembly of a batch's fragments)
(REASM_WHOLE, REASM_JOINED, REASM_PENDING, REASM_SKIPPED, REASM_NO_IP, REASM_SPAN, REASM_BAD_HDR, REASM_TRUNC,
 REASM_TOO_BIG) = range(9)
REASM_STATUS = ["WHOLE", "JOINED", "PENDING", "SKIPPED", "NO_IP", "SPAN", "BAD_HDR", "TRUNC", "TOO_BIG"]
REASM_STATUS_COUNT = 9
REASM_ONLY_JOINED = 1    # flags: a WHOLE packet gives no output
REASM_NO_WRITE = 2       # flags: decide and total everything, store no packet byte and no per-output array
REASM_NONE = 0xFFFFFFFF  # out_index[i] / src_index[q] when there is none

# pkt_scan_*: limits, the pattern flag, regions, statuses, placements
SCAN_MAX_PATTERNS = 8192
SCAN_MAX_LEN = 64
SCAN_MAX_BYTES = 131072
SCAN_NONE = 0xFFFFFFFF  # pat[i] when nothing occurs
SCAN_NOCASE = 1
SCAN_PACKET, SCAN_PAYLOAD = range(2)
SCAN_REGION = {"packet": SCAN_PACKET, "payload": SCAN_PAYLOAD}
SCAN_MISS, SCAN_HIT, SCAN_SKIPPED, SCAN_NO_CHAIN, SCAN_SPAN = range(5)
SCAN_STATUS = ["MISS", "HIT", "SKIPPED", "NO_CHAIN", "SPAN"]
SCAN_PLACE_GLOBAL, SCAN_PLACE_LDS = range(2)

# pkt_icmp_err_* (ICMP errors for the packets a router refuses): reasons, statuses, the two default maps
(ICMP_R_NONE, ICMP_R_TIME_EXCEEDED, ICMP_R_TOO_BIG, ICMP_R_NET_UNREACH, ICMP_R_HOST_UNREACH, ICMP_R_PROHIBITED,
 ICMP_R_PORT_UNREACH) = range(7)
ICMP_REASON = ["NONE", "TIME_EXCEEDED", "TOO_BIG", "NET_UNREACH", "HOST_UNREACH", "PROHIBITED", "PORT_UNREACH"]
# reason -> ((type, code) under IPv4, (type, code) under IPv6)
ICMP_TYPE_CODE = {ICMP_R_TIME_EXCEEDED: ((11, 0), (3, 0)), ICMP_R_TOO_BIG: ((3, 4), (2, 0)),
                  ICMP_R_NET_UNREACH: ((3, 0), (1, 0)), ICMP_R_HOST_UNREACH: ((3, 1), (1, 3)),
                  ICMP_R_PROHIBITED: ((3, 13), (1, 1)), ICMP_R_PORT_UNREACH: ((3, 3), (1, 4))}
(ICMPE_SENT, ICMPE_SKIPPED, ICMPE_BAD_REASON, ICMPE_NO_IP, ICMPE_SPAN, ICMPE_NO_ETHER, ICMPE_NO_SRC, ICMPE_BAD_HDR,
 ICMPE_FRAGMENT, ICMPE_BAD_SRC, ICMPE_MCAST, ICMPE_ICMP_ERR) = range(12)
ICMPE_STATUS = ["SENT", "SKIPPED", "BAD_REASON", "NO_IP", "SPAN", "NO_ETHER", "NO_SRC", "BAD_HDR", "FRAGMENT", "BAD_SRC",
                "MCAST", "ICMP_ERR"]
ICMPE_STATUS_COUNT = 12
ICMPE_NO_WRITE = 1        # flags: decide and total everything, store no packet byte and no per-output array
ICMPE_NONE = 0xFFFFFFFF   # out_index[i] / src_index[q] when there is none


def _icmp_map(pairs):
    m = np.zeros(256, np.uint8)
    for k, v in pairs.items():
        m[k] = v
    m.setflags(write=False)
    return m


# code -> reason for Forwarder.run's status (DROP is a silent discard) and for fragment's
ICMP_MAP_FWD = _icmp_map({FWD_TTL: ICMP_R_TIME_EXCEEDED, FWD_MTU: ICMP_R_TOO_BIG, FWD_NO_ADJ: ICMP_R_NET_UNREACH})
ICMP_MAP_FRAG = _icmp_map({FRAG_DF: ICMP_R_TOO_BIG, FRAG_IPV6: ICMP_R_TOO_BIG})

# pkt_tunnel_* (VXLAN / GRE / IP-in-IP encap and decap): kinds, entry flags, the statuses of the two calls
TUN_VXLAN, TUN_GRE, TUN_IPIP = range(3)
TUN_KIND = {"vxlan": TUN_VXLAN, "gre": TUN_GRE, "ipip": TUN_IPIP}
TUN_F_KEY, TUN_F_DF, TUN_F_INHERIT_TOS, TUN_F_UDP_CSUM, TUN_F_ANY_REMOTE = 1, 2, 4, 8, 16
(TUNE_OK, TUNE_SKIPPED, TUNE_NO_TUNNEL, TUNE_NO_IP, TUNE_SPAN, TUNE_BAD_L2, TUNE_BAD_HDR, TUNE_TRUNC, TUNE_TOO_BIG,
 TUNE_DEPTH) = range(10)
TUNE_STATUS = ["OK", "SKIPPED", "NO_TUNNEL", "NO_IP", "SPAN", "BAD_L2", "BAD_HDR", "TRUNC", "TOO_BIG", "DEPTH"]
TUNE_STATUS_COUNT = 10
(TUND_OK, TUND_SKIPPED, TUND_NO_IP, TUND_SPAN, TUND_BAD_HDR, TUND_FRAGMENT, TUND_NOT_TUNNEL, TUND_BAD_GRE, TUND_NO_MATCH,
 TUND_TRUNC, TUND_NO_INNER) = range(11)
TUND_STATUS = ["OK", "SKIPPED", "NO_IP", "SPAN", "BAD_HDR", "FRAGMENT", "NOT_TUNNEL", "BAD_GRE", "NO_MATCH", "TRUNC",
               "NO_INNER"]
TUND_STATUS_COUNT = 11
TUN_NO_WRITE = 1         # call flags: decide and total everything, store no packet byte and no per-output array
TUN_NONE = 0xFFFFFFFF    # out_index[i] / src_index[q] / tunnel_out[i] when there is none
TUN_MAX_ENTRIES = 65536
# pkt_tunnel_entry_t as a numpy record (addresses: wire bytes, IPv4 in the first 4)
TUNNEL_ENTRY_DTYPE = np.dtype([("kind", np.uint8), ("ipver", np.uint8), ("ttl", np.uint8), ("tos", np.uint8),
                               ("flags", np.uint32), ("id", np.uint32), ("sport_lo", np.uint16), ("sport_hi", np.uint16),
                               ("src", np.uint8, 16), ("dst", np.uint8, 16), ("eth_dst", np.uint8, 6),
                               ("eth_src", np.uint8, 6), ("zero", np.uint32)])

# pkt_flow_key_t / pkt_flow_record_t as numpy records
FLOW_KEY_DTYPE = np.dtype([("src", np.uint8, 16), ("dst", np.uint8, 16), ("sport", np.uint16), ("dport", np.uint16),
                           ("proto", np.uint8), ("ipver", np.uint8), ("zero", np.uint16)])
FLOW_RECORD_DTYPE = np.dtype([("key", FLOW_KEY_DTYPE), ("first", np.uint64), ("pkts", np.uint64, 2),
                              ("bytes", np.uint64, 2)])

# pkt_lpm_route_t as a numpy record
LPM_ROUTE_DTYPE = np.dtype([("addr", np.uint8, 16), ("ipver", np.uint8), ("plen", np.uint8), ("zero", np.uint16),
                            ("nexthop", np.uint32)])
# pkt_scan_pattern_t
SCAN_PATTERN_DTYPE = np.dtype([("off", np.uint32), ("len", np.uint16), ("flags", np.uint8), ("group", np.uint8),
                               ("action", np.uint32), ("reserved", np.uint32)])

# pkt_fwd_adj_t as a numpy record
FWD_ADJ_DTYPE = np.dtype([("dmac", np.uint8, 6), ("smac", np.uint8, 6), ("port", np.uint32), ("mtu", np.uint16),
                          ("action", np.uint8), ("zero", np.uint8)])

# pkt_nat_static_t and pkt_nat_record_t as numpy records (addresses: wire bytes; ports: host order)
NAT_STATIC_DTYPE = np.dtype([("in_addr", np.uint8, 4), ("out_addr", np.uint8, 4), ("in_port", np.uint16),
                             ("out_port", np.uint16), ("proto", np.uint8), ("zero", np.uint8, 3)])
NAT_RECORD_DTYPE = np.dtype([("in_addr", np.uint8, 4), ("out_addr", np.uint8, 4), ("in_port", np.uint16),
                             ("out_port", np.uint16), ("proto", np.uint8), ("flags", np.uint8), ("zero", np.uint16),
                             ("last_seen", np.uint32)])

# pkt_meter_cfg_t and pkt_meter_state_t as numpy records
METER_CFG_DTYPE = np.dtype([("cir", np.uint64), ("pir", np.uint64), ("cbs", np.uint32), ("xbs", np.uint32),
                            ("mode", np.uint8), ("flags", np.uint8), ("action", np.uint8, 3), ("dscp", np.uint8, 3)])
METER_STATE_DTYPE = np.dtype([("c", np.uint64), ("x", np.uint64), ("last", np.uint64), ("packets", np.uint64, 3),
                              ("bytes", np.uint64, 3)])

# pkt_hdr_type_t -> Header::name() of the reference (headers.rs:529-827)
HDR_NAMES = [
    "", "Ether", "Vlan", "IPv4", "IPv6", "ICMP", "TCP", "UDP", "ARP", "Vxlan", "Dot3",
    "LLC", "SNAP", "GRE", "GREChksumOffset", "GRESequenceNum", "GREKey", "ERSPAN2",
    "ERSPAN3", "ERSPANPLATFORM", "STP", "MPLS",
]
HDR_ID = {n: i for i, n in enumerate(HDR_NAMES) if n}
HDR_SIZES = [0, 14, 4, 20, 40, 4, 20, 8, 28, 8, 14, 3, 5, 4, 4, 4, 4, 8, 12, 8, 35, 4]

# pkt_entry_t: one per pub fn of parser::fast (fast.rs)
ENTRIES = [
    "parse", "parse_dot3", "parse_llc", "parse_snap", "parse_ethernet", "parse_vlan",
    "parse_mpls", "parse_mpls_bos", "parse_ipv4", "parse_ipv6", "parse_gre",
    "parse_erspan2", "parse_erspan3", "parse_arp", "parse_icmp", "parse_tcp", "parse_udp",
    "parse_vxlan",
]
ENTRY_ID = {n: i for i, n in enumerate(ENTRIES)}

# (column, dtype, per-packet shape, group).  Shape "slots" = slot-major [MAX_HDRS][n].
OUT_COLUMNS = [
    ("status", np.uint8, (), "chain"),
    ("n_hdrs", np.uint8, (), "chain"),
    ("hdr_type", np.uint8, "slots", "chain"),
    ("hdr_off", np.uint16, "slots", "chain"),
    ("payload_off", np.uint16, (), "chain"),
    ("payload_len", np.uint16, (), "chain"),
    ("hdr_mask", np.uint32, (), "chain"),
    ("eth_dst", np.uint64, (), "ether"),
    ("eth_src", np.uint64, (), "ether"),
    ("eth_etype", np.uint16, (), "ether"),
    ("vlan_pcp", np.uint8, (), "vlan"),
    ("vlan_cfi", np.uint8, (), "vlan"),
    ("vlan_vid", np.uint16, (), "vlan"),
    ("vlan_etype", np.uint16, (), "vlan"),
    ("ipv4_version", np.uint8, (), "ipv4"),
    ("ipv4_ihl", np.uint8, (), "ipv4"),
    ("ipv4_diffserv", np.uint8, (), "ipv4"),
    ("ipv4_total_len", np.uint16, (), "ipv4"),
    ("ipv4_identification", np.uint16, (), "ipv4"),
    ("ipv4_flags", np.uint8, (), "ipv4"),
    ("ipv4_frag_startset", np.uint16, (), "ipv4"),
    ("ipv4_ttl", np.uint8, (), "ipv4"),
    ("ipv4_protocol", np.uint8, (), "ipv4"),
    ("ipv4_header_checksum", np.uint16, (), "ipv4"),
    ("ipv4_src", np.uint32, (), "ipv4"),
    ("ipv4_dst", np.uint32, (), "ipv4"),
    ("ipv4_csum_calc", np.uint16, (), "ipv4"),
    ("ipv6_version", np.uint8, (), "ipv6"),
    ("ipv6_traffic_class", np.uint8, (), "ipv6"),
    ("ipv6_flow_label", np.uint32, (), "ipv6"),
    ("ipv6_payload_len", np.uint16, (), "ipv6"),
    ("ipv6_next_hdr", np.uint8, (), "ipv6"),
    ("ipv6_hop_limit", np.uint8, (), "ipv6"),
    ("ipv6_src", np.uint8, (16,), "ipv6"),
    ("ipv6_dst", np.uint8, (16,), "ipv6"),
    ("tcp_src", np.uint16, (), "tcp"),
    ("tcp_dst", np.uint16, (), "tcp"),
    ("tcp_seq_no", np.uint32, (), "tcp"),
    ("tcp_ack_no", np.uint32, (), "tcp"),
    ("tcp_data_startset", np.uint8, (), "tcp"),
    ("tcp_res", np.uint8, (), "tcp"),
    ("tcp_flags", np.uint8, (), "tcp"),
    ("tcp_window", np.uint16, (), "tcp"),
    ("tcp_checksum", np.uint16, (), "tcp"),
    ("tcp_urgent_ptr", np.uint16, (), "tcp"),
    ("udp_src", np.uint16, (), "udp"),
    ("udp_dst", np.uint16, (), "udp"),
    ("udp_length", np.uint16, (), "udp"),
    ("udp_checksum", np.uint16, (), "udp"),
]
COLUMN_NAMES = [c[0] for c in OUT_COLUMNS]
GROUPS = ["chain", "ether", "vlan", "ipv4", "ipv6", "tcp", "udp"]


def columns_of(groups):
    """Column names of the given groups (e.g. ["chain", "ether", "ipv4", "udp"])."""
    groups = set(groups)
    bad = groups - set(GROUPS)
    if bad:
        raise ValueError(f"unknown column groups {sorted(bad)}")
    return [c[0] for c in OUT_COLUMNS if c[3] in groups]


def column_shape(name, n):
    """numpy shape of column `name` for a batch of n packets."""
    for c, dt, shp, _ in OUT_COLUMNS:
        if c == name:
            if shp == "slots":
                return (MAX_HDRS, n)
            return (n,) + tuple(shp)
    raise KeyError(name)


def column_dtype(name):
    for c, dt, _, _ in OUT_COLUMNS:
        if c == name:
            return np.dtype(dt)
    raise KeyError(name)


def column_mask(columns):
    """pkt_out_t column mask (bit k = k-th member) of a set of column names."""
    cols = set(columns)
    return sum(1 << k for k, c in enumerate(COLUMN_NAMES) if c in cols)


def bytes_per_packet(columns, n_slots=MAX_HDRS):
    """Bytes written per packet for a column set; slot columns count `n_slots` slots."""
    total = 0
    for c, dt, shp, _ in OUT_COLUMNS:
        if c not in columns:
            continue
        isz = np.dtype(dt).itemsize
        if shp == "slots":
            total += isz * n_slots
        else:
            total += isz * int(np.prod(shp)) if shp else isz
    return total
