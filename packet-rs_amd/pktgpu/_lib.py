"""ctypes binding of lib/libpktgpu.so (the C ABI of include/pktgpu.h).

There is no fallback: if the library is missing or fails to load, importing raises.  Import
torch before this module so that the HIP runtime torch loaded (same soname,
libamdhip64.so.7) is the one the library binds to, and device pointers are shared.
"""
import ctypes
import os

from . import schema

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
# PKTGPU_LIB overrides the library path (A/B builds of the same ABI in one session).
LIB_PATH = os.environ.get("PKTGPU_LIB") or os.path.join(PKG_ROOT, "lib", "libpktgpu.so")


class PktBatch(ctypes.Structure):
    _fields_ = [("slab", ctypes.c_void_p), ("slab_len", ctypes.c_uint64),
                ("offsets", ctypes.c_void_p), ("lens", ctypes.c_void_p),
                ("stride", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("n", ctypes.c_uint64)]


class PktOut(ctypes.Structure):
    _fields_ = [(c, ctypes.c_void_p) for c in schema.COLUMN_NAMES]


class PktChain(ctypes.Structure):
    _fields_ = [("n_hdrs", ctypes.c_void_p), ("hdr_type", ctypes.c_void_p),
                ("hdr_off", ctypes.c_void_p)]


class PktFieldSpec(ctypes.Structure):
    _fields_ = [("hdr_type", ctypes.c_uint8), ("occurrence", ctypes.c_uint8),
                ("start", ctypes.c_uint16), ("end", ctypes.c_uint16),
                ("reserved", ctypes.c_uint16)]


class PktCmpSummary(ctypes.Structure):
    _fields_ = [("n_equal", ctypes.c_uint64), ("n_len", ctypes.c_uint64), ("n_bytes", ctypes.c_uint64),
                ("first_bad", ctypes.c_uint64)]


class PktEditOp(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint8), ("hdr_type", ctypes.c_uint8), ("index", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8), ("data_off", ctypes.c_uint32)]


class PktGatherPiece(ctypes.Structure):
    _fields_ = [("src", ctypes.c_uint64), ("dst", ctypes.c_uint64), ("bytes", ctypes.c_uint64),
                ("shard", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


class PktGenField(ctypes.Structure):
    _fields_ = [("field", PktFieldSpec), ("kind", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("base", ctypes.c_uint64), ("step", ctypes.c_uint64), ("count", ctypes.c_uint64)]


class PktFlowKey(ctypes.Structure):
    _fields_ = [("src", ctypes.c_uint8 * 16), ("dst", ctypes.c_uint8 * 16), ("sport", ctypes.c_uint16),
                ("dport", ctypes.c_uint16), ("proto", ctypes.c_uint8), ("ipver", ctypes.c_uint8),
                ("zero", ctypes.c_uint16)]


class PktFlowRecord(ctypes.Structure):
    _fields_ = [("key", PktFlowKey), ("first", ctypes.c_uint64), ("pkts", ctypes.c_uint64 * 2),
                ("bytes", ctypes.c_uint64 * 2)]


class PktMatchTerm(ctypes.Structure):
    _fields_ = [("field", PktFieldSpec), ("op", ctypes.c_uint8), ("flags", ctypes.c_uint8),
                ("reserved", ctypes.c_uint16), ("reserved2", ctypes.c_uint32), ("a", ctypes.c_uint64),
                ("b", ctypes.c_uint64)]


class PktMatchRule(ctypes.Structure):
    _fields_ = [("first_term", ctypes.c_uint16), ("nterms", ctypes.c_uint16), ("action", ctypes.c_uint32)]


class PktLpmRoute(ctypes.Structure):
    _fields_ = [("addr", ctypes.c_uint8 * 16), ("ipver", ctypes.c_uint8), ("plen", ctypes.c_uint8),
                ("zero", ctypes.c_uint16), ("nexthop", ctypes.c_uint32)]


class PktScanPattern(ctypes.Structure):
    _fields_ = [("off", ctypes.c_uint32), ("len", ctypes.c_uint16), ("flags", ctypes.c_uint8), ("group", ctypes.c_uint8),
                ("action", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class PktScanInfo(ctypes.Structure):
    _fields_ = [("npatterns", ctypes.c_uint32), ("nstates", ctypes.c_uint32), ("max_len", ctypes.c_uint32),
                ("placement", ctypes.c_uint32), ("table_bytes", ctypes.c_uint64)]


class PktLpmInfo(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint64) for k in ("routes_v4", "routes_v6", "nodes_v4", "nodes_v6", "depth_v4", "depth_v6",
                                               "bytes")]


class PktIcmpCfg(ctypes.Structure):
    _fields_ = [("src4", ctypes.c_uint8 * 4), ("src6", ctypes.c_uint8 * 16), ("max4", ctypes.c_uint16),
                ("max6", ctypes.c_uint16), ("ident", ctypes.c_uint16), ("ttl", ctypes.c_uint8), ("tos", ctypes.c_uint8)]


class PktNatStatic(ctypes.Structure):
    _fields_ = [("in_addr", ctypes.c_uint8 * 4), ("out_addr", ctypes.c_uint8 * 4), ("in_port", ctypes.c_uint16),
                ("out_port", ctypes.c_uint16), ("proto", ctypes.c_uint8), ("zero", ctypes.c_uint8 * 3)]


class PktNatRecord(ctypes.Structure):
    _fields_ = [("in_addr", ctypes.c_uint8 * 4), ("out_addr", ctypes.c_uint8 * 4), ("in_port", ctypes.c_uint16),
                ("out_port", ctypes.c_uint16), ("proto", ctypes.c_uint8), ("flags", ctypes.c_uint8),
                ("zero", ctypes.c_uint16), ("last_seen", ctypes.c_uint32)]


class PktMeterCfg(ctypes.Structure):
    _fields_ = [("cir", ctypes.c_uint64), ("pir", ctypes.c_uint64), ("cbs", ctypes.c_uint32), ("xbs", ctypes.c_uint32),
                ("mode", ctypes.c_uint8), ("flags", ctypes.c_uint8), ("action", ctypes.c_uint8 * 3),
                ("dscp", ctypes.c_uint8 * 3)]


class PktMeterState(ctypes.Structure):
    _fields_ = [("c", ctypes.c_uint64), ("x", ctypes.c_uint64), ("last", ctypes.c_uint64),
                ("packets", ctypes.c_uint64 * 3), ("bytes", ctypes.c_uint64 * 3)]


class PktTunnelEntry(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint8), ("ipver", ctypes.c_uint8), ("ttl", ctypes.c_uint8), ("tos", ctypes.c_uint8),
                ("flags", ctypes.c_uint32), ("id", ctypes.c_uint32), ("sport_lo", ctypes.c_uint16),
                ("sport_hi", ctypes.c_uint16), ("src", ctypes.c_uint8 * 16), ("dst", ctypes.c_uint8 * 16),
                ("eth_dst", ctypes.c_uint8 * 6), ("eth_src", ctypes.c_uint8 * 6), ("zero", ctypes.c_uint32)]


class PktFwdAdj(ctypes.Structure):
    _fields_ = [("dmac", ctypes.c_uint8 * 6), ("smac", ctypes.c_uint8 * 6), ("port", ctypes.c_uint32),
                ("mtu", ctypes.c_uint16), ("action", ctypes.c_uint8), ("zero", ctypes.c_uint8)]


# Every function declared in include/pktgpu.h: name -> (restype, argtypes)
_P = ctypes.c_void_p
SIGNATURES = {
    "pkt_abi_version": (ctypes.c_int, []),
    "pkt_sizeof_batch": (ctypes.c_size_t, []),
    "pkt_sizeof_out": (ctypes.c_size_t, []),
    "pkt_sizeof_field_spec": (ctypes.c_size_t, []),
    "pkt_hdr_name": (ctypes.c_char_p, [ctypes.c_int]),
    "pkt_hdr_size": (ctypes.c_int, [ctypes.c_int]),
    "pkt_hdr_field_count": (ctypes.c_int, [ctypes.c_int]),
    "pkt_hdr_field": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p),
                                     ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint16)]),
    "pkt_status_name": (ctypes.c_char_p, [ctypes.c_int]),
    "pkt_entry_name": (ctypes.c_char_p, [ctypes.c_int]),
    "pkt_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_P)]),
    "pkt_ctx_destroy": (ctypes.c_int, [_P]),
    "pkt_ctx_last_error": (ctypes.c_char_p, [_P]),
    "pkt_ctx_set_window": (ctypes.c_int, [_P, ctypes.c_uint32]),
    "pkt_ctx_set_fastpath": (ctypes.c_int, [_P, ctypes.c_int]),
    "pkt_ctx_set_staging": (ctypes.c_int, [_P, ctypes.c_int]),
    "pkt_ctx_set_walk": (ctypes.c_int, [_P, ctypes.c_int]),
    "pkt_ctx_set_host_piece": (ctypes.c_int, [_P, ctypes.c_uint64]),
    "pkt_ctx_set_pcap_scan64": (ctypes.c_int, [_P, ctypes.c_int]),
    "pkt_parse_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.c_int,
                                       ctypes.POINTER(PktOut), _P]),
    "pkt_parse_batches": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.c_uint32, ctypes.c_int,
                                         ctypes.POINTER(PktOut), _P]),
    "pkt_parse_host": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.c_int, ctypes.POINTER(PktOut),
                                      ctypes.c_uint64]),
    "pkt_parse_pcap_host": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(PktOut),
                                           _P, _P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_host_alloc": (ctypes.c_int, [_P, ctypes.c_uint64, ctypes.POINTER(_P)]),
    "pkt_host_free": (ctypes.c_int, [_P, _P]),
    "pkt_extract_fields": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain),
                                          ctypes.POINTER(PktFieldSpec), ctypes.c_uint32,
                                          ctypes.POINTER(_P), ctypes.POINTER(_P), _P]),
    "pkt_to_vec_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktOut), _P,
                                        ctypes.c_uint64, _P, _P, _P]),
    "pkt_set_fields": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain),
                                      ctypes.POINTER(PktFieldSpec), ctypes.c_uint32,
                                      ctypes.POINTER(_P), _P]),
    "pkt_set_fields_csum": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain),
                                           ctypes.POINTER(PktFieldSpec), ctypes.c_uint32,
                                           ctypes.POINTER(_P), ctypes.c_int32, _P]),
    "pkt_ipv4_update_checksum": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain),
                                                ctypes.c_uint32, _P]),
    "pkt_broadcast": (ctypes.c_int, [_P, _P, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, _P, _P]),
    "pkt_sizeof_gen_field": (ctypes.c_size_t, []),
    "pkt_gen_create": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_int,
                                      ctypes.POINTER(PktGenField), ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.POINTER(_P)]),
    "pkt_gen_run": (ctypes.c_int, [_P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                   ctypes.POINTER(_P), _P, _P]),
    "pkt_gen_destroy": (ctypes.c_int, [_P]),
    "pkt_ipv4_checksum_batch": (ctypes.c_int, [_P, _P, ctypes.c_uint32, ctypes.c_uint64, _P, _P]),
    "pkt_pcap_index": (ctypes.c_int, [_P, ctypes.c_uint64, _P, _P, ctypes.c_uint64,
                                      ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_pcap_index_device": (ctypes.c_int, [_P, _P, ctypes.c_uint64, _P, _P, ctypes.c_uint64,
                                             ctypes.POINTER(ctypes.c_uint64), _P]),
    "pkt_pcap_index_device_timed": (ctypes.c_int, [_P, _P, ctypes.c_uint64, _P, _P, ctypes.c_uint64,
                                                   ctypes.POINTER(ctypes.c_uint64), _P,
                                                   ctypes.POINTER(ctypes.c_float)]),
    "pkt_parse_pcap": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(PktOut), _P, _P,
                                      ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), _P]),
    "pkt_parse_pcap_host_async": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(PktOut),
                                                 ctypes.c_uint64]),
    "pkt_parse_pcap_host_result": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_parse_pcap_async": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(PktOut), _P, _P,
                                            ctypes.c_uint64, _P]),
    "pkt_parse_pcap_result": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_pcap_write": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), _P, ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.c_uint32, _P, _P, _P, ctypes.c_uint64, _P, _P, _P,
                                      ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), _P]),
    "pkt_pcap_write_async": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), _P, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_uint32, _P, _P, _P, ctypes.c_uint64, _P, _P, _P, _P]),
    "pkt_pcap_write_result": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64),
                                             ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_pcap_write_host": (ctypes.c_int, [ctypes.POINTER(PktBatch), _P, ctypes.c_uint32, ctypes.c_uint32,
                                           ctypes.c_uint32, _P, _P, _P, ctypes.c_uint64, _P, _P, _P,
                                           ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_sizeof_cmp_summary": (ctypes.c_size_t, []),
    "pkt_compare_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktBatch),
                                         ctypes.POINTER(PktChain), ctypes.POINTER(PktFieldSpec), ctypes.c_uint32,
                                         _P, _P, _P, ctypes.POINTER(PktCmpSummary), _P]),
    "pkt_compare_batch_async": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktBatch),
                                               ctypes.POINTER(PktChain), ctypes.POINTER(PktFieldSpec),
                                               ctypes.c_uint32, _P, _P, _P, _P]),
    "pkt_compare_result": (ctypes.c_int, [_P, ctypes.POINTER(PktCmpSummary)]),
    "pkt_compare_host": (ctypes.c_int, [ctypes.POINTER(PktBatch), ctypes.POINTER(PktBatch),
                                        ctypes.POINTER(PktChain), ctypes.POINTER(PktFieldSpec), ctypes.c_uint32,
                                        _P, _P, _P, ctypes.POINTER(PktCmpSummary)]),
    "pkt_sizeof_edit_op": (ctypes.c_size_t, []),
    "pkt_edit_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktOut), ctypes.POINTER(PktEditOp),
                                      ctypes.c_uint32, _P, ctypes.c_uint32, _P, _P, ctypes.c_uint64, _P, ctypes.c_uint32,
                                      _P, _P, ctypes.POINTER(PktOut), _P]),
    "pkt_edit_host": (ctypes.c_int, [ctypes.POINTER(PktBatch), ctypes.POINTER(PktOut), ctypes.POINTER(PktEditOp),
                                     ctypes.c_uint32, _P, ctypes.c_uint32, _P, _P, ctypes.c_uint64, _P, ctypes.c_uint32,
                                     _P, _P, ctypes.POINTER(PktOut)]),
    "pkt_l4_checksum_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                             ctypes.c_uint32, _P, _P, _P, _P]),
    "pkt_l4_checksum_host": (ctypes.c_int, [ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                            ctypes.c_uint32, _P, _P, _P]),
    "pkt_sizeof_flow_key": (ctypes.c_size_t, []),
    "pkt_flow_key_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                          ctypes.c_uint32, ctypes.c_uint64, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pkt_flow_key_host": (ctypes.c_int, [ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                         ctypes.c_uint32, ctypes.c_uint64, _P, _P, _P, _P, _P, _P, _P]),
    "pkt_sizeof_flow_record": (ctypes.c_size_t, []),
    "pkt_flow_table_create": (ctypes.c_int, [_P, ctypes.c_uint64, ctypes.POINTER(_P)]),
    "pkt_flow_table_create_host": (ctypes.c_int, [ctypes.c_uint64, ctypes.POINTER(_P)]),
    "pkt_flow_table_set_tag_bits": (ctypes.c_int, [_P, ctypes.c_uint32]),
    "pkt_flow_table_update": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint64, _P, _P, _P]),
    "pkt_flow_table_count": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), _P]),
    "pkt_flow_table_export": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), _P]),
    "pkt_flow_table_clear": (ctypes.c_int, [_P, _P]),
    "pkt_flow_table_destroy": (ctypes.c_int, [_P]),
    "pkt_flow_table_last_error": (ctypes.c_char_p, [_P]),
    "pkt_sizeof_match_term": (ctypes.c_size_t, []),
    "pkt_sizeof_match_rule": (ctypes.c_size_t, []),
    "pkt_match_create": (ctypes.c_int, [_P, ctypes.POINTER(PktMatchTerm), ctypes.c_uint32, ctypes.POINTER(PktMatchRule),
                                        ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_P)]),
    "pkt_match_destroy": (ctypes.c_int, [_P]),
    "pkt_match_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), _P, _P, _P, _P, _P, _P,
                                       _P]),
    "pkt_match_host": (ctypes.c_int, [ctypes.POINTER(PktMatchTerm), ctypes.c_uint32, ctypes.POINTER(PktMatchRule),
                                      ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(PktBatch),
                                      ctypes.POINTER(PktChain), _P, _P, _P, _P, _P, _P]),
    "pkt_dispatch_create": (ctypes.c_int, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, ctypes.c_uint64,
                                           ctypes.POINTER(_P)]),
    "pkt_dispatch_destroy": (ctypes.c_int, [_P]),
    "pkt_dispatch_batch": (ctypes.c_int, [_P, _P, _P, ctypes.c_uint64, _P, _P, _P, _P, _P]),
    "pkt_dispatch_host": (ctypes.c_int, [ctypes.c_uint32, _P, ctypes.c_uint32, _P, _P, ctypes.c_uint64, _P, _P, _P,
                                         _P]),
    "pkt_reorder_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktOut), _P, ctypes.c_uint64,
                                         _P, ctypes.c_uint32, _P, ctypes.c_uint64, ctypes.c_uint32, _P,
                                         ctypes.POINTER(PktOut), _P]),
    "pkt_reorder_host": (ctypes.c_int, [ctypes.POINTER(PktBatch), ctypes.POINTER(PktOut), _P, ctypes.c_uint64, _P,
                                        ctypes.c_uint32, _P, ctypes.c_uint64, ctypes.c_uint32, _P,
                                        ctypes.POINTER(PktOut)]),
    "pkt_sizeof_lpm_route": (ctypes.c_size_t, []),
    "pkt_lpm_create": (ctypes.c_int, [_P, _P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(_P)]),
    "pkt_lpm_create_host": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(_P)]),
    "pkt_lpm_info": (ctypes.c_int, [_P, ctypes.POINTER(PktLpmInfo)]),
    "pkt_lpm_lookup_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                            ctypes.c_uint32, _P, _P, _P, _P, _P]),
    "pkt_lpm_lookup_keys": (ctypes.c_int, [_P, _P, _P, ctypes.c_uint64, ctypes.c_uint32, _P, _P, _P, _P, _P]),
    "pkt_lpm_destroy": (ctypes.c_int, [_P]),
    "pkt_lpm_last_error": (ctypes.c_char_p, [_P]),
    "pkt_sizeof_fwd_adj": (ctypes.c_size_t, []),
    "pkt_fwd_create": (ctypes.c_int, [_P, _P, ctypes.c_uint32, ctypes.POINTER(_P)]),
    "pkt_fwd_destroy": (ctypes.c_int, [_P]),
    "pkt_fwd_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                     ctypes.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pkt_fwd_host": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain),
                                    ctypes.c_uint32, ctypes.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pkt_frag_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                      ctypes.c_uint32, _P, ctypes.c_uint32, _P, _P, _P, _P, _P, ctypes.c_uint64,
                                      ctypes.c_uint64, _P, _P, _P, _P, ctypes.POINTER(PktChain), _P,
                                      ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), _P]),
    "pkt_frag_batch_async": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                            ctypes.c_uint32, _P, ctypes.c_uint32, _P, _P, _P, _P, _P, ctypes.c_uint64,
                                            ctypes.c_uint64, _P, _P, _P, _P, ctypes.POINTER(PktChain), _P, _P]),
    "pkt_frag_result": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_frag_host": (ctypes.c_int, [ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                     ctypes.c_uint32, _P, ctypes.c_uint32, _P, _P, _P, _P, _P, ctypes.c_uint64,
                                     ctypes.c_uint64, _P, _P, _P, _P, ctypes.POINTER(PktChain), _P,
                                     ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_reasm_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                       ctypes.c_uint32, _P, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint64, _P, _P, _P, _P,
                                       ctypes.POINTER(PktChain), _P, ctypes.POINTER(ctypes.c_uint64),
                                       ctypes.POINTER(ctypes.c_uint64), _P]),
    "pkt_reasm_batch_async": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                             ctypes.c_uint32, _P, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint64, _P, _P, _P,
                                             _P, ctypes.POINTER(PktChain), _P, _P]),
    "pkt_reasm_result": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_reasm_host": (ctypes.c_int, [ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                      ctypes.c_uint32, _P, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint64, _P, _P, _P, _P,
                                      ctypes.POINTER(PktChain), _P, ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_sizeof_scan_pattern": (ctypes.c_size_t, []),
    "pkt_scan_create": (ctypes.c_int, [_P, _P, ctypes.c_uint64, _P, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_P)]),
    "pkt_scan_create_host": (ctypes.c_int, [_P, ctypes.c_uint64, _P, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_P)]),
    "pkt_scan_info": (ctypes.c_int, [_P, ctypes.POINTER(PktScanInfo)]),
    "pkt_scan_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                      _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pkt_scan_destroy": (ctypes.c_int, [_P]),
    "pkt_scan_last_error": (ctypes.c_char_p, [_P]),
    "pkt_sizeof_icmp_cfg": (ctypes.c_size_t, []),
    "pkt_icmp_err_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                          ctypes.c_uint32, ctypes.POINTER(PktIcmpCfg), _P, ctypes.c_uint32, _P, _P,
                                          ctypes.c_uint32, _P, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint64, _P, _P, _P,
                                          ctypes.POINTER(PktChain), _P, ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.POINTER(ctypes.c_uint64), _P]),
    "pkt_icmp_err_batch_async": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                                ctypes.c_uint32, ctypes.POINTER(PktIcmpCfg), _P, ctypes.c_uint32, _P, _P,
                                                ctypes.c_uint32, _P, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint64, _P, _P,
                                                _P, ctypes.POINTER(PktChain), _P, _P]),
    "pkt_icmp_err_result": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_icmp_err_host": (ctypes.c_int, [ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                         ctypes.c_uint32, ctypes.POINTER(PktIcmpCfg), _P, ctypes.c_uint32, _P, _P,
                                         ctypes.c_uint32, _P, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint64, _P, _P, _P,
                                         ctypes.POINTER(PktChain), _P, ctypes.POINTER(ctypes.c_uint64),
                                         ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_sizeof_nat_static": (ctypes.c_size_t, []),
    "pkt_sizeof_nat_record": (ctypes.c_size_t, []),
    "pkt_nat_create": (ctypes.c_int, [_P, _P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, _P,
                                      ctypes.c_uint32, ctypes.POINTER(_P)]),
    "pkt_nat_create_host": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, _P,
                                           ctypes.c_uint32, ctypes.POINTER(_P)]),
    "pkt_nat_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                     ctypes.c_uint32, ctypes.c_uint32, _P, _P, ctypes.c_uint32, _P, _P, _P, _P, _P, _P]),
    "pkt_nat_expire": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                      ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_nat_count": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_nat_export": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_nat_clear": (ctypes.c_int, [_P, _P]),
    "pkt_nat_destroy": (ctypes.c_int, [_P]),
    "pkt_nat_last_error": (ctypes.c_char_p, [_P]),
    "pkt_sizeof_meter_cfg": (ctypes.c_size_t, []),
    "pkt_sizeof_meter_state": (ctypes.c_size_t, []),
    "pkt_meter_create": (ctypes.c_int, [_P, _P, ctypes.c_uint32, ctypes.c_int32, ctypes.POINTER(_P)]),
    "pkt_meter_create_host": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_int32, ctypes.POINTER(_P)]),
    "pkt_meter_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                       ctypes.c_uint32, ctypes.c_uint32, _P, ctypes.c_uint64, _P, _P, _P, _P, _P, _P, _P,
                                       _P, _P]),
    "pkt_meter_reset": (ctypes.c_int, [_P, _P]),
    "pkt_meter_export": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, _P]),
    "pkt_meter_destroy": (ctypes.c_int, [_P]),
    "pkt_meter_last_error": (ctypes.c_char_p, [_P]),
    "pkt_sizeof_tunnel_entry": (ctypes.c_size_t, []),
    "pkt_tunnel_create": (ctypes.c_int, [_P, _P, ctypes.c_uint32, ctypes.POINTER(_P)]),
    "pkt_tunnel_create_host": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.POINTER(_P)]),
    "pkt_tunnel_destroy": (ctypes.c_int, [_P]),
    "pkt_tunnel_last_error": (ctypes.c_char_p, [_P]),
    "pkt_tunnel_encap_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                              ctypes.c_uint32, _P, _P, ctypes.c_uint32, _P, ctypes.c_uint32, _P, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint64, _P, _P, _P, ctypes.POINTER(PktChain), _P,
                                              ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), _P]),
    "pkt_tunnel_encap_batch_async": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain),
                                                    ctypes.c_uint32, ctypes.c_uint32, _P, _P, ctypes.c_uint32, _P, ctypes.c_uint32,
                                                    _P, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint64, _P, _P, _P,
                                                    ctypes.POINTER(PktChain), _P, _P]),
    "pkt_tunnel_encap_result": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_tunnel_encap_host": (ctypes.c_int, [ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                             ctypes.c_uint32, _P, _P, ctypes.c_uint32, _P, ctypes.c_uint32, _P, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint64, _P, _P, _P, ctypes.POINTER(PktChain), _P,
                                             ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_tunnel_decap_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                              ctypes.c_uint32, _P, _P, _P, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint64, _P, _P,
                                              _P, ctypes.POINTER(PktChain), _P, ctypes.POINTER(ctypes.c_uint64),
                                              ctypes.POINTER(ctypes.c_uint64), _P]),
    "pkt_tunnel_decap_batch_async": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain),
                                                    ctypes.c_uint32, ctypes.c_uint32, _P, _P, _P, _P, _P, _P, ctypes.c_uint64,
                                                    ctypes.c_uint64, _P, _P, _P, ctypes.POINTER(PktChain), _P, _P]),
    "pkt_tunnel_decap_result": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_tunnel_decap_host": (ctypes.c_int, [ctypes.POINTER(PktBatch), ctypes.POINTER(PktChain), ctypes.c_uint32,
                                             ctypes.c_uint32, _P, _P, _P, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint64, _P, _P,
                                             _P, ctypes.POINTER(PktChain), _P, ctypes.POINTER(ctypes.c_uint64),
                                             ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_ipv4_checksum_host": (ctypes.c_uint16, [ctypes.c_char_p, ctypes.c_size_t]),
    # packed outputs + multi-GPU (pkt_mgpu_*)
    "pkt_out_packed": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, _P, ctypes.POINTER(PktOut),
                                      ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_out_packed_pieces": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                             ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                             ctypes.POINTER(ctypes.c_int)]),
    "pkt_chain_max_hdrs": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32), _P]),
    "pkt_out_mask": (ctypes.c_uint64, [ctypes.POINTER(PktOut)]),
    "pkt_view": (ctypes.c_int, [ctypes.POINTER(PktOut), ctypes.c_uint64, ctypes.c_uint64,
                                ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint16),
                                ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint16),
                                ctypes.POINTER(ctypes.c_uint16)]),
    "pkt_sizeof_gather_piece": (ctypes.c_size_t, []),
    "pkt_gather_plan": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                                       ctypes.POINTER(ctypes.c_uint32), ctypes.c_int,
                                       ctypes.POINTER(PktGatherPiece), ctypes.c_uint64,
                                       ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_mgpu_set_root_copy": (ctypes.c_int, [_P, ctypes.c_int]),
    "pkt_mgpu_set_gather_rows": (ctypes.c_int, [_P, ctypes.c_int]),
    "pkt_shard_range": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_pcap_stream_open": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                            ctypes.POINTER(PktOut), ctypes.c_uint64, ctypes.POINTER(_P)]),
    "pkt_pcap_stream_push": (ctypes.c_int, [_P, _P, ctypes.c_uint64]),
    "pkt_pcap_stream_poll": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), _P, _P]),
    "pkt_pcap_stream_finish": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), _P, _P]),
    "pkt_pcap_stream_release": (ctypes.c_int, [_P, ctypes.c_uint64]),
    "pkt_pcap_stream_room": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_pcap_stream_released": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_pcap_stream_batch": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch)]),
    "pkt_pcap_stream_ctx": (_P, [_P]),
    "pkt_pcap_stream_last_error": (ctypes.c_char_p, [_P]),
    "pkt_pcap_stream_close": (ctypes.c_int, [_P]),
    "pkt_mgpu_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(_P)]),
    "pkt_mgpu_create_virtual": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(_P)]),
    "pkt_mgpu_is_virtual": (ctypes.c_int, [_P]),
    "pkt_mgpu_destroy": (ctypes.c_int, [_P]),
    "pkt_mgpu_ndev": (ctypes.c_int, [_P]),
    "pkt_mgpu_last_error": (ctypes.c_char_p, [_P]),
    "pkt_mgpu_ctx": (_P, [_P, ctypes.c_int]),
    "pkt_mgpu_stream": (_P, [_P, ctypes.c_int]),
    "pkt_mgpu_parse": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.c_int, ctypes.c_uint64,
                                      ctypes.POINTER(_P)]),
    "pkt_mgpu_parse_steps": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.c_int, ctypes.c_int,
                                            ctypes.c_uint64, ctypes.POINTER(_P), ctypes.c_int]),
    "pkt_mgpu_gather": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_uint64),
                                       _P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    "pkt_mgpu_parse_gather": (ctypes.c_int, [_P, ctypes.POINTER(PktBatch), ctypes.c_int, ctypes.c_uint64,
                                             ctypes.POINTER(_P), ctypes.c_int, _P, ctypes.c_uint64,
                                             ctypes.c_int, ctypes.POINTER(PktOut)]),
    "pkt_mgpu_synchronize": (ctypes.c_int, [_P]),
}

_lib = None


def load():
    """Load libpktgpu.so and declare every prototype; raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C packet-rs_amd` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    if L.pkt_abi_version() != schema.ABI_VERSION:
        raise ImportError("libpktgpu ABI version mismatch")
    if L.pkt_sizeof_out() != ctypes.sizeof(PktOut) or L.pkt_sizeof_batch() != ctypes.sizeof(PktBatch) \
            or L.pkt_sizeof_field_spec() != ctypes.sizeof(PktFieldSpec) \
            or L.pkt_sizeof_gen_field() != ctypes.sizeof(PktGenField) \
            or L.pkt_sizeof_gather_piece() != ctypes.sizeof(PktGatherPiece) \
            or L.pkt_sizeof_cmp_summary() != ctypes.sizeof(PktCmpSummary) \
            or L.pkt_sizeof_edit_op() != ctypes.sizeof(PktEditOp) \
            or L.pkt_sizeof_flow_key() != ctypes.sizeof(PktFlowKey) \
            or L.pkt_sizeof_flow_record() != ctypes.sizeof(PktFlowRecord) \
            or L.pkt_sizeof_match_term() != ctypes.sizeof(PktMatchTerm) \
            or L.pkt_sizeof_match_rule() != ctypes.sizeof(PktMatchRule) \
            or L.pkt_sizeof_lpm_route() != ctypes.sizeof(PktLpmRoute) \
            or L.pkt_sizeof_scan_pattern() != ctypes.sizeof(PktScanPattern) \
            or L.pkt_sizeof_fwd_adj() != ctypes.sizeof(PktFwdAdj) \
            or L.pkt_sizeof_nat_static() != ctypes.sizeof(PktNatStatic) \
            or L.pkt_sizeof_nat_record() != ctypes.sizeof(PktNatRecord) \
            or L.pkt_sizeof_meter_cfg() != ctypes.sizeof(PktMeterCfg) \
            or L.pkt_sizeof_meter_state() != ctypes.sizeof(PktMeterState) \
            or L.pkt_sizeof_tunnel_entry() != ctypes.sizeof(PktTunnelEntry):
        raise ImportError("libpktgpu struct layout mismatch with pktgpu/_lib.py")
    _lib = L
    return L
