/*
 * pktgpu.h — C ABI of the MI355X-native batched packet-header parser.
 *
 * This is the drop-in boundary for packet_rs 0.4.0's decode path:
 *   - the protocol walk `parser::fast::parse` and its 17 sub-entries
 *     (reference src/parser/fast.rs:5-227),
 *   - the `make_header!` MSB-first bit-field getters of the Slice headers
 *     (reference src/headers.rs:195-201 getters, 202-211 bytes(), 252-263 bit_range,
 *      field tables 529-827),
 *   - `Packet::ipv4_checksum` (reference src/packet.rs:93-107, incl. its carry-fold quirk).
 *
 * The reference is a Rust crate with no FFI of its own; these entry points are what a
 * Rust `extern "C"` block binds in place of calling
 * `fast::parse(&[u8]) -> PacketSlice` once per packet.  Everything here is plain C:
 * pointers, sizes and status codes.  No HIP, torch or C++ types cross the boundary
 * (streams are passed as `void*` = hipStream_t, 0 = the null stream).
 *
 * Errors: every function returns an int, 0 on success and a negative PKT_ERR_* code
 * otherwise.  Nothing panics or aborts across the ABI (the reference panics on short
 * input, fast.rs:6 and every `&arr[0..X::size()]`; here that is a per-packet
 * PKT_TRUNCATED status instead).
 */
#ifndef PKTGPU_H
#define PKTGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PKTGPU_ABI_VERSION 5

/* Maximum number of headers recorded per packet.  The reference recursion is unbounded
 * (fast.rs:53 VLAN stacks, :69 MPLS stacks, :89/:92/:104/:107 IP-in-IP, :168/:186/:219
 * tunnels back to Ethernet); chains longer than this report PKT_DEPTH_LIMIT. */
#define PKT_MAX_HDRS 16

/* Call-level return codes. */
#define PKT_SUCCESS            0
#define PKT_ERR_INVALID_ARG   -1
#define PKT_ERR_HIP           -2
#define PKT_ERR_NO_DEVICE     -3
#define PKT_ERR_UNSUPPORTED   -4
#define PKT_ERR_GATHER_ROWS   -5  /* pkt_mgpu_synchronize: a packet had more headers than the fixed gather rows */

/* Per-packet status (out->status). */
typedef enum pkt_status {
    PKT_OK          = 0, /* walk reached `accept` (fast.rs:223-227) */
    PKT_TRUNCATED   = 1, /* the reference would panic on a slice index (Q7) */
    PKT_DEPTH_LIMIT = 2  /* more than PKT_MAX_HDRS headers (build-only bound) */
} pkt_status_t;

/* Header type ids.  Names (pkt_hdr_name) are the reference's `Header::name()` strings,
 * i.e. the make_header! identifiers of headers.rs:529-827. */
typedef enum pkt_hdr_type {
    PKT_HDR_NONE               = 0,
    PKT_HDR_ETHER              = 1,  /* headers.rs:530-540  14 B */
    PKT_HDR_VLAN               = 2,  /* headers.rs:543-552   4 B */
    PKT_HDR_IPV4               = 3,  /* headers.rs:555-574  20 B */
    PKT_HDR_IPV6               = 4,  /* headers.rs:577-592  40 B */
    PKT_HDR_ICMP               = 5,  /* headers.rs:595-603   4 B */
    PKT_HDR_TCP                = 6,  /* headers.rs:606-622  20 B */
    PKT_HDR_UDP                = 7,  /* headers.rs:625-634   8 B */
    PKT_HDR_ARP                = 8,  /* headers.rs:637-653  28 B */
    PKT_HDR_VXLAN              = 9,  /* headers.rs:656-665   8 B */
    PKT_HDR_DOT3               = 10, /* headers.rs:668-678  14 B */
    PKT_HDR_LLC                = 11, /* headers.rs:681-689   3 B */
    PKT_HDR_SNAP               = 12, /* headers.rs:692-699   5 B */
    PKT_HDR_GRE                = 13, /* headers.rs:702-716   4 B */
    PKT_HDR_GRE_CHKSUM_OFFSET  = 14, /* headers.rs:719-726   4 B */
    PKT_HDR_GRE_SEQUENCE_NUM   = 15, /* headers.rs:729-735   4 B */
    PKT_HDR_GRE_KEY            = 16, /* headers.rs:738-744   4 B */
    PKT_HDR_ERSPAN2            = 17, /* headers.rs:747-760   8 B */
    PKT_HDR_ERSPAN3            = 18, /* headers.rs:763-782  12 B */
    PKT_HDR_ERSPAN_PLATFORM    = 19, /* headers.rs:785-792   8 B */
    PKT_HDR_STP                = 20, /* headers.rs:795-815  35 B (never produced by the walk) */
    PKT_HDR_MPLS               = 21, /* headers.rs:818-827   4 B */
    PKT_HDR_COUNT              = 22
} pkt_hdr_type_t;

/* Entry points: one per public function of parser::fast (fast.rs).  Parsing a batch with
 * entry E is `fast::parse_E(&pkt[..])` for every packet. */
typedef enum pkt_entry {
    PKT_ENTRY_PARSE     = 0,  /* fast::parse          fast.rs:5   (Dot3 if bytes 12..13 < 1500) */
    PKT_ENTRY_DOT3      = 1,  /* fast::parse_dot3     fast.rs:13  */
    PKT_ENTRY_LLC       = 2,  /* fast::parse_llc      fast.rs:19  */
    PKT_ENTRY_SNAP      = 3,  /* fast::parse_snap     fast.rs:29  */
    PKT_ENTRY_ETHERNET  = 4,  /* fast::parse_ethernet fast.rs:35  */
    PKT_ENTRY_VLAN      = 5,  /* fast::parse_vlan     fast.rs:49  */
    PKT_ENTRY_MPLS      = 6,  /* fast::parse_mpls     fast.rs:63  */
    PKT_ENTRY_MPLS_BOS  = 7,  /* fast::parse_mpls_bos fast.rs:74  */
    PKT_ENTRY_IPV4      = 8,  /* fast::parse_ipv4     fast.rs:84  */
    PKT_ENTRY_IPV6      = 9,  /* fast::parse_ipv6     fast.rs:99  */
    PKT_ENTRY_GRE       = 10, /* fast::parse_gre      fast.rs:114 */
    PKT_ENTRY_ERSPAN2   = 11, /* fast::parse_erspan2  fast.rs:166 */
    PKT_ENTRY_ERSPAN3   = 12, /* fast::parse_erspan3  fast.rs:172 */
    PKT_ENTRY_ARP       = 13, /* fast::parse_arp      fast.rs:193 */
    PKT_ENTRY_ICMP      = 14, /* fast::parse_icmp     fast.rs:198 */
    PKT_ENTRY_TCP       = 15, /* fast::parse_tcp      fast.rs:203 */
    PKT_ENTRY_UDP       = 16, /* fast::parse_udp      fast.rs:208 */
    PKT_ENTRY_VXLAN     = 17, /* fast::parse_vxlan    fast.rs:218 */
    PKT_ENTRY_COUNT     = 18
} pkt_entry_t;

/* A batch of packets resident in device memory (the caller owns every buffer).
 *  - Fixed-stride slab: offsets == NULL; packet i starts at slab + i*stride.  Its length is
 *    lens[i] when lens != NULL, else `stride`.
 *  - Indexed slab (e.g. a pcap file copied as-is): offsets[i] / lens[i] (both required)
 *    give each packet's byte range inside the slab.
 *  - A packet is the bytes of that range that lie inside [slab, slab + slab_len): its length
 *    is clamped to the slab end (a slot past the end is an empty packet) and to 65535 (the
 *    u16 offset/length columns).
 * The slab pointer must be 16-byte aligned; the kernels may read up to 15 bytes past a
 * packet's end but never past round_up(slab + slab_len, 16) (always inside a hipMalloc /
 * torch allocation, whose granularity is >= 256 B). */
typedef struct pkt_batch {
    const uint8_t  *slab;      /* device */
    uint64_t        slab_len;  /* bytes */
    const uint64_t *offsets;   /* device, [n] or NULL */
    const uint32_t *lens;      /* device, [n] or NULL */
    uint32_t        stride;    /* bytes between packets when offsets == NULL */
    uint32_t        reserved;
    uint64_t        n;         /* number of packets */
} pkt_batch_t;

/* Output columns (struct-of-arrays, device memory, caller-owned).  Every pointer may be
 * NULL: that column is then neither computed nor written (the reference's getters are
 * lazy, headers.rs:195-201 — a caller asks only for what it reads).
 *
 * Chain columns = PacketSlice (lib.rs:136-140, packet.rs:714-761):
 *   hdr_type/hdr_off are slot-major: slot j of packet i lives at [j*n + i]; slots
 *   j < n_hdrs[i] hold the chain; later slots are unspecified (not written for a parsed packet;
 *   a packet that fails may have written some before its failing header).  List order is the reference's `Vec::insert(0, ..)` order,
 *   i.e. wire order except GRE options (Q2: GRE, SeqNum, Key, ChksumOffset).
 *   hdr_off is the header's byte offset from the start of the packet (the Slice's
 *   pointer, headers.rs:187-192); payload_off/payload_len = PacketSlice::payload().
 *   On PKT_TRUNCATED / PKT_DEPTH_LIMIT no PacketSlice exists (the reference panics):
 *   n_hdrs = 0, hdr_mask = 0, payload_off = payload_len = 0 and every field column is 0.
 *
 * Field columns = the Slice getters of the FIRST header of that type in the list
 * (Packet's Index<&str> returns the first match, packet.rs:64-66 — Q11).  Values are the
 * reference's u64 getter results narrowed to the field's natural width; 0 when the packet
 * has no such header (check hdr_mask).  ipv6_src/dst are the 16 raw bytes that
 * `bytes(msb, lsb)` returns (headers.rs:202-211; the u64 getter is Q8).
 * ipv4_csum_calc = Packet::ipv4_checksum over that IPv4 header's 20 bytes (packet.rs:93-107). */
typedef struct pkt_out {
    /* chain */
    uint8_t  *status;          /* pkt_status_t */
    uint8_t  *n_hdrs;
    uint8_t  *hdr_type;        /* [PKT_MAX_HDRS][n] */
    uint16_t *hdr_off;         /* [PKT_MAX_HDRS][n] */
    uint16_t *payload_off;
    uint16_t *payload_len;
    uint32_t *hdr_mask;        /* bit t set iff a header of type t is in the list */
    /* Ether (headers.rs:530-540) */
    uint64_t *eth_dst;
    uint64_t *eth_src;
    uint16_t *eth_etype;
    /* Vlan (headers.rs:543-552) */
    uint8_t  *vlan_pcp;
    uint8_t  *vlan_cfi;
    uint16_t *vlan_vid;
    uint16_t *vlan_etype;
    /* IPv4 (headers.rs:555-574) */
    uint8_t  *ipv4_version;
    uint8_t  *ipv4_ihl;
    uint8_t  *ipv4_diffserv;
    uint16_t *ipv4_total_len;
    uint16_t *ipv4_identification;
    uint8_t  *ipv4_flags;
    uint16_t *ipv4_frag_startset;
    uint8_t  *ipv4_ttl;
    uint8_t  *ipv4_protocol;
    uint16_t *ipv4_header_checksum;
    uint32_t *ipv4_src;
    uint32_t *ipv4_dst;
    uint16_t *ipv4_csum_calc;  /* Packet::ipv4_checksum (packet.rs:93-107) */
    /* IPv6 (headers.rs:577-592) */
    uint8_t  *ipv6_version;
    uint8_t  *ipv6_traffic_class;
    uint32_t *ipv6_flow_label;
    uint16_t *ipv6_payload_len;
    uint8_t  *ipv6_next_hdr;
    uint8_t  *ipv6_hop_limit;
    uint8_t  *ipv6_src;        /* [n][16] */
    uint8_t  *ipv6_dst;        /* [n][16] */
    /* TCP (headers.rs:606-622) */
    uint16_t *tcp_src;
    uint16_t *tcp_dst;
    uint32_t *tcp_seq_no;
    uint32_t *tcp_ack_no;
    uint8_t  *tcp_data_startset;
    uint8_t  *tcp_res;
    uint8_t  *tcp_flags;
    uint16_t *tcp_window;
    uint16_t *tcp_checksum;
    uint16_t *tcp_urgent_ptr;
    /* UDP (headers.rs:625-634) */
    uint16_t *udp_src;
    uint16_t *udp_dst;
    uint16_t *udp_length;
    uint16_t *udp_checksum;
} pkt_out_t;

/* A field request for pkt_extract_fields: bits [start..=end] (MSB-first from the header's
 * first byte, the make_header! convention) of the `occurrence`-th header of `hdr_type`
 * in the chain (0 = first, as Packet's Index<&str>).  Any bit range is allowed, so a
 * user-defined make_header! field (lib.rs:81-103) is extracted the same way.  Widths
 * above 64 bits follow bit_range's release-build result (headers.rs:262, Q8). */
typedef struct pkt_field_spec {
    uint8_t  hdr_type;
    uint8_t  occurrence;
    uint16_t start;
    uint16_t end;
    uint16_t reserved;
} pkt_field_spec_t;

/* Chain columns produced by pkt_parse_batch, as input to pkt_extract_fields. */
typedef struct pkt_chain {
    const uint8_t  *n_hdrs;    /* [n] */
    const uint8_t  *hdr_type;  /* [PKT_MAX_HDRS][n] */
    const uint16_t *hdr_off;   /* [PKT_MAX_HDRS][n] */
} pkt_chain_t;

typedef struct pkt_ctx pkt_ctx_t;

/* ---- metadata (host only, no device needed) ---- */
int         pkt_abi_version(void);
/* sizeof the ABI structs, so a foreign binding (Rust/ctypes) can check its layout. */
size_t      pkt_sizeof_batch(void);
size_t      pkt_sizeof_out(void);
size_t      pkt_sizeof_field_spec(void);
/* Header::name() (headers.rs:218-220); NULL for an unknown id. */
const char *pkt_hdr_name(int hdr_type);
/* <Hdr>::size() (headers.rs:212-214); 0 for an unknown id. */
int         pkt_hdr_size(int hdr_type);
/* Field table of a header type (make_header! field list, headers.rs:529-827). */
int         pkt_hdr_field_count(int hdr_type);
int         pkt_hdr_field(int hdr_type, int idx, const char **name, uint16_t *start, uint16_t *end);
const char *pkt_status_name(int status);
const char *pkt_entry_name(int entry);   /* "parse", "parse_ethernet", ... */

/* ---- context ---- */
/* Binds to HIP device `device`.  No per-call allocation happens after creation. */
int         pkt_ctx_create(int device, pkt_ctx_t **ctx);
int         pkt_ctx_destroy(pkt_ctx_t *ctx);
const char *pkt_ctx_last_error(const pkt_ctx_t *ctx);
/* Tuning knob: packets staged per wave window (bytes of each packet copied to LDS).
 * 0 = automatic.  Values are rounded to a multiple of 16 and clamped to [16, 256]. */
int         pkt_ctx_set_window(pkt_ctx_t *ctx, uint32_t window_bytes);
/* Fast path (default on).  For entries PARSE and ETHERNET, a packet that starts on a 16-byte
 * boundary and whose first bytes read Ether / 0-2 x Vlan / IPv4 / UDP (dst != 4789) or TCP, long
 * enough for every header, has its chain decided by a few compares on the registers its bytes
 * were loaded into, so it skips the walk.  Results are identical to the walk's (the same fast.rs
 * path; the parity tests run with it forced on and off).  0 = off, 1 = on. */
int         pkt_ctx_set_fastpath(pkt_ctx_t *ctx, int enable);

/* Tuning knob: how packet bytes reach LDS.  0 = automatic (currently 1), 1 = per-lane windows of
 * pkt_ctx_set_window bytes (deeper headers read through L2), 2 = wave spans: each wave of 64
 * packets copies the contiguous byte range its packets occupy (up to 16 KiB; else per-lane
 * windows) into LDS by LDS-DMA and walks every header from there.  Results are identical in every
 * mode.  Any other value is PKT_ERR_INVALID_ARG. */
int         pkt_ctx_set_staging(pkt_ctx_t *ctx, int mode);

/* Tuning knob: walk schedule.  0 = automatic (lockstep for indexed batches, waterfall for fixed
 * stride), 1 = waterfall (each iteration advances the lanes in one state: one case per header
 * when a wave's packets share a layout), 2 = lockstep (every lane advances one header per
 * iteration: mixed chains in a wave cost their longest chain, not their number of distinct
 * states).  Results are identical in every mode. */
int         pkt_ctx_set_walk(pkt_ctx_t *ctx, int mode);

/* Tuning knob: bytes of file per copied piece of pkt_parse_pcap_host (pinned columns): 0 = the
 * default (16 MiB), else any value >= 4096; a capture is cut into at most 1024 pieces (larger pieces
 * for files past 1024 x the knob).  Results are identical for every value. */
int         pkt_ctx_set_host_piece(pkt_ctx_t *ctx, uint64_t bytes);

/* Tuning / test knob: 1 = the device pcap indexer composes its regions' states in 64-bit positions
 * and counts for every file (the form files of 4 GiB and more always take), 0 (default) = 32-bit ones
 * for files under 4 GiB.  Results are identical either way. */
int         pkt_ctx_set_pcap_scan64(pkt_ctx_t *ctx, int enable);

/* ---- the hot path ---- */
/* fast::parse_<entry> over every packet of `batch`, writing the requested columns of `out`.
 * Asynchronous on `stream`; returns after the launch.  `batch` and `out` may also point into pinned
 * host memory from pkt_host_alloc (mapped into the device): the kernel then reads and writes it
 * over the link directly — zero copy, still asynchronous (see pkt_parse_host for the blocking
 * form; pkt_ctx_set_staging(ctx, 2) suits host-resident indexed batches). */
int pkt_parse_batch(pkt_ctx_t *ctx, const pkt_batch_t *batch, int entry,
                    const pkt_out_t *out, void *stream);

/* `nbatch` independent batches: batches[k] -> outs[k], as nbatch pkt_parse_batch calls would write
 * them.  When the batches have the same n (<= 2^26), stride and layout (indexed or not, lens or not),
 * nbatch <= 16, and every batch's column pointers lie at one common byte distance from batch 0's (one
 * packed output buffer per batch, pkt_out_packed, qualifies), it is ONE launch whose grid covers every
 * batch's tiles, so the launch's ramp and drain are paid once; otherwise one launch per batch.
 * Asynchronous on `stream`. */
int pkt_parse_batches(pkt_ctx_t *ctx, const pkt_batch_t *batches, uint32_t nbatch, int entry,
                      const pkt_out_t *outs, void *stream);

/* ---- host-memory path ----
 * The reference's path starts and ends in host memory (a pcap file, a NIC ring).  One call moves
 * a HOST batch through the device: `batch` (slab, offsets, lens) and `out` (column pointers, the
 * pkt_out_t layout of pkt_parse_batch with slot columns strided by batch->n) are host memory.
 * The batch is cut into chunks of `chunk` packets (0 = 262144; 131072 with pinned columns)
 * pipelined over three streams of the ctx: the copy-in of chunk k+1 and the copy-out of chunk k-1
 * overlap the parse of chunk k.  Indexed chunks copy the byte span their records cover.  When the
 * slab, offsets, lens and every requested column are pinned memory from pkt_host_alloc, there are no
 * copies at all: one launch reads the slab and writes the columns over the link directly (zero copy;
 * `chunk` unused).  When only the columns are pinned, a chunk's columns go out by one kernel writing
 * them over the link in 16-byte chunks (else one copy per column).  Pageable buffers work, staged by
 * the runtime.  Blocks until every output is in host memory.  One host call at a time per ctx. */
int pkt_parse_host(pkt_ctx_t *ctx, const pkt_batch_t *batch, int entry, const pkt_out_t *out,
                   uint64_t chunk);
/* The capture path of tests/pcap.rs:7-37 end to end, host memory in and out: a pcap file in HOST
 * memory (`buf`, `len` bytes; pinned from pkt_host_alloc for the full link rate) is copied to the
 * device, indexed there (pkt_pcap_index_device: same records, count, cap behaviour and errors
 * as pkt_pcap_index) and parsed with `entry` (an indexed batch over the file in place); the requested
 * columns of `out` are HOST memory sized for `cap` records, slot columns strided by cap
 * ([PKT_MAX_HDRS][cap]).  Pinned columns are written by the parse kernel over the link directly; others
 * through the staged pipeline of pkt_parse_host.  offsets / lens (HOST, [cap], may be NULL) receive
 * the records' (data offset, incl_len).  *n_out = the record count (> cap: only the first cap are
 * parsed).  Blocking.  One host call at a time per ctx.
 * With pinned columns and a file longer than one piece (pkt_ctx_set_host_piece) the file is copied in
 * pieces and parsed while it arrives: once piece k has landed, the bytes it adds are indexed from the
 * previous piece's carry on the device (the first record it could not count and its record count —
 * pkt_pcap_stream_*'s steps; the file is indexed once, O(file), whatever the piece count; a record
 * running past a piece's end belongs to a later piece) and the records it completes are parsed, their
 * columns flowing out over the link while piece k + 1 flows in.  The last piece ends the file, indexed
 * with pkt_pcap_index's errors; on such an error the records of the earlier pieces may already be
 * written to `out`. */
int pkt_parse_pcap_host(pkt_ctx_t *ctx, const uint8_t *buf, uint64_t len, int entry, const pkt_out_t *out,
                        uint64_t *offsets, uint32_t *lens, uint64_t cap, uint64_t *n_out);
/* pkt_parse_pcap_host without the wait, for a stream of captures (cap <= 2^26, every column of `out`
 * in pinned memory from pkt_host_alloc, no index output): queues pkt_parse_pcap_host's pieces — the
 * copies in, the prefix indexes, the parses and the column exports — on the ctx's own streams and
 * returns; `buf` and `out` must stay untouched until pkt_parse_pcap_host_result, which waits for them
 * and gives the outcome as pkt_parse_pcap_host's (*n_out = the record count; on an error in the last
 * record the earlier pieces' records may be written).  One capture in flight per ctx (as
 * pkt_parse_pcap_async): two ctxs keep one capture's copy in flowing while the other's columns flow
 * out. */
int pkt_parse_pcap_host_async(pkt_ctx_t *ctx, const uint8_t *buf, uint64_t len, int entry, const pkt_out_t *out,
                              uint64_t cap);
int pkt_parse_pcap_host_result(pkt_ctx_t *ctx, uint64_t *n_out);
/* Pinned (page-locked) host memory for pkt_parse_host buffers. */
int pkt_host_alloc(pkt_ctx_t *ctx, uint64_t bytes, void **p);
int pkt_host_free(pkt_ctx_t *ctx, void *p);

/* Batched make_header! getter: for each spec s and packet i, values[s][i] = the field of
 * the chain's matching header (0 and found[s][i] = 0 when absent).  `values` and `found`
 * are HOST arrays of `nspec` DEVICE pointers, each to n elements; found may be NULL and
 * so may any found[s]. */
int pkt_extract_fields(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain,
                       const pkt_field_spec_t *specs, uint32_t nspec,
                       uint64_t *const *values, uint8_t *const *found, void *stream);

/* PacketSlice::to_vec / Packet::to_vec (packet.rs:733-740, 385-392) of every parsed packet:
 * its header slices in LIST order, then its payload, written to dst + dst_offsets[i]
 * (dst_offsets == NULL: the input batch's own layout, i*stride or offsets[i]).  With two or
 * more GRE options the list order differs from wire order (Q2), so the bytes are reordered
 * exactly as the reference's round trip reorders them.  `parsed` holds the chain columns of a
 * pkt_parse_batch over the same batch (status, n_hdrs, hdr_type, hdr_off, payload_off,
 * payload_len are read; the rest is ignored).  out_len[i] = bytes written (0 and nothing
 * written for a packet whose status is not PKT_OK); out_len may be NULL.
 * In the input's own layout (dst_offsets == NULL) of an indexed batch whose records share no
 * 16-byte chunk of the slab (e.g. a capture, with its record headers between the packets), a
 * destination chunk that holds a packet's first or last bytes is read, merged and written back
 * whole: the dst bytes between records inside such a chunk are rewritten with their own values,
 * not atomically — no other stream may write them while the call runs. */
int pkt_to_vec_batch(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_out_t *parsed,
                     uint8_t *dst, uint64_t dst_len, const uint64_t *dst_offsets,
                     uint32_t *out_len, void *stream);

/* Batched header rewrite, in place in the slab (the slab of `batch` must be writable):
 * `<Hdr>::set_<field>(v)` (headers.rs:340-344 -> set_bit_range 315-324) for each spec, in spec
 * order, on the spec's header of every packet's chain.  The low (end-start+1) bits of
 * values[s][i] go to bits [start..=end] (bits of a field wider than 64 above the value's 64
 * bits become 0, as set_bit_range shifts the u64 right once per bit).  Packets whose chain lacks
 * the header are untouched.  `values` is a HOST array of nspec DEVICE pointers ([n] each).
 * The packets of one batch must not overlap: a packet's bytes may be stored back whole (with
 * their values unchanged outside the fields set), never bytes outside [offset, offset + len). */
int pkt_set_fields(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain,
                   const pkt_field_spec_t *specs, uint32_t nspec, const uint64_t *const *values,
                   void *stream);

/* pkt_set_fields followed, in the same launch, by pkt_ipv4_update_checksum of the
 * `ipv4_occurrence`-th IPv4 header (< 0: no checksum refresh; nspec may then be 0 for a refresh
 * alone), as one pass over each packet's bytes.  The reference's update+clone loop
 * (tests/lib.rs:778-787) is setters only (set_etype; ipv4_occurrence < 0); the checksum refresh is
 * what the create_* builders do after setting IPv4 fields (utils.rs:233-236). */
int pkt_set_fields_csum(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain,
                        const pkt_field_spec_t *specs, uint32_t nspec, const uint64_t *const *values,
                        int32_t ipv4_occurrence, void *stream);

/* `ipv4.set_header_checksum(Packet::ipv4_checksum(ipv4.to_vec()))` (utils.rs:233-236;
 * packet.rs:93-107 with the Q1 fold) on the `occurrence`-th IPv4 header of every packet, in
 * place.  Packets without that header are untouched. */
int pkt_ipv4_update_checksum(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain,
                             uint32_t occurrence, void *stream);

/* Batched packet generation, clone step (`pkt.clone().to_vec()` of tests/lib.rs:770-776 for n
 * copies): writes the `len`-byte DEVICE packet `src` n times, at dst + i*stride, and zero-fills
 * the rest of each stride slot.  Follow with pkt_parse_batch (chain), pkt_set_fields and
 * pkt_ipv4_update_checksum to vary fields per packet (the update+clone workload, 778-787). */
int pkt_broadcast(pkt_ctx_t *ctx, const uint8_t *src, uint32_t len, uint64_t n, uint32_t stride,
                  uint8_t *dst, void *stream);

/* ---- batched packet generation: the pktgen loop (tests/lib.rs:756-788) ----
 * The reference builds a packet with a `utils::create_*` builder (utils.rs:7-876), clones it,
 * updates fields through the setters (headers.rs:340-344 -> set_bit_range 315-324) and serialises
 * it with to_vec, once per packet.  Here the builder's bytes are a TEMPLATE: pkt_gen_create parses
 * it once on the device (entry as for pkt_parse_batch) and places every generator field by its
 * (header, occurrence, bits) in the template's chain (Index<&str> semantics, packet.rs:64-66);
 * pkt_gen_run then writes n packets at dst + i*stride in one pass (the template, every field set
 * to its value for that packet, the listed IPv4 checksums refreshed with Packet::ipv4_checksum
 * (packet.rs:93-107) as the builders do, utils.rs:233-236; the rest of each stride slot zeroed).
 * A field gets the value's low (end-start+1) <= 64 bits, as set_bit_range does.  Packet i of a
 * run has global index g = first + i; the value of a field is
 *   PKT_GEN_VALUES  values[f][i]                   (a DEVICE array per field, given to pkt_gen_run)
 *   PKT_GEN_INC     base + step * (g % count)      (count 0: base + step * g; the reference's
 *                                                   update loop is base 0, step 1, count 0xFFFF)
 *   PKT_GEN_RANDOM  splitmix64(base + g)           (z = x + 0x9E3779B97F4A7C15;
 *                   z = (z ^ z>>30) * 0xBF58476D1CE4E5B9; z = (z ^ z>>27) * 0x94D049BB133111EB;
 *                   z ^ z>>31) — base is the seed.
 * Fields apply in order (a later field wins where two overlap); checksum refreshes come last. */
typedef enum pkt_gen_kind {
    PKT_GEN_VALUES = 0,
    PKT_GEN_INC    = 1,
    PKT_GEN_RANDOM = 2
} pkt_gen_kind_t;
typedef struct pkt_gen_field {
    pkt_field_spec_t field;  /* header type, occurrence, bits [start..=end], width 1..64 */
    uint32_t kind;           /* pkt_gen_kind_t */
    uint32_t reserved;
    uint64_t base;
    uint64_t step;
    uint64_t count;
} pkt_gen_field_t;
typedef struct pkt_gen pkt_gen_t;
size_t pkt_sizeof_gen_field(void);
/* `tpl` is HOST memory (len bytes, <= 65535); at most 32 fields.  ipv4_csum_mask bit k refreshes
 * the checksum of the template's k-th IPv4 header (at most 8).  Blocking (one template parse).
 * Fails with PKT_ERR_INVALID_ARG if the template does not parse to PKT_OK or lacks a named header. */
int pkt_gen_create(pkt_ctx_t *ctx, const uint8_t *tpl, uint32_t len, int entry,
                   const pkt_gen_field_t *fields, uint32_t nfields, uint32_t ipv4_csum_mask,
                   pkt_gen_t **gen);
/* Writes packets first .. first+n-1 to `dst` (device, 16-byte aligned, n*stride bytes; stride a
 * multiple of 16 and >= the template length).  `values` is a HOST array with one DEVICE pointer
 * ([n] uint64) per field, used by PKT_GEN_VALUES fields (may be NULL when there are none).
 * Asynchronous on `stream`. */
int pkt_gen_run(pkt_gen_t *gen, uint64_t first, uint64_t n, uint32_t stride,
                const uint64_t *const *values, uint8_t *dst, void *stream);
int pkt_gen_destroy(pkt_gen_t *gen);

/* Packet::ipv4_checksum (packet.rs:93-107) over n headers of 20 bytes at a fixed stride
 * in device memory: out[i] = checksum(hdrs + i*stride). */
int pkt_ipv4_checksum_batch(pkt_ctx_t *ctx, const uint8_t *hdrs, uint32_t stride, uint64_t n,
                            uint16_t *out, void *stream);

/* ---- host-side helpers ---- */
/* Index a pcap byte buffer in the tests/pcap.rs:7-37 format (LE magic d4 c3 b2 a1, 24-byte
 * global header, 16-byte record headers).  Writes up to `cap` record (data offset, incl_len)
 * pairs and the record count to *n_out (which can exceed cap: call again with a larger cap).
 * Returns PKT_ERR_INVALID_ARG on a bad magic or a record running past `len`. */
int pkt_pcap_index(const uint8_t *buf, uint64_t len, uint64_t *offsets, uint32_t *lens,
                   uint64_t cap, uint64_t *n_out);

/* pkt_pcap_index for a pcap file resident in DEVICE memory (`buf` 16-byte aligned, readable up to
 * round_up(len, 16)): same records, count, cap behaviour and errors, with `offsets` / `lens` in
 * device memory — ready for an indexed pkt_batch_t over the same buffer.  The sequential record
 * chain is recovered per 4 KiB region by a speculative guess plus exact fix-up rounds
 * (pktgpu_pcap.hip).  Blocking: returns once *n_out is known (work is ordered on `stream`). */
int pkt_pcap_index_device(pkt_ctx_t *ctx, const uint8_t *buf, uint64_t len, uint64_t *offsets,
                          uint32_t *lens, uint64_t cap, uint64_t *n_out, void *stream);
/* pkt_pcap_index_device with the index's three kernels timed by HIP events recorded between
 * them on `stream` (measurement): kernel_ms[0..2] = guess, scan, emit (emit ~0 when cap == 0). */
int pkt_pcap_index_device_timed(pkt_ctx_t *ctx, const uint8_t *buf, uint64_t len, uint64_t *offsets,
                                uint32_t *lens, uint64_t cap, uint64_t *n_out, void *stream,
                                float *kernel_ms);

/* The capture path of tests/pcap.rs:7-37 on a pcap file already in DEVICE memory, in one call:
 * pkt_pcap_index_device into offsets / lens (device, [cap], cap >= 1), then fast::parse_<entry> of
 * every record (an indexed batch over `buf` in place) into `out` (device columns sized for cap
 * records, slot columns strided by cap).  The parse takes the record count from the device (its
 * blocks past it exit), so the host waits once, for both; *n_out = the record count (> cap: only
 * the first cap records are indexed and parsed).  Errors as pkt_pcap_index_device (nothing is
 * parsed then).  Blocking. */
int pkt_parse_pcap(pkt_ctx_t *ctx, const uint8_t *buf, uint64_t len, int entry, const pkt_out_t *out,
                   uint64_t *offsets, uint32_t *lens, uint64_t cap, uint64_t *n_out, void *stream);

/* pkt_parse_pcap without the host wait, for a stream of captures: queues the index kernels and the
 * counted parse on `stream` (cap <= 2^26) and returns.  pkt_parse_pcap_result waits for them and
 * gives the outcome (the record count, or the errors of pkt_pcap_index_device; after an error
 * nothing was parsed).  The ctx's index scratch belongs to the queued capture until its result is
 * taken: one capture in flight per ctx (two in flight = two ctxs, e.g. one per stream); another
 * index call on the ctx before that fails with PKT_ERR_INVALID_ARG. */
int pkt_parse_pcap_async(pkt_ctx_t *ctx, const uint8_t *buf, uint64_t len, int entry, const pkt_out_t *out,
                         uint64_t *offsets, uint32_t *lens, uint64_t cap, void *stream);
int pkt_parse_pcap_result(pkt_ctx_t *ctx, uint64_t *n_out);

/* ---- writing a capture ----
 * tests/pcap.rs:7-37 as a batch operation: the selected packets of `batch`, in batch order, as one
 * capture in dst: the 24-byte global header of pcap.rs:20-23, then per packet a 16-byte record header
 * (tv_sec, tv_usec, incl_len, orig_len, little-endian u32, pcap.rs:27-32) and incl_len packet bytes.
 *  - batch: any pkt_batch_t, fixed-stride or indexed, under its usual slab rules (the slab is only read,
 *    so indexed offsets need not be ordered and may overlap).  len_i = the batch's packet length, clamped
 *    to the slab end and to 65535.
 *  - select: device [n] or NULL (every packet); packet i is written iff select[i] != 0.
 *  - snaplen: 0 = no truncation, else incl_len = min(len_i, snaplen); orig_len = len_i always (with
 *    snaplen 0 the reference's `plen, plen`).  The global header is always the reference's 24 bytes
 *    (file snaplen 0xffff).
 *  - ts_sec / ts_usec: device [n] arrays indexed by the SOURCE packet i, each NULL for the constant
 *    tv_sec / tv_usec (the reference stamps one time on the whole file).
 *  - dst: device memory, 16-byte aligned, dst_len bytes of capacity.  total = 24 + sum over the selected
 *    packets of (16 + incl_len), as uint64.  Bytes [0, total) are written, each once and fully defined;
 *    nothing at or past total is written and no byte of dst is read.  If total > dst_len the call
 *    returns PKT_ERR_INVALID_ARG with *bytes_out = total and *n_out = the selected count (the capacity
 *    to retry with); dst's contents are then unspecified, but nothing outside [0, dst_len) is written.
 *    (The decision is taken on the device, where total is known: the writing kernels read it and exit.)
 *  - rec_offsets / rec_lens / src_index: device arrays sized for n, each may be NULL.  For the k-th
 *    written record: its data offset in dst, its incl_len (what pkt_pcap_index returns on the result, so
 *    {dst, total, rec_offsets, rec_lens, *n_out} is an indexed pkt_batch_t) and its source packet index.
 *    Entries at index >= *n_out are not written.
 *  - n may be 0 and the selection may be empty: the 24-byte header alone.  n >= 2^32 is
 *    PKT_ERR_INVALID_ARG.
 * pkt_pcap_write is blocking: one host wait, for the two totals (work is ordered on `stream`).
 * pkt_pcap_write_async queues the same work and returns; the totals go to pinned words of the ctx and
 * pkt_pcap_write_result waits for them and gives the outcome as pkt_pcap_write's.  One write in flight
 * per ctx: another write on the ctx before the result is taken fails with PKT_ERR_INVALID_ARG.
 * pkt_pcap_write_host is the same operation on HOST pointers (batch, select, ts_*, dst and the three
 * outputs) and needs no device or ctx, like pkt_pcap_index. */
int pkt_pcap_write(pkt_ctx_t *ctx, const pkt_batch_t *batch, const uint8_t *select, uint32_t snaplen,
                   uint32_t tv_sec, uint32_t tv_usec, const uint32_t *ts_sec, const uint32_t *ts_usec,
                   uint8_t *dst, uint64_t dst_len, uint64_t *rec_offsets, uint32_t *rec_lens,
                   uint32_t *src_index, uint64_t *bytes_out, uint64_t *n_out, void *stream);
int pkt_pcap_write_async(pkt_ctx_t *ctx, const pkt_batch_t *batch, const uint8_t *select, uint32_t snaplen,
                         uint32_t tv_sec, uint32_t tv_usec, const uint32_t *ts_sec, const uint32_t *ts_usec,
                         uint8_t *dst, uint64_t dst_len, uint64_t *rec_offsets, uint32_t *rec_lens,
                         uint32_t *src_index, void *stream);
int pkt_pcap_write_result(pkt_ctx_t *ctx, uint64_t *bytes_out, uint64_t *n_out);
int pkt_pcap_write_host(const pkt_batch_t *batch, const uint8_t *select, uint32_t snaplen, uint32_t tv_sec,
                        uint32_t tv_usec, const uint32_t *ts_sec, const uint32_t *ts_usec, uint8_t *dst,
                        uint64_t dst_len, uint64_t *rec_offsets, uint32_t *rec_lens, uint32_t *src_index,
                        uint64_t *bytes_out, uint64_t *n_out);

/* ---- comparing two batches ----
 * Packet::compare / compare_with_slice (packet.rs:326-358) as a batch operation: packet i of `a`
 * against packet i of `b`.  la, lb = the two packets' lengths under the pkt_batch_t rules (clamped to
 * the slab end and to 65535), m = min(la, lb).
 *  - byte j < m MATCHES iff ((a[j] ^ b[j]) & ~ign[j]) == 0 (ign = the packet's ignore mask, below).
 *  - matching[i]   = the number of matching j in [0, m): the reference's zip/filter/count
 *    (packet.rs:347), a count of equal positions and not a prefix length.
 *  - first_diff[i] = the smallest non-matching j, or m when there is none (an extension: the reference
 *    prints only the count).
 *  - result[i]     = PKT_CMP_LEN if la != lb (the reference's first test, packet.rs:342: decided
 *    before any byte, never changed by the ignores), else PKT_CMP_BYTES if matching != la, else
 *    PKT_CMP_EQUAL.  For PKT_CMP_LEN, matching and first_diff still cover the common m bytes (a
 *    snaplen-cut capture shows matching == m).
 *  - ignore: up to 16 specs, resolved per packet against chain_a, the chain columns of a parse of
 *    `a`.  Spec (hdr_type, occurrence, start, end) ignores bits [start..=end] (MSB-first from the
 *    header's first byte, as pkt_extract_fields; any width end >= start) of that header of packet i's
 *    own chain, in a[i] and at the same bit positions in b[i].  Bits at or past 8 m are dropped; a
 *    packet whose chain lacks the header (n_hdrs == 0 included) ignores nothing for that spec; specs
 *    may overlap.  nignore == 0 needs no chain.
 *  - a, b: any two pkt_batch_t, fixed-stride or indexed in any mix, under the usual slab rules; both
 *    are only read and may overlap or be the same buffer.  result / matching / first_diff: device
 *    [n], each may be NULL.  summary (host) may be NULL.
 *  - PKT_ERR_INVALID_ARG: a->n != b->n, n >= 2^32, nignore > 16, nignore > 0 with a NULL chain, a spec
 *    with end < start.  n == 0 succeeds with an all-zero summary (first_bad = 0).
 * The reference's compare is self.to_vec() against the other's bytes; here BOTH sides are the raw
 * batch bytes.  A caller who wants the to_vec order (a packet with two or more GRE options, Q2) runs
 * pkt_to_vec_batch first and compares its output.
 * pkt_compare_batch is blocking: one host wait, for the summary (work is ordered on `stream`).
 * pkt_compare_batch_async queues the same work and returns; the summary goes to pinned words of the
 * ctx and pkt_compare_result waits for them.  One compare in flight per ctx: another compare on the
 * ctx before the result is taken fails with PKT_ERR_INVALID_ARG.  pkt_compare_host is the same
 * operation on HOST pointers and needs no device or ctx. */
typedef enum pkt_cmp { PKT_CMP_EQUAL = 0, PKT_CMP_LEN = 1, PKT_CMP_BYTES = 2 } pkt_cmp_t;
typedef struct pkt_cmp_summary {
    uint64_t n_equal;    /* packets per result; the three sum to n */
    uint64_t n_len;
    uint64_t n_bytes;
    uint64_t first_bad;  /* lowest i with result != PKT_CMP_EQUAL, n if none */
} pkt_cmp_summary_t;
size_t pkt_sizeof_cmp_summary(void);
int pkt_compare_batch(pkt_ctx_t *ctx, const pkt_batch_t *a, const pkt_batch_t *b, const pkt_chain_t *chain_a,
                      const pkt_field_spec_t *ignore, uint32_t nignore, uint8_t *result, uint32_t *matching,
                      uint32_t *first_diff, pkt_cmp_summary_t *summary, void *stream);
int pkt_compare_batch_async(pkt_ctx_t *ctx, const pkt_batch_t *a, const pkt_batch_t *b,
                            const pkt_chain_t *chain_a, const pkt_field_spec_t *ignore, uint32_t nignore,
                            uint8_t *result, uint32_t *matching, uint32_t *first_diff, void *stream);
int pkt_compare_result(pkt_ctx_t *ctx, pkt_cmp_summary_t *summary);
int pkt_compare_host(const pkt_batch_t *a, const pkt_batch_t *b, const pkt_chain_t *chain_a,
                     const pkt_field_spec_t *ignore, uint32_t nignore, uint8_t *result, uint32_t *matching,
                     uint32_t *first_diff, pkt_cmp_summary_t *summary);

/* ---- editing a batch's header lists ----
 * Packet::push / insert / pop / remove (packet.rs:117-164), `Add` (75-84) and the to_vec that
 * serialises the result (385-392) as a batch operation.  For packet i of a parsed batch the
 * reference's Packet is the list L whose entry j is the packet's bytes [hdr_off[j], hdr_off[j] +
 * pkt_hdr_size(hdr_type[j])), in list order (Q2 order for GRE options), with the payload
 * [payload_off, payload_off + payload_len).  The `nops` <= 8 ops of the program, the same for every
 * packet, are applied to L in order; then to_vec is written: the list's slices back to back, then
 * the payload.
 *  - PKT_EDIT_POP         Packet::pop: drops the last entry; no-op on an empty list (143-147).
 *  - PKT_EDIT_REMOVE_AT   Packet::remove(index): no-op when index >= len (160-164).
 *  - PKT_EDIT_REMOVE_HDR  (extension) removes the `index`-th entry of `hdr_type` in the CURRENT list,
 *                         counted as Index<&str> counts (64-66); no-op when the list has none.
 *  - PKT_EDIT_INSERT      a new header of hdr_type whose pkt_hdr_size(hdr_type) bytes are
 *                         hdr_data[data_off ..]: index 0 = Packet::insert (129-131), index PKT_EDIT_END
 *                         = Packet::push (117-119; `Add` is push header by header), any other index =
 *                         Vec::insert(min(index, len)) (extension).
 *  - batch / parsed: as pkt_to_vec_batch: `parsed` holds the chain columns of a parse of the same batch
 *    (status, n_hdrs, hdr_type, hdr_off, payload_off, payload_len are required and read; hdr_mask and the
 *    field columns are ignored).  n_hdrs is taken as min(n_hdrs, PKT_MAX_HDRS) and every slice is clamped
 *    to the packet's [0, len) under the pkt_batch_t rules: whatever the columns hold, no byte outside
 *    the packet is read and none outside its slot is written (columns that are not a parse of the batch
 *    give unspecified output bytes, never other accesses).
 *  - hdr_data: HOST memory, hdr_data_len <= 320 bytes, captured at the call (the caller may free it on
 *    return).  Every INSERT names pkt_hdr_size(hdr_type) bytes inside it, hdr_type in 1..21.
 *  - select: device [n] or NULL; a packet with select[i] == 0 is written with no op applied (plain
 *    to_vec) and still counts as PKT_EDIT_OK.
 *  - dst: device, 16-byte aligned, dst_len bytes.  Packet i owns [o_i, o_i + room_i), o_i = dst_offsets ?
 *    dst_offsets[i] : i * slot (any alignment), room_i = min(slot, dst_len - o_i), 0 when o_i >= dst_len.
 *    The caller keeps the slots disjoint from each other and from the source slab.  Exactly the bytes
 *    [o_i, o_i + out_len[i]) are written, each once; no other byte of dst is written, not even with
 *    its own value, and dst is never read (a packet's first and last partial 16-byte chunks go out in
 *    narrower stores, not as a read-merge-write).
 *  - edit_status[i] (device [n], may be NULL): PKT_EDIT_OK = written; PKT_EDIT_SKIPPED = the source
 *    status is not PKT_OK (the reference panicked: there is no Packet); PKT_EDIT_DEPTH = the list
 *    exceeded PKT_MAX_HDRS right after some INSERT (even if a later op would shrink it);
 *    PKT_EDIT_NO_ROOM = the new length exceeds room_i or 65535.  For the three others nothing is
 *    written and out_len[i] = 0.  out_len (device [n]) may be NULL.
 *  - out_chain (may be NULL): a pkt_out_t of which only the seven chain columns are honoured, each of
 *    which may be NULL.  It receives the edited Packet's own list, not a re-parse of its bytes: n_hdrs,
 *    slot-major hdr_type / hdr_off for slots < n_hdrs (entry k's offset = the sum of the sizes before
 *    it; later slots are not written, as pkt_parse_batch leaves them), payload_off, payload_len,
 *    hdr_mask, and status = PKT_OK.  For the other results status = the source status (SKIPPED),
 *    PKT_DEPTH_LIMIT (DEPTH) or PKT_TRUNCATED (NO_ROOM) and n_hdrs = payload_off = payload_len = hdr_mask
 *    = 0: pkt_parse_batch's contract for a failed packet.  So {dst, o_i, out_len} with out_chain feeds
 *    pkt_set_fields_csum, pkt_extract_fields, pkt_compare_batch's ignores, pkt_pcap_write and
 *    pkt_to_vec_batch with no second parse.
 *  - The per-packet encap flow: INSERT the constant outer headers (e.g. Vxlan, UDP, IPv4, Ether, each at
 *    index 0), then pkt_set_fields_csum on {dst, out_len} with out_chain: IPv4 total_len = out_len - 14
 *    and UDP length = out_len - 34 as per-packet values, ipv4_occurrence = 0 for the checksum.
 *  - PKT_ERR_INVALID_ARG, before any launch: nops > 8, an unknown kind, an INSERT with a bad type or
 *    bytes running past hdr_data_len, hdr_data_len > 320, a NULL required pointer, n >= 2^32, slot == 0.
 *    n == 0 succeeds and does nothing.
 * Asynchronous on `stream`, like pkt_to_vec_batch: no host wait and no summary.  pkt_edit_host is the
 * same operation on HOST pointers (batch, parsed, select, dst and the outputs) and needs no device or
 * ctx. */
#define PKT_EDIT_END 0xFF
typedef enum pkt_edit_kind {
    PKT_EDIT_POP        = 0,
    PKT_EDIT_REMOVE_AT  = 1,
    PKT_EDIT_REMOVE_HDR = 2,
    PKT_EDIT_INSERT     = 3
} pkt_edit_kind_t;
typedef enum pkt_edit_status {
    PKT_EDIT_OK      = 0,
    PKT_EDIT_SKIPPED = 1,
    PKT_EDIT_DEPTH   = 2,
    PKT_EDIT_NO_ROOM = 3
} pkt_edit_status_t;
typedef struct pkt_edit_op {
    uint8_t  kind;      /* pkt_edit_kind_t */
    uint8_t  hdr_type;  /* REMOVE_HDR, INSERT */
    uint8_t  index;     /* REMOVE_AT: position; REMOVE_HDR: occurrence; INSERT: position or PKT_EDIT_END */
    uint8_t  reserved;
    uint32_t data_off;  /* INSERT: the header's first byte in hdr_data */
} pkt_edit_op_t;
size_t pkt_sizeof_edit_op(void);
int pkt_edit_batch(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_out_t *parsed, const pkt_edit_op_t *ops,
                   uint32_t nops, const uint8_t *hdr_data, uint32_t hdr_data_len, const uint8_t *select,
                   uint8_t *dst, uint64_t dst_len, const uint64_t *dst_offsets, uint32_t slot,
                   uint32_t *out_len, uint8_t *edit_status, const pkt_out_t *out_chain, void *stream);
int pkt_edit_host(const pkt_batch_t *batch, const pkt_out_t *parsed, const pkt_edit_op_t *ops, uint32_t nops,
                  const uint8_t *hdr_data, uint32_t hdr_data_len, const uint8_t *select, uint8_t *dst,
                  uint64_t dst_len, const uint64_t *dst_offsets, uint32_t slot, uint32_t *out_len,
                  uint8_t *edit_status, const pkt_out_t *out_chain);

/* ---- L4 checksums of a batch ----
 * The TCP / UDP / ICMP checksum of every packet, verified and optionally stored: the sibling of
 * pkt_ipv4_checksum_batch that the reference announces and never builds (`_tcp_checksum`, `_udp_checksum`:
 * utils.rs:156, 213, 261, 439, 480, 520, 565 take the flag and ignore it; the v6 builders store a literal
 * 0xffff, utils.rs:461, 589).  It is the one rewrite-side operation that reads every payload byte.
 *  - batch / chain: any pkt_batch_t under its usual slab rules, with the chain columns of a parse of it, or
 *    pkt_edit_batch's out_chain.  n_hdrs is taken as min(n_hdrs, PKT_MAX_HDRS).
 *  - The L4 header is the `which`-th list entry whose type is TCP, UDP or ICMP, the three counted together
 *    in list order from 0; PKT_L4_LAST takes the last such entry.  (A VXLAN packet has its outer UDP at 0
 *    and its inner TCP at 1, which is also LAST.)  `which` in 16..0xFE is PKT_ERR_INVALID_ARG.  A chain
 *    without that entry (n_hdrs == 0 included) is PKT_L4_ABSENT.
 *  - The IP header is the list entry immediately before the L4 header, where the walk always puts it
 *    (fast.rs:84-113).  Any other type there, or an L4 header at slot 0, is PKT_L4_NO_IP.
 *  - The segment is the packet-relative span [s, e).  s = the chain's hdr_off of the L4 header (the
 *    reference places L4 at IP + 20 whatever ihl says; this call follows the chain).  e = hdr_off(IP) +
 *    total_len for IPv4, hdr_off(IP) + 40 + payload_len for IPv6: the IP header's length, not the packet's
 *    end (a 60-byte padded frame carries bytes past e that are not summed).  PKT_L4_SPAN: the IP header's
 *    20 / 40 bytes do not lie inside the packet (its length under the pkt_batch_t clamp rules), e exceeds
 *    that length, or e < s + pkt_hdr_size(L4 type).  PKT_L4_FRAGMENT: IPv4 with (bytes 6..7 & 0x3FFF) != 0,
 *    decided after the IP header is known to be inside the packet and before e is examined.
 *  - The sum is RFC 1071's: the one's-complement sum of the 16-bit big-endian words of the pseudo-header
 *    and the segment, the segment's checksum field (TCP bytes 16-17, UDP 6-7, ICMP 2-3) taken as zero and
 *    an odd last byte padded with zero.  It is the correct end-around-carry fold, not Packet::ipv4_checksum's
 *    (Q1): this value has to interoperate with real stacks and the reference defines none.  IPv4
 *    pseudo-header: src, dst, 0, proto, e - s as u16.  IPv6: src, dst, e - s as u32, 0, 0, 0, next.  proto /
 *    next comes from the L4 type: TCP 6, UDP 17, ICMP under IPv6 58; ICMP under IPv4 has no pseudo-header.
 *    calc = ~fold(sum); for UDP a calc of 0 becomes 0xFFFF.
 *  - calc / stored / l4_status: device [n], each may be NULL.  calc = the value that belongs in the field,
 *    stored = the field as read, before any update.  l4_status: UDP over IPv4 with stored == 0 is
 *    PKT_L4_UNCHECKED, UDP over IPv6 with stored == 0 is PKT_L4_BAD, otherwise PKT_L4_OK or PKT_L4_BAD by
 *    the rule at the enum.  For ABSENT, NO_IP, SPAN and FRAGMENT calc = stored = 0 and the packet is never
 *    written.
 *  - PKT_L4_UPDATE: the slab must be writable and the packets must not overlap, as for pkt_set_fields.  For
 *    a packet with status OK, BAD or UNCHECKED exactly the two checksum bytes are stored, big-endian (with
 *    PKT_L4_KEEP_ZERO_UDP an UNCHECKED packet is not stored); no other byte of the slab is written, not
 *    even with its own value.  The status still describes the field as it was read.
 *  - PKT_ERR_INVALID_ARG, before any launch: the usual batch and slab refusals, a NULL chain (with n > 0, a
 *    NULL chain column), n >= 2^32, unknown flag bits, KEEP_ZERO_UDP without UPDATE, a bad `which`.  n == 0
 *    succeeds and launches nothing.
 * Asynchronous on `stream`, like pkt_edit_batch: no host wait, no summary and no ctx state.
 * pkt_l4_checksum_host is the same operation on HOST pointers and needs no device or ctx.
 * Out of scope: incremental (RFC 1624) updates after a field rewrite: pkt_fwd_batch (the ttl) and pkt_nat_batch (an
 * address and a port, with the TCP / UDP / ICMP checksum; no payload byte is read) are the calls that make them. */
typedef enum pkt_l4_status {
    PKT_L4_OK        = 0, /* stored == calc (or stored 0xFFFF with calc 0: the two encodings of zero) */
    PKT_L4_BAD       = 1,
    PKT_L4_UNCHECKED = 2, /* UDP over IPv4 with a stored checksum of 0 (RFC 768: none sent) */
    PKT_L4_ABSENT    = 3, /* the chain has no such L4 header (n_hdrs == 0 included) */
    PKT_L4_NO_IP     = 4, /* the list entry just before the L4 header is neither IPv4 nor IPv6 */
    PKT_L4_SPAN      = 5, /* the IP length puts the segment's end past the packet, or before the L4 header's end */
    PKT_L4_FRAGMENT  = 6  /* IPv4 with MF set or a non-zero fragment offset */
} pkt_l4_status_t;
#define PKT_L4_LAST            0xFFu  /* which: the last TCP/UDP/ICMP header of the list */
#define PKT_L4_UPDATE          1u     /* flags: store calc into the packet */
#define PKT_L4_KEEP_ZERO_UDP   2u     /* flags: with UPDATE, leave an UNCHECKED packet's 0 alone */
int pkt_l4_checksum_batch(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain,
                          uint32_t which, uint32_t flags, uint16_t *calc, uint16_t *stored,
                          uint8_t *l4_status, void *stream);
int pkt_l4_checksum_host(const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which,
                         uint32_t flags, uint16_t *calc, uint16_t *stored, uint8_t *l4_status);

/* ---- flow keys of a batch, and a flow table that accumulates them ----
 * Which flow each packet belongs to, and how many packets and bytes each flow has carried.  The reference
 * defines nothing here (it is a packet library, not a dataplane), so this header fixes the semantics; the one
 * outside standard, the Toeplitz hash NICs compute for RSS, is matched bit for bit.  Two pieces that meet at
 * caller-owned arrays: a stateless key kernel over a parsed batch, and a hash table over keys that never sees
 * packets or chains.
 *
 * pkt_flow_key_batch
 *  - batch / chain: any pkt_batch_t under its usual slab rules, with the chain columns of a parse of it, of a
 *    stream's columns over pkt_pcap_stream_batch, or pkt_edit_batch's out_chain.  n_hdrs is taken as
 *    min(n_hdrs, PKT_MAX_HDRS).  Whatever the columns hold, no byte outside the packet is used.
 *  - The IP header is the `which_ip`-th list entry of type IPv4 or IPv6, the two counted together from 0;
 *    PKT_FLOW_LAST takes the last such entry (a VXLAN packet's outer IP is 0, its inner IP is 1 and LAST).
 *    `which_ip` in 16..0xFE is PKT_ERR_INVALID_ARG.  No such entry (n_hdrs == 0 included): PKT_FLOW_NO_IP.
 *    The entry's 20 / 40 bytes not inside the packet (its length under the pkt_batch_t clamp): PKT_FLOW_SPAN.
 *  - Ports are taken iff the list entry right after the IP entry is TCP or UDP, PKT_FLOW_NO_PORTS is not
 *    set and, for IPv4, (bytes 6..7 & 0x3FFF) == 0 (pkt_l4_checksum_batch's fragment test: every fragment
 *    of a datagram gets one key).  Ports that are taken are the 4 bytes at that entry's hdr_off; if they do
 *    not lie inside the packet the status is PKT_FLOW_SPAN.  Not taken: sport = dport = 0.  proto is always
 *    the IP header's own byte, so a GRE or ICMP packet keys on addresses and protocol alone.
 *  - PKT_FLOW_SYMMETRIC: if the byte string src[16] | sport (big-endian) compares greater than dst[16] |
 *    dport, the two ends are swapped and dir = 1; otherwise, and always without the flag, dir = 0.  Both
 *    directions of a connection then give the same key, hash and rss.
 *  - hash: h = seed; for each of the five little-endian u64 words w of the key as it lies in memory,
 *    h = splitmix64(h ^ w) (splitmix64: the function spelled out at PKT_GEN_RANDOM).
 *  - rss (computed iff rss != NULL): the Toeplitz hash of Microsoft RSS with the 40-byte `rss_key` (HOST
 *    memory, captured at the call; may be NULL iff rss == NULL) over the key after any swap: src | dst (4 or
 *    16 wire bytes each), then sport | dport (big-endian) iff ports were taken: 8, 12, 32 or 36 bytes.  For
 *    each set input bit b, MSB first, the result is XORed with the 32 bits of rss_key that start at bit b.
 *  - plen: the packet's length under the batch clamp rules (the table's byte weight for fixed-stride callers).
 *  - A packet whose status is not PKT_FLOW_OK has an all-zero key and hash = rss = dir = 0; plen is written.
 *  - keys / hash / rss / dir / plen / status: device [n], each may be NULL.
 *  - PKT_ERR_INVALID_ARG, before any launch: pkt_l4_checksum_batch's refusals (batch and slab rules, a NULL
 *    chain or, with n > 0, chain column, n >= 2^32, unknown flag bits, a bad which_ip), rss without rss_key,
 *    keys not 2-byte aligned.  n == 0 succeeds and launches nothing.
 * Asynchronous on `stream`; keeps no ctx state.  pkt_flow_key_host: the same on HOST pointers, no device. */
typedef struct pkt_flow_key {      /* 40 bytes */
    uint8_t  src[16];              /* wire bytes; IPv4 in [0..4), the rest 0 */
    uint8_t  dst[16];
    uint16_t sport;                /* values (host order); 0 when not taken */
    uint16_t dport;
    uint8_t  proto;                /* IPv4 byte 9 / IPv6 byte 6, as read */
    uint8_t  ipver;                /* 4 or 6 */
    uint16_t zero;
} pkt_flow_key_t;
typedef enum pkt_flow_status {
    PKT_FLOW_OK    = 0,
    PKT_FLOW_NO_IP = 1, /* the chain has no such IPv4 / IPv6 entry */
    PKT_FLOW_SPAN  = 2  /* the IP header, or the ports that would be taken, do not lie inside the packet */
} pkt_flow_status_t;
#define PKT_FLOW_LAST       0xFFu  /* which_ip: the last (innermost) IPv4 / IPv6 entry of the list */
#define PKT_FLOW_SYMMETRIC  1u     /* flags: order the two ends, so both directions share a key */
#define PKT_FLOW_NO_PORTS   2u     /* flags: never take ports */
size_t pkt_sizeof_flow_key(void);
int pkt_flow_key_batch(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                       uint32_t flags, uint64_t seed, const uint8_t rss_key[40], pkt_flow_key_t *keys,
                       uint64_t *hash, uint32_t *rss, uint8_t *dir, uint32_t *plen, uint8_t *status, void *stream);
int pkt_flow_key_host(const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip, uint32_t flags,
                      uint64_t seed, const uint8_t rss_key[40], pkt_flow_key_t *keys, uint64_t *hash,
                      uint32_t *rss, uint8_t *dir, uint32_t *plen, uint8_t *status);

/* pkt_flow_table_*: an open-addressing table of `slots` entries (a power of two, 64..2^28; 128 bytes each) that
 * the handle owns, in the memory of the ctx's device (create) or in host memory (create_host: every call
 * then takes HOST pointers, runs a sequential loop and touches no device).  No memory is allocated in any
 * call after create.  One call at a time per table.
 *  - update (asynchronous; [n] arrays, n < 2^32): keys (8-byte aligned) and hash are required; dir NULL =
 *    every packet is direction 0 (otherwise its bit 0 counts); weight NULL = bytes are not counted; status
 *    NULL = every packet is OK; flow_id and upd_status may each be NULL.  Packet i has the global index
 *    base + i, and base must be >= the previous update's base + n on this table (the table keeps that
 *    high-water mark, clear resets it), else PKT_ERR_INVALID_ARG.
 *  - tag = hash & mask(tag_bits), 0 mapped to 1.  Probing starts at splitmix64(tag) & (slots - 1) and is
 *    linear.  An entry belongs to one tag; its key is the key of the first packet, by base + i, that ever
 *    reached it.  A packet whose key equals its entry's key is PKT_FLOW_UPD_OK: pkts[dir] += 1, bytes[dir] +=
 *    weight, flow_id = the slot.  One with the same tag and another key is PKT_FLOW_UPD_COLLISION and is
 *    counted nowhere (at 64 tag bits that needs a 64-bit hash collision; set_tag_bits, 1..64, allowed on a
 *    table that has seen no update since create / clear, lets a test make them happen).  A tag that finds
 *    neither its entry nor an empty slot in `slots` probes makes its packets PKT_FLOW_UPD_FULL: which tags
 *    lose when the table fills is unspecified, the entries the table holds stay exact.  A packet with
 *    status[i] != 0 is PKT_FLOW_UPD_SKIPPED.  flow_id is 0xFFFFFFFF for every packet that is not UPD_OK.
 *  - Counters are integer atomics: exact.  Slot numbers may differ from run to run, the set of records not.
 *  - count (blocking): the number of entries.  export (blocking): the entries in ascending slot order,
 *    min(cap, count) records written, *n_out = count.  clear (asynchronous): the empty table.
 *  - On the device, update is three launches (claim the entry and its lowest index; the packet with that
 *    index stores the key; compare and count), the kernel boundaries publish the data: no lane ever waits
 *    for another; a wave adds once per entry and direction it holds, a block of packets of one flow once. */
typedef struct pkt_flow_table pkt_flow_table_t;
typedef struct pkt_flow_record {   /* 80 bytes */
    pkt_flow_key_t key;
    uint64_t first;                /* lowest base + i of the flow's packets */
    uint64_t pkts[2];              /* by dir */
    uint64_t bytes[2];
} pkt_flow_record_t;
typedef enum pkt_flow_upd {
    PKT_FLOW_UPD_OK        = 0,
    PKT_FLOW_UPD_SKIPPED   = 1,
    PKT_FLOW_UPD_COLLISION = 2,
    PKT_FLOW_UPD_FULL      = 3
} pkt_flow_upd_t;
size_t pkt_sizeof_flow_record(void);
int pkt_flow_table_create(pkt_ctx_t *ctx, uint64_t slots, pkt_flow_table_t **table);
int pkt_flow_table_create_host(uint64_t slots, pkt_flow_table_t **table);
int pkt_flow_table_set_tag_bits(pkt_flow_table_t *table, uint32_t bits);
int pkt_flow_table_update(pkt_flow_table_t *table, const pkt_flow_key_t *keys, const uint64_t *hash,
                          const uint8_t *dir, const uint32_t *weight, const uint8_t *status, uint64_t n,
                          uint64_t base, uint32_t *flow_id, uint8_t *upd_status, void *stream);
int pkt_flow_table_count(pkt_flow_table_t *table, uint64_t *flows, void *stream);
int pkt_flow_table_export(pkt_flow_table_t *table, pkt_flow_record_t *records, uint64_t cap, uint64_t *n_out,
                          void *stream);
int pkt_flow_table_clear(pkt_flow_table_t *table, void *stream);
int pkt_flow_table_destroy(pkt_flow_table_t *table);
const char *pkt_flow_table_last_error(const pkt_flow_table_t *table);

/* ---- first-match rule tables over a parsed batch ----
 * Which packets a consumer keeps: the producer of the `select` mask that pkt_pcap_write and pkt_edit_batch
 * take, and the classifier beside the flow table.  The reference defines nothing here, so this header fixes the
 * semantics.  A program is up to PKT_MATCH_MAX_RULES rules over up to PKT_MATCH_MAX_TERMS terms; it is compiled
 * and uploaded once (pkt_match_create) and evaluated by one kernel in a single pass over the packets' bytes.
 *  - batch / chain: any pkt_batch_t under its usual slab rules, with the chain columns of a parse of it, of a
 *    stream's columns over pkt_pcap_stream_batch, or pkt_edit_batch's out_chain.  `len` is the packet's length
 *    under the pkt_batch_t clamp rules (clamped to the slab end and to 65535); n_hdrs is taken as
 *    min(n_hdrs, PKT_MAX_HDRS).  Whatever the columns hold, no byte outside the packet is used.
 *  - A term's header is the `occurrence`-th list entry of `hdr_type` (0 = first), counted as
 *    pkt_extract_fields counts.  It is PRESENT iff such an entry exists and hdr_off + pkt_hdr_size(hdr_type)
 *    <= len.  v = bits [start..=end], MSB-first from the header's first byte: pkt_extract_fields' value;
 *    width 1..64.
 *  - PKT_MATCH_HAS: raw = present (start, end, a, b ignored).  PKT_MATCH_EQ: raw = present and
 *    ((v ^ a) & b & widthmask) == 0, so a mask of 0 is true whenever the header is present.  PKT_MATCH_RANGE:
 *    raw = present and a <= v <= b, unsigned; a > b is allowed and never true.  PKT_MATCH_LEN: raw = a <= len
 *    <= b; its `field` must be all zero.  A term's result is raw ^ PKT_MATCH_NOT, so NOT on an absent header
 *    is true.  An IPv6 address is two 64-bit terms, a /64 prefix one.
 *  - Rule r matches iff all its terms [first_term, first_term + nterms) are true; a rule with nterms == 0
 *    matches every packet (n_hdrs == 0 included).  The rules' ranges may overlap or share terms.
 *  - matched[i]: bit r set iff rule r matches.  rule[i]: the lowest matching r, else PKT_MATCH_NONE.
 *    action[i]: that rule's action, else default_action.  select[i] = action[i] != 0: exactly what
 *    pkt_pcap_write and pkt_edit_batch take.  rule / action / select / matched: device [n], each may be NULL.
 *  - hits / bytes: device uint64_t[nrules + 1], 8-byte aligned, caller-owned, each may be NULL.  They are ADDED
 *    to: the caller zeroes them once and they accumulate across batches and stream windows.  hits[rule[i]] +=
 *    1, bytes[rule[i]] += len, index nrules standing for "none".  Integer atomics, exact: every call adds
 *    exactly n to sum(hits).  With all six outputs NULL the call succeeds and launches nothing.
 *  - pkt_match_create validates, compiles and uploads the program; blocking, and the only allocation (the
 *    pkt_gen_create pattern).  PKT_ERR_INVALID_ARG with a text in pkt_ctx_last_error: nrules > 64 or nterms >
 *    256; a rule range that runs past nterms; an unknown op or flag bit; non-zero reserved fields; a non-LEN
 *    term with hdr_type outside 1..21, end < start, end >= 8 * pkt_hdr_size(hdr_type) or a width above 64
 *    (HAS ignores the bits but still needs a valid type); a LEN term with a non-zero `field`; a NULL pointer
 *    with a non-zero count.  nrules == 0 is legal: every packet gets default_action.
 *  - pkt_match_batch is asynchronous on `stream`, keeps no ctx state and never writes the program: several
 *    calls on one program may be in flight on different streams.  PKT_ERR_INVALID_ARG before any launch (the
 *    text: pkt_ctx_last_error of the ctx the program was created on): the batch and slab rules, a NULL chain or,
 *    with n > 0, chain column, n >= 2^32, a matched, hits or bytes that is not 8-byte aligned.  n == 0
 *    succeeds, launches nothing and leaves the counters untouched.  pkt_match_destroy is the caller's to order
 *    after the queued calls.
 *  - On the device a lane owns a packet: its window and chain are loaded once whatever the number of rules,
 *    the compiled program is read through uniform (scalar) loads, each distinct (hdr_type, occurrence) is
 *    resolved once per packet, a block merges its counts in LDS and adds once per non-zero (rule, counter).
 *    No lane waits for another.
 * pkt_match_host is the same operation on HOST pointers, straight from the terms and rules: no ctx, no device. */
#define PKT_MATCH_MAX_RULES 64
#define PKT_MATCH_MAX_TERMS 256
#define PKT_MATCH_NONE      0xFFu      /* rule[i] when no rule matched */
#define PKT_MATCH_NOT       1u         /* term flag: invert the term */
typedef enum pkt_match_op { PKT_MATCH_HAS = 0, PKT_MATCH_EQ = 1, PKT_MATCH_RANGE = 2, PKT_MATCH_LEN = 3 } pkt_match_op_t;
typedef struct pkt_match_term {        /* 32 bytes */
    pkt_field_spec_t field;            /* header type, occurrence, bits [start..=end] as pkt_extract_fields */
    uint8_t  op;                       /* pkt_match_op_t */
    uint8_t  flags;                    /* PKT_MATCH_NOT or 0 */
    uint16_t reserved;                 /* 0 */
    uint32_t reserved2;                /* 0 */
    uint64_t a;                        /* EQ: value.  RANGE / LEN: lo */
    uint64_t b;                        /* EQ: mask.   RANGE / LEN: hi, inclusive */
} pkt_match_term_t;
typedef struct pkt_match_rule {        /* 8 bytes */
    uint16_t first_term;               /* the rule is the AND of terms [first_term, first_term + nterms) */
    uint16_t nterms;
    uint32_t action;                   /* caller-defined; 0 means "not selected" */
} pkt_match_rule_t;
typedef struct pkt_match pkt_match_t;
size_t pkt_sizeof_match_term(void);
size_t pkt_sizeof_match_rule(void);
int pkt_match_create(pkt_ctx_t *ctx, const pkt_match_term_t *terms, uint32_t nterms,
                     const pkt_match_rule_t *rules, uint32_t nrules, uint32_t default_action, pkt_match_t **m);
int pkt_match_destroy(pkt_match_t *m);
int pkt_match_batch(pkt_match_t *m, const pkt_batch_t *batch, const pkt_chain_t *chain,
                    uint8_t *rule, uint32_t *action, uint8_t *select, uint64_t *matched,
                    uint64_t *hits, uint64_t *bytes, void *stream);
int pkt_match_host(const pkt_match_term_t *terms, uint32_t nterms, const pkt_match_rule_t *rules, uint32_t nrules,
                   uint32_t default_action, const pkt_batch_t *batch, const pkt_chain_t *chain,
                   uint8_t *rule, uint32_t *action, uint8_t *select, uint64_t *matched, uint64_t *hits, uint64_t *bytes);

/* ---- per-queue batches: a stable bucket partition and the gather that follows it ----
 * What an RSS hash exists for: hand each packet of a device batch to one of N queues, workers or GPUs, in one pass
 * over the bytes.  pkt_dispatch_batch partitions n packets into buckets by a 32-bit key (pkt_flow_key_batch's rss,
 * pkt_match_batch's action or rule, a shard number); pkt_reorder_batch gathers packets and columns by the
 * resulting permutation into per-bucket batches every pkt_*_batch call accepts.  The reference defines nothing
 * here, so this header fixes the semantics; the one outside convention is the RSS indirection table,
 * queue = table[hash & (len - 1)].
 *
 * pkt_dispatch_create: blocking, and the only allocation (the pkt_match_create pattern); the handle owns the
 * scratch for max_n packets.  nbuckets in 1..PKT_DISPATCH_MAX_BUCKETS; `table` is HOST memory, captured at the
 * call: NULL selects DIRECT mode, otherwise table_len is a power of two in 1..PKT_DISPATCH_MAX_TABLE and every
 * entry is < nbuckets or PKT_DISPATCH_DROP; max_n in 1..2^32-1.  A violation is PKT_ERR_INVALID_ARG with a text
 * starting "pkt_dispatch" in pkt_ctx_last_error.
 *  - The bucket b_i of packet i: PKT_DISPATCH_DROP if `select` is non-NULL and select[i] == 0; in DIRECT mode
 *    key[i] < nbuckets ? key[i] : PKT_DISPATCH_DROP; in table mode table[key[i] & (table_len - 1)].
 *  - Order: packets are ordered by (b'_i, i) with b' = nbuckets for DROP, so the partition is stable (source
 *    order is kept within a bucket) and the dropped packets form the tail.  perm[pos] = i and rank[i] = pos
 *    (device uint32_t[n]); bucket[i] = b_i (device uint16_t[n], DROP as 0xFFFF); start: device
 *    uint64_t[nbuckets + 2], 8-byte aligned, start[b] = the number of packets with b' < b, so start[0] = 0,
 *    start[nbuckets] = the kept count and start[nbuckets + 1] = n.  start is written, not added to.  All results
 *    are exact and the same from run to run.
 *  - Every output may be NULL; with all four NULL nothing is launched.  key (device uint32_t[n]) is required when
 *    n > 0.  For n == 0, start (if given) is zero-filled on the stream and nothing else happens.  n > max_n,
 *    n >= 2^32 or a misaligned start is PKT_ERR_INVALID_ARG before any launch (the text: pkt_ctx_last_error of the
 *    ctx the handle was created on).  Asynchronous on `stream`; one call at a time per handle (the calls share
 *    its scratch), as for pkt_flow_table.  pkt_dispatch_destroy is the caller's to order after the queued calls.
 *  - On the device three launches whose boundaries publish the data (no lane waits for another, no global
 *    atomics): each tile of 2048 packets counts its buckets; one exclusive scan over the [bucket][tile] counts
 *    gives every tile's first position in every bucket, and start; each tile then ranks its packets again, within
 *    a wave by ballots over the bucket's bits, and stores perm, rank and bucket.
 * pkt_dispatch_host is the same operation on HOST pointers: no ctx, no device, no handle.
 *
 * pkt_reorder_batch: position k < m takes source packet p = perm[k] (`perm`: device uint32_t[m], pkt_dispatch_
 * batch's perm or any index list).  p >= batch->n is an EMPTY position: out_len = 0, every gathered column 0, no
 * packet byte written.  Whatever perm and the columns hold, no byte outside the source packets is used and none
 * outside what is listed here is written.
 *  - Bytes (dst != NULL): dst is 16-byte aligned, `slot` a multiple of 16 and at least 16, dst_len >= m * slot.
 *    out_len[k] = min(len_p, slot) with len_p the packet's length under the pkt_batch_t clamp rules: the cut is
 *    pkt_pcap_write's snaplen, not an error.  Exactly bytes [k*slot, k*slot + round_up(out_len[k], 16)) of dst
 *    are written, the packet's bytes, then zeros; the rest of the slot is not written and dst is never read.  The
 *    source is any pkt_batch_t under its usual slab rules, its packets at any alignment; it must not overlap dst.
 *    out_len (device uint32_t[m]) may be NULL.  dst == NULL means columns only; out_len must then be NULL.
 *  - Columns: column c (any of pkt_out_t's 49) is gathered iff cols->c and out_cols->c are both non-NULL;
 *    out_cols->c without cols->c is PKT_ERR_INVALID_ARG; either struct may be NULL (no columns).  Input slot
 *    columns are strided by batch->n.  A per-packet column writes element k.  With nseg == 0 the slot columns are
 *    written as [PKT_MAX_HDRS][m].
 *  - Segments: seg_start is a device uint64_t[nseg + 1] holding what pkt_dispatch_batch's `start` holds, nseg <=
 *    257; the caller promises it is non-decreasing from 0; its values are clamped to m.  Segment s is positions
 *    [seg_start[s], seg_start[s+1]) and n_s its size; row j of a slot column lies at element PKT_MAX_HDRS *
 *    seg_start[s] + j * n_s + (k - seg_start[s]).  Positions at or past seg_start[nseg] are not written at all
 *    (no bytes, no out_len, no columns): with m = n and nseg = nbuckets this skips the dropped tail.
 *  - Slot rows: when cols->n_hdrs is given only rows j < min(n_hdrs[p], PKT_MAX_HDRS) are written, as a parse
 *    leaves the later ones; without it, and for an empty position, all PKT_MAX_HDRS rows are.
 *  - Why this layout: segment s is a batch of its own, {slab = dst + seg_start[s]*slot, slab_len = n_s*slot,
 *    stride = slot, lens = out_len + seg_start[s], n = n_s} with the chain {n_hdrs + seg_start[s], hdr_type +
 *    PKT_MAX_HDRS*seg_start[s], hdr_off + PKT_MAX_HDRS*seg_start[s]}: slot-major over ITS n_s packets, which a
 *    slice of a [PKT_MAX_HDRS][m] column is not.  Every pkt_*_batch call takes it with no second parse.
 *  - PKT_ERR_INVALID_ARG before any launch: the batch and slab rules with their texts (with dst, for a batch of
 *    n > 0), m >= 2^32, a bad slot, a misaligned dst, a dst_len below m * slot, out_len without dst, nseg > 257,
 *    nseg > 0 with a NULL seg_start, a seg_start that is not 8-byte aligned, a NULL perm with m > 0, an out column without its source.  m == 0 succeeds
 *    and launches nothing.  Asynchronous on `stream`; keeps no ctx state.
 *  - On the device: a bytes kernel (a wave covers 64 positions and walks their 16-byte chunks together: aligned
 *    16-byte stores, the tail chunk masked) and a column kernel (a lane owns a position, reads perm[k] once for
 *    all columns and finds its segment in a copy of seg_start in LDS).
 * pkt_reorder_host is the same operation on HOST pointers: no ctx, no device.
 * Out of scope: more than 256 buckets or a full key sort; variable-length packed output (pkt_pcap_write on a
 * segment gives the packed form); concurrent calls on one handle. */
#define PKT_DISPATCH_MAX_BUCKETS 256
#define PKT_DISPATCH_MAX_TABLE   4096
#define PKT_DISPATCH_DROP        0xFFFFu
#define PKT_REORDER_MAX_SEGS     257
typedef struct pkt_dispatch pkt_dispatch_t;
int pkt_dispatch_create(pkt_ctx_t *ctx, uint32_t nbuckets, const uint16_t *table, uint32_t table_len,
                        uint64_t max_n, pkt_dispatch_t **d);
int pkt_dispatch_destroy(pkt_dispatch_t *d);
int pkt_dispatch_batch(pkt_dispatch_t *d, const uint32_t *key, const uint8_t *select, uint64_t n,
                       uint16_t *bucket, uint32_t *perm, uint32_t *rank, uint64_t *start, void *stream);
int pkt_dispatch_host(uint32_t nbuckets, const uint16_t *table, uint32_t table_len, const uint32_t *key,
                      const uint8_t *select, uint64_t n, uint16_t *bucket, uint32_t *perm, uint32_t *rank,
                      uint64_t *start);
int pkt_reorder_batch(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_out_t *cols, const uint32_t *perm,
                      uint64_t m, const uint64_t *seg_start, uint32_t nseg, uint8_t *dst, uint64_t dst_len,
                      uint32_t slot, uint32_t *out_len, const pkt_out_t *out_cols, void *stream);
int pkt_reorder_host(const pkt_batch_t *batch, const pkt_out_t *cols, const uint32_t *perm, uint64_t m,
                     const uint64_t *seg_start, uint32_t nseg, uint8_t *dst, uint64_t dst_len, uint32_t slot,
                     uint32_t *out_len, const pkt_out_t *out_cols);

/* ---- longest-prefix-match route tables over a parsed batch ----
 * Where an IP packet goes: the step between "classified" and "dispatched", and the natural producer of the 32-bit
 * key pkt_dispatch_batch takes in DIRECT mode (a next hop, an egress port, a queue).  A route table of up to
 * PKT_LPM_MAX_ROUTES IPv4 and IPv6 prefixes is compiled once into a device-resident multibit trie
 * (pkt_lpm_create); one kernel then gives, per packet, the longest matching route and its next hop.  The
 * reference defines nothing here, so this header fixes the semantics.
 *
 * pkt_lpm_create / pkt_lpm_create_host
 *  - Blocking, and the only allocation (the pkt_match_create pattern).  `routes` is HOST memory, captured at the
 *    call.  max_bytes bounds the compiled table; 0 means 1 GiB.  nroutes == 0 is legal: every IP packet is
 *    PKT_LPM_NO_ROUTE.
 *  - PKT_ERR_INVALID_ARG with a text starting "pkt_lpm": nroutes > PKT_LPM_MAX_ROUTES; NULL routes with nroutes >
 *    0; an ipver that is neither 4 nor 6; a plen above 32 (IPv4) or 128 (IPv6); a non-zero `zero`; any address bit
 *    at or past plen set (IPv4's bytes 4..15 included); two routes with the same (ipver, plen, prefix).
 *    PKT_ERR_UNSUPPORTED when the compiled table needs more than max_bytes; the text names the bytes needed.
 *    The text of a failed pkt_lpm_create is in pkt_ctx_last_error; that of a failed pkt_lpm_create_host, which has
 *    neither ctx nor handle, in pkt_lpm_last_error(NULL) of the calling thread.
 *  - The table: one root of 2^16 entries per IP version (the address's first 16 bits), below it nodes of 256
 *    entries (8 bits each): at most 3 levels for IPv4 and 15 for IPv6.  An entry is a uint32_t: bit 31 set = the
 *    low bits are a child node's index, otherwise a route's index + 1, 0 = no route.  A route of length L <= 16
 *    fills 2^(16-L) root entries, one with 16+8k < L <= 24+8k fills 2^(24+8k-L) entries of one node of level k+1;
 *    routes go in by ascending plen, so a longer prefix overwrites a shorter one where they overlap, and a new
 *    child node starts as a copy of the entry it hangs under (leaf pushing).  A lookup is a chain of dependent
 *    4-byte loads that ends at the first entry without bit 31, with no backtracking; a route's {nexthop, plen}
 *    record (8 bytes) is read once at the end.  pkt_lpm_info: routes_v4 / routes_v6, nodes_v4 / nodes_v6 (256-entry
 *    nodes, roots not counted), depth_v4 / depth_v6 (the deepest level a route reached, the root being 1; 0 for no
 *    route), bytes = both roots (2 x 256 KiB) + 1 KiB per node + 8 per route.
 *
 * The result for one address: the route of the address's IP version with the greatest plen whose first plen bits
 * equal the address's (unique: duplicates are refused); a /0 route matches every address of its version.  On a
 * match status = PKT_LPM_OK, route[i] = the route's index in the caller's array, nexthop[i] = its nexthop, plen[i]
 * = its plen.  For every other status route = PKT_LPM_NONE, nexthop = default_nexthop, plen = 0xFF.
 *
 * pkt_lpm_lookup_batch
 *  - batch / chain / which_ip (PKT_FLOW_LAST included) and the min(n_hdrs, PKT_MAX_HDRS) rule are exactly
 *    pkt_flow_key_batch's; whatever the columns hold, no byte outside the packet is used.  The address is bytes
 *    16..19 (destination) or, with PKT_LPM_SRC, 12..15 of an IPv4 entry, and 24..39 or 8..23 of an IPv6 entry.
 *    No such entry: PKT_LPM_NO_IP.  The entry's 20 / 40 bytes not inside the packet: PKT_LPM_SPAN (the test
 *    PKT_FLOW_SPAN makes for the IP header).
 *  - PKT_ERR_INVALID_ARG before any launch, with a text in pkt_lpm_last_error: pkt_flow_key_batch's refusals (the
 *    batch and slab rules, a NULL chain or, with n > 0, chain column, n >= 2^32, a bad which_ip) and unknown flag
 *    bits.
 * pkt_lpm_lookup_keys
 *  - The address is keys[i].dst (or .src with PKT_LPM_SRC) and the version keys[i].ipver: pkt_flow_key_batch's
 *    output.  A packet is PKT_LPM_SKIPPED if key_status is non-NULL and key_status[i] != 0, or if ipver is neither
 *    4 nor 6.  With PKT_FLOW_SYMMETRIC keys the two ends may have been swapped: which one is the destination is
 *    then the caller's concern.
 *  - PKT_ERR_INVALID_ARG: NULL keys with n > 0, keys not 2-byte aligned, n >= 2^32, unknown flag bits.
 * Both lookups
 *  - route / nexthop: uint32_t[n]; plen / status: uint8_t[n].  Every output may be NULL; with all four NULL nothing
 *    is launched.  n == 0 succeeds and launches nothing.
 *  - Asynchronous on `stream`.  A lookup never writes the table, so several lookups on one handle may be in flight
 *    on different streams.  pkt_lpm_destroy is the caller's to order after the queued calls.
 *  - A handle from pkt_lpm_create_host takes HOST pointers everywhere, ignores `stream`, runs a sequential loop
 *    and touches no device (the pkt_flow_table_create_host pattern; the slab's alignment rule is waived).  Both
 *    kinds of handle share one compile and one walk.
 *  - On the device a lane owns a packet: one kernel, no lane waits for another, no atomics.  The loop over levels
 *    is bounded by the table's depth, not by 3 / 15.
 * Out of scope: incremental insert and delete (rebuild, then swap handles); per-route hit counters (a bincount of
 * `route`); path compression of long IPv6 chains; ECMP / multipath; IPv4 options and IPv6 extension headers (the
 * walk models neither). */
typedef struct pkt_lpm_route {     /* 24 bytes */
    uint8_t  addr[16];             /* wire bytes; IPv4 in [0..4), the rest 0 */
    uint8_t  ipver;                /* 4 or 6 */
    uint8_t  plen;                 /* 0..32 / 0..128 */
    uint16_t zero;
    uint32_t nexthop;              /* caller-defined: a port, a queue, an adjacency index */
} pkt_lpm_route_t;
typedef struct pkt_lpm_info {      /* 56 bytes */
    uint64_t routes_v4;
    uint64_t routes_v6;
    uint64_t nodes_v4;
    uint64_t nodes_v6;
    uint64_t depth_v4;
    uint64_t depth_v6;
    uint64_t bytes;
} pkt_lpm_info_t;
typedef enum pkt_lpm_status {
    PKT_LPM_OK       = 0,
    PKT_LPM_NO_ROUTE = 1, /* no route of the address's version covers it */
    PKT_LPM_NO_IP    = 2, /* the chain has no such IPv4 / IPv6 entry */
    PKT_LPM_SPAN     = 3, /* the IP header does not lie inside the packet */
    PKT_LPM_SKIPPED  = 4  /* lookup_keys: key_status[i] != 0, or an ipver that is neither 4 nor 6 */
} pkt_lpm_status_t;
#define PKT_LPM_NONE       0xFFFFFFFFu /* route[i] when status != PKT_LPM_OK */
#define PKT_LPM_SRC        1u          /* flags: look up the source address (default: destination) */
#define PKT_LPM_MAX_ROUTES (1u << 24)
typedef struct pkt_lpm pkt_lpm_t;
size_t pkt_sizeof_lpm_route(void);
int pkt_lpm_create(pkt_ctx_t *ctx, const pkt_lpm_route_t *routes, uint32_t nroutes, uint32_t default_nexthop,
                   uint64_t max_bytes, pkt_lpm_t **lpm);
int pkt_lpm_create_host(const pkt_lpm_route_t *routes, uint32_t nroutes, uint32_t default_nexthop,
                        uint64_t max_bytes, pkt_lpm_t **lpm);
int pkt_lpm_info(const pkt_lpm_t *lpm, pkt_lpm_info_t *info);
int pkt_lpm_lookup_batch(pkt_lpm_t *lpm, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                         uint32_t flags, uint32_t *route, uint32_t *nexthop, uint8_t *plen, uint8_t *status,
                         void *stream);
int pkt_lpm_lookup_keys(pkt_lpm_t *lpm, const pkt_flow_key_t *keys, const uint8_t *key_status, uint64_t n,
                        uint32_t flags, uint32_t *route, uint32_t *nexthop, uint8_t *plen, uint8_t *status,
                        void *stream);
int pkt_lpm_destroy(pkt_lpm_t *lpm);
const char *pkt_lpm_last_error(const pkt_lpm_t *lpm);

/* ---- L3 forwarding rewrite over a routed batch ----
 * The step a router takes between "routed" and "queued": resolve the next hop's adjacency, rewrite the two MAC
 * addresses, decrement the TTL / hop limit and refuse the packets whose TTL has run out, fix the IPv4 header
 * checksum, check the egress MTU and say which port the packet leaves on.  pkt_lpm's next hop is "a port, a queue, an
 * adjacency index"; this call resolves the adjacency index, in one kernel, optionally fused with the route lookup.
 * The reference defines nothing here, so this header fixes the semantics.
 *
 * pkt_fwd_create: blocking, and the only allocation (the pkt_match_create pattern).  `adj` is HOST memory, captured at
 * the call; nadj == 0 is legal (every packet that gets as far as the adjacency is PKT_FWD_NO_ADJ).
 * PKT_ERR_INVALID_ARG with a text starting "pkt_fwd" in pkt_ctx_last_error: nadj > PKT_FWD_MAX_ADJ; NULL adj with
 * nadj > 0; an `action` above 2; a non-zero `zero`.  The device copy is padded (32 bytes an entry, so that an entry
 * is two aligned 16-byte loads); that layout is private.
 *
 * pkt_fwd_batch, per packet i: the first test that applies gives status[i], and a packet whose status is not
 * PKT_FWD_OK is not written at all.
 *  1. select != NULL && select[i] == 0: PKT_FWD_SKIPPED.
 *  2. The IP entry is found exactly as in pkt_flow_key_batch / pkt_lpm_lookup_batch: which_ip (PKT_FLOW_LAST
 *     included) counts the IPv4 and IPv6 entries of the list together, over min(n_hdrs, PKT_MAX_HDRS) entries; a
 *     which_ip in 16..0xFE is refused.  No such entry: PKT_FWD_NO_IP.  Its 20 / 40 bytes not inside the packet's
 *     length (under the pkt_batch_t clamp rules): PKT_FWD_SPAN.
 *  3. Unless PKT_FWD_KEEP_L2: the Ether entry is the list entry of type PKT_HDR_ETHER with the greatest index below
 *     the IP entry's index (for a VXLAN packet's inner IP that is the inner Ethernet header).  None:
 *     PKT_FWD_NO_ETHER.  Its 14 bytes not inside the packet: PKT_FWD_SPAN.
 *  4. t = byte 8 of an IPv4 entry (ttl), byte 7 of an IPv6 entry (hop limit).  t <= 1: PKT_FWD_TTL.
 *  5. The adjacency index a: nexthop[i] when `nexthop` is given; otherwise what pkt_lpm_lookup_batch(lpm, batch,
 *     chain, which_ip, 0, ...) writes to nexthop[i]: the next hop of the destination address's route, or the
 *     table's default_nexthop when no route covers it.  Exactly one of lpm / nexthop must be non-NULL.
 *     a >= nadj: PKT_FWD_NO_ADJ.  adj[a].action PKT_FWD_ACT_DROP: PKT_FWD_DROP; PKT_FWD_ACT_PUNT: PKT_FWD_PUNT.
 *  6. adj[a].mtu != 0 and the L3 length > mtu: PKT_FWD_MTU.  The L3 length is bytes 2..3 of an IPv4 entry, or 40 +
 *     bytes 4..5 of an IPv6 entry, big-endian: it comes from the IP header, not from the packet's length.
 *  7. PKT_FWD_OK.
 * The writes of an OK packet (none with PKT_FWD_NO_WRITE):
 *  - Ether bytes 0..5 = dmac and 6..11 = smac (not with PKT_FWD_KEEP_L2).
 *  - IPv4 byte 8 = t - 1; IPv6 byte 7 = t - 1.
 *  - IPv4 bytes 10..11 = HC', big-endian, by RFC 1624 eq. 3: with HC the stored checksum, m = bytes 8..9 as a
 *    big-endian word and m' = m - 0x0100: s = (~HC & 0xFFFF) + (~m & 0xFFFF) + m', folded twice (s = (s & 0xFFFF)
 *    + (s >> 16)), HC' = ~s & 0xFFFF.  This is deliberately NOT Packet::ipv4_checksum: the header is not summed
 *    again and there is no Q1 fold, so a checksum that was wrong before stays wrong by the same amount, as it does
 *    in a forwarding plane (pkt_set_fields_csum / pkt_ipv4_update_checksum are the recomputing calls).
 *  - Stores may rewrite other bytes of the packet's own Ether bytes 0..11 and of its own IP header with their
 *    unchanged values; no byte outside those two ranges is written, not even with its own value.  Packets of one
 *    batch must not overlap (the pkt_set_fields rule).  Columns that are not a parse of the batch give
 *    unspecified packet bytes, but never an access outside the packet.
 * Outputs: device arrays of n elements, each may be NULL.  status: uint8_t.  port: uint32_t, adj[a].port iff
 * status is PKT_FWD_OK, else PKT_FWD_NONE: pkt_dispatch_batch in DIRECT mode then drops what was not forwarded.
 * adj_index: uint32_t, a for every packet that reached step 5, else PKT_FWD_NONE.  hits / bytes: device
 * uint64_t[PKT_FWD_STATUS_COUNT], 8-byte aligned, caller-owned, ADDED to as pkt_match_batch's counters are:
 * hits[status] += 1, bytes[status] += the packet's length under the batch clamp; integer atomics, exact: every call
 * adds exactly n to sum(hits).  With every output NULL and PKT_FWD_NO_WRITE set nothing is launched.
 *  - PKT_ERR_INVALID_ARG before any launch (the text, starting "pkt_fwd", in pkt_ctx_last_error of the ctx the
 *    handle was created on): pkt_flow_key_batch's batch and slab rules, a NULL chain or, with n > 0, chain column,
 *    n >= 2^32, a bad which_ip, unknown flag bits, both or neither of lpm / nexthop, an lpm that is a host handle
 *    or was created on another device, hits / bytes that are not 8-byte aligned.  n == 0 succeeds, launches
 *    nothing and leaves the counters alone.
 *  - Asynchronous on `stream`.  The call never writes the handle or the lpm table, so calls over different batches
 *    may be in flight on different streams.  pkt_fwd_destroy is the caller's to order after the queued calls.
 *  - On the device a lane owns a packet: one kernel, the IP header's first 12 bytes (and, with lpm, the address)
 *    by the aligned 16-byte chunks that hold them, the adjacency by two 16-byte loads, narrow stores to the bytes
 *    named above; a block merges its per-status counts in LDS and adds once per non-zero (status, counter).  No
 *    lane waits for another.
 * pkt_fwd_host is the same operation on HOST pointers: no ctx, no device, no handle.  Its lpm, if given, must be a
 * handle from pkt_lpm_create_host; the slab's 16-byte alignment rule is waived, as for that handle.
 * Out of scope: VLAN push or rewrite (pkt_edit_batch / pkt_set_fields); ICMP time-exceeded and fragmentation-needed
 * generation (pkt_icmp_err_batch, below, takes this call's status array; fragmentation itself is pkt_frag_batch, below: it takes the PKT_FWD_MTU packets); ECMP; per-adjacency counters (a bincount of adj_index); NAT (pkt_nat_batch, below,
 * before this call); IPv4 options and
 * IPv6 extension headers (the walk models neither). */
typedef struct pkt_fwd_adj {       /* 20 bytes */
    uint8_t  dmac[6];              /* written to the Ether header's bytes 0..5 */
    uint8_t  smac[6];              /* written to bytes 6..11 */
    uint32_t port;                 /* caller-defined egress port / queue: the key pkt_dispatch_batch takes (DIRECT) */
    uint16_t mtu;                  /* 0 = no check; else the largest L3 length forwarded */
    uint8_t  action;               /* pkt_fwd_action_t */
    uint8_t  zero;
} pkt_fwd_adj_t;
typedef enum pkt_fwd_action { PKT_FWD_ACT_FORWARD = 0, PKT_FWD_ACT_DROP = 1, PKT_FWD_ACT_PUNT = 2 } pkt_fwd_action_t;
typedef enum pkt_fwd_status {
    PKT_FWD_OK       = 0,
    PKT_FWD_SKIPPED  = 1, /* select[i] == 0 */
    PKT_FWD_NO_IP    = 2, /* the chain has no such IPv4 / IPv6 entry */
    PKT_FWD_SPAN     = 3, /* the IP or the Ether header does not lie inside the packet */
    PKT_FWD_NO_ETHER = 4, /* no Ether entry before the IP entry */
    PKT_FWD_TTL      = 5, /* ttl / hop limit <= 1 */
    PKT_FWD_NO_ADJ   = 6, /* the adjacency index is not below nadj */
    PKT_FWD_DROP     = 7, /* the adjacency's action */
    PKT_FWD_PUNT     = 8, /* the adjacency's action */
    PKT_FWD_MTU      = 9  /* the L3 length is above the adjacency's mtu */
} pkt_fwd_status_t;
#define PKT_FWD_STATUS_COUNT 10
#define PKT_FWD_NONE     0xFFFFFFFFu   /* port[i] / adj_index[i] when there is none */
#define PKT_FWD_KEEP_L2  1u            /* flags: no Ether entry is looked for, no MAC is written */
#define PKT_FWD_NO_WRITE 2u            /* flags: decide everything, store nothing into the slab */
#define PKT_FWD_MAX_ADJ  (1u << 20)
typedef struct pkt_fwd pkt_fwd_t;
size_t pkt_sizeof_fwd_adj(void);
int pkt_fwd_create(pkt_ctx_t *ctx, const pkt_fwd_adj_t *adj, uint32_t nadj, pkt_fwd_t **f);
int pkt_fwd_destroy(pkt_fwd_t *f);
int pkt_fwd_batch(pkt_fwd_t *f, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                  uint32_t flags, pkt_lpm_t *lpm, const uint32_t *nexthop, const uint8_t *select,
                  uint8_t *status, uint32_t *port, uint32_t *adj_index, uint64_t *hits, uint64_t *bytes,
                  void *stream);
int pkt_fwd_host(const pkt_fwd_adj_t *adj, uint32_t nadj, const pkt_batch_t *batch, const pkt_chain_t *chain,
                 uint32_t which_ip, uint32_t flags, pkt_lpm_t *lpm, const uint32_t *nexthop,
                 const uint8_t *select, uint8_t *status, uint32_t *port, uint32_t *adj_index,
                 uint64_t *hits, uint64_t *bytes);

/* ---- IPv4 fragmentation of a batch to a per-packet MTU ----
 * What a router does with the packets pkt_fwd_batch leaves at PKT_FWD_MTU: one source packet becomes one or several
 * output packets, packed into a second slab, with the chain columns the following calls need (a second parse would
 * walk a non-first fragment's payload as an L4 header).  The reference defines nothing here, so this header fixes the
 * semantics; they follow RFC 791's fragmentation procedure and RFC 1624 for the checksum.
 *
 * pkt_frag_batch, per source packet i: the first test that applies gives status[i].
 *  1. select != NULL && select[i] == 0: PKT_FRAG_SKIPPED.
 *  2. The IP entry is found exactly as in pkt_flow_key_batch / pkt_lpm_lookup_batch / pkt_fwd_batch: which_ip
 *     (PKT_FLOW_LAST included) counts the IPv4 and IPv6 entries together over min(n_hdrs, PKT_MAX_HDRS) entries; a
 *     which_ip in 16..0xFE is refused.  No such entry: PKT_FRAG_NO_IP.  Its 20 / 40 bytes not inside the packet's
 *     length (under the pkt_batch_t clamp rules): PKT_FRAG_SPAN.
 *  3. m = mtu ? mtu[i] : mtu_all (mtu_all > 65535 is refused).  L is pkt_fwd_batch's L3 length: bytes 2..3 of an IPv4
 *     entry, or 40 + bytes 4..5 of an IPv6 entry.  m == 0 || L <= m: PKT_FRAG_FITS, with no other header check:
 *     FITS is exactly "step 6 of pkt_fwd_batch would not say PKT_FWD_MTU".
 *  4. An IPv6 entry: PKT_FRAG_IPV6 (routers do not fragment IPv6).
 *  5. Byte 0 != 0x45, or L < 20: PKT_FRAG_BAD_HDR (IPv4 options are out of scope; the walk does not model them).
 *  6. ip_off + L > the packet's length: PKT_FRAG_TRUNC.
 *  7. Byte 6 & 0x40: PKT_FRAG_DF.
 *  8. m < 28: PKT_FRAG_MTU (not even 8 payload bytes fit).
 *  9. per = (m - 20) & ~7, P = L - 20, k = ceil(P / per), w = bytes 6..7 big-endian, o = w & 0x1FFF.
 *     o + (k - 1) * per / 8 > 0x1FFF: PKT_FRAG_BAD_HDR.
 * 10. PKT_FRAG_SPLIT with nfrag = k (k >= 2, because L > m).
 * Outputs per source packet: FITS gives 1 (0 with PKT_FRAG_ONLY_SPLIT), SPLIT gives k, every other status 0.
 * nfrag[i] is that count, first[i] the index of its first output, or PKT_FRAG_NONE when nfrag[i] == 0.  Outputs are
 * ordered by (i, j): source order, then fragment order; the result is exact and the same from run to run.
 * A FITS output is the packet's bytes [0, len_i) verbatim, trailing padding included.  Fragment j of a SPLIT packet is
 *  - the source bytes [0, ip_off) verbatim: the L2 prefix and any outer headers.  When which_ip selects an inner
 *    header the outer headers' length fields (outer IP total length, UDP length) are NOT corrected: encapsulate
 *    first (pkt_tunnel_encap_batch, below, sets them) and fragment the outer datagram;
 *  - the 20-byte IP header, the source's with bytes 2..3 = 20 + the slice's length; bytes 6..7 = (w & 0xC000) | MF |
 *    (o + j * per / 8), MF = 0x2000 for j < k - 1 and w & 0x2000 for the last fragment (a fragment of a fragment keeps
 *    its more-fragments bit); bytes 10..11 = HC', updated incrementally over the two changed words, pkt_fwd_batch's
 *    way: s = (~HC & 0xFFFF) + (~L & 0xFFFF) + L' + (~w & 0xFFFF) + w', folded twice, HC' = ~s & 0xFFFF.  This is not
 *    Packet::ipv4_checksum: a checksum that was wrong stays wrong by the same amount;
 *  - payload bytes [j * per, min((j + 1) * per, P)) of the datagram.  Source bytes past ip_off + L (Ethernet padding)
 *    go nowhere.
 * Layout of dst: output q starts at out_off[q]; out_off[0] = 0 and out_off[q + 1] = out_off[q] + round_up(out_len[q],
 * 16); exactly the bytes [out_off[q], out_off[q] + round_up(out_len[q], 16)) are written: the packet, then zeros.  dst
 * is 16-byte aligned, never read, and must not overlap the source slab.  *bytes_out_total is the sum of the rounded
 * lengths, *n_out the number of outputs; nothing at or past *bytes_out_total is written.  Entries q in [*n_out,
 * out_cap) of the per-output arrays are written as empty (out_off 0, out_len 0, src_index PKT_FRAG_NONE, frag_index 0,
 * out_chain->n_hdrs 0), so the out_cap-sized arrays are at once an indexed pkt_batch_t of out_cap packets with an
 * empty tail, and out_chain is slot-major over it (columns strided by out_cap).  src_index, frag_index and each
 * out_chain column may be NULL (out_chain itself too).
 * out_chain: a FITS output gets the source's rows j < min(n_hdrs, PKT_MAX_HDRS) and that n_hdrs; a fragment gets the
 * rows up to and including the IP entry (index e), n_hdrs = e + 1: the bytes before the IP header are copied
 * verbatim, so the offsets hold, and the entries after it describe bytes a fragment may not have.  Later rows are not
 * written.  pkt_fwd_batch, pkt_flow_key_batch (fragments key without ports), pkt_lpm_lookup_batch and pkt_pcap_write
 * take the result with no second parse.
 * Overflow: if *n_out > out_cap, *n_out >= 2^32 or *bytes_out_total > dst_len, the call (or pkt_frag_result) returns
 * PKT_ERR_INVALID_ARG with both totals set: the capacity to retry with.  The decision is taken on the device, as in
 * pkt_pcap_write, and the writing kernels exit: dst and the per-output arrays (and first) are unspecified, but nothing
 * outside their capacities is written; status / nfrag / hits stay valid.  With PKT_FRAG_NO_WRITE dst, out_cap and the
 * per-output arrays are ignored and may be NULL / 0: only status, nfrag, first, hits and the totals are produced.  That
 * is the sizing pass, and it never overflows (first is meaningful while *n_out < 2^32).
 * hits: device uint64_t[PKT_FRAG_STATUS_COUNT], 8-byte aligned, ADDED to as pkt_fwd_batch's is; exact, every call adds
 * exactly n.  status, nfrag, first and hits may each be NULL.
 *  - PKT_ERR_INVALID_ARG before any launch, with a text starting "pkt_frag" in pkt_ctx_last_error:
 *    pkt_flow_key_batch's batch and slab rules; a NULL chain, or a NULL chain column with n > 0; n >= 2^32; a bad
 *    which_ip; unknown flag bits; mtu_all > 65535; a misaligned dst (16), hits (8), out_off (8) or mtu (2); without
 *    PKT_FRAG_NO_WRITE a NULL dst, out_off or out_len, or out_cap == 0 or >= 2^32; a second call on the ctx before
 *    pkt_frag_result (the one-in-flight rule of pkt_pcap_write_async).  n == 0 succeeds with both totals 0 and
 *    writes the empty tail.
 *  - pkt_frag_batch waits for the two totals (one host wait); pkt_frag_batch_async queues the same kernels and
 *    pkt_frag_result takes the totals and the overflow verdict.  Scratch lives in the ctx and grows on demand.
 *  - On the device: a decision kernel (a lane owns a source packet; per tile of 256 the outputs and rounded bytes;
 *    per-status counts merged per block in LDS), a one-block scan that also decides the overflow, an emit kernel (a
 *    packet's rows are closed-form from per and P; a wave spreads the rows of its 64 packets over its lanes, so a
 *    packet of 8190 fragments costs its rows, not a loop in one lane) and a copy kernel (a wave walks 64 outputs'
 *    16-byte chunks together; each chunk is built in registers from the aligned source chunks that hold its bytes and
 *    stored whole).  No lane waits for another; no global atomics but the hits adds.
 * pkt_frag_host is the same operation on HOST pointers: no ctx, no device; the slab's and dst's alignment rules hold
 * for dst, hits, out_off and mtu and are waived for the slab.
 * Out of scope: ICMP fragmentation-needed / packet-too-big generation (pkt_icmp_err_batch, below: PKT_FRAG_DF and
 * PKT_FRAG_IPV6 are its inputs);
 * reassembly (pkt_reasm_batch, below); IPv4 options.  With which_ip on an inner header the outer tunnel's length fields
 * are left as they are: to send tunnelled packets over a smaller MTU, fragment the inner packets first and encapsulate
 * the fragments, or encapsulate first and fragment the OUTER datagram (pkt_tunnel_encap_batch, below, sets its lengths). */
typedef enum pkt_frag_status {
    PKT_FRAG_FITS    = 0, /* one output: the packet, whole */
    PKT_FRAG_SPLIT   = 1, /* nfrag >= 2 outputs */
    PKT_FRAG_SKIPPED = 2, /* select[i] == 0 */
    PKT_FRAG_NO_IP   = 3, /* the chain has no such IPv4 / IPv6 entry */
    PKT_FRAG_SPAN    = 4, /* the IP entry's 20 / 40 bytes are not inside the packet */
    PKT_FRAG_IPV6    = 5, /* an IPv6 packet above the mtu: routers do not fragment it */
    PKT_FRAG_BAD_HDR = 6, /* byte 0 != 0x45, total length < 20, or the last fragment's offset would not fit 13 bits */
    PKT_FRAG_TRUNC   = 7, /* the datagram's total length does not lie inside the packet */
    PKT_FRAG_DF      = 8, /* don't-fragment is set */
    PKT_FRAG_MTU     = 9  /* mtu < 28: not even 8 payload bytes fit */
} pkt_frag_status_t;
#define PKT_FRAG_STATUS_COUNT 10
#define PKT_FRAG_ONLY_SPLIT 1u          /* flags: a FITS packet gives no output */
#define PKT_FRAG_NO_WRITE   2u          /* flags: decide and total everything, store no packet byte and no per-output array */
#define PKT_FRAG_NONE       0xFFFFFFFFu /* first[i] / src_index[q] when there is none */
int pkt_frag_batch(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                   uint32_t flags, const uint16_t *mtu, uint32_t mtu_all, const uint8_t *select,
                   uint8_t *status, uint32_t *nfrag, uint32_t *first,
                   uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                   uint64_t *out_off, uint32_t *out_len, uint32_t *src_index, uint16_t *frag_index,
                   const pkt_chain_t *out_chain,
                   uint64_t *hits, uint64_t *bytes_out_total, uint64_t *n_out, void *stream);
int pkt_frag_batch_async(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                         uint32_t flags, const uint16_t *mtu, uint32_t mtu_all, const uint8_t *select,
                         uint8_t *status, uint32_t *nfrag, uint32_t *first,
                         uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                         uint64_t *out_off, uint32_t *out_len, uint32_t *src_index, uint16_t *frag_index,
                         const pkt_chain_t *out_chain, uint64_t *hits, void *stream);
int pkt_frag_result(pkt_ctx_t *ctx, uint64_t *bytes_out_total, uint64_t *n_out);
int pkt_frag_host(const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                  uint32_t flags, const uint16_t *mtu, uint32_t mtu_all, const uint8_t *select,
                  uint8_t *status, uint32_t *nfrag, uint32_t *first,
                  uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                  uint64_t *out_off, uint32_t *out_len, uint32_t *src_index, uint16_t *frag_index,
                  const pkt_chain_t *out_chain,
                  uint64_t *hits, uint64_t *bytes_out_total, uint64_t *n_out);

/* ---- IPv4 reassembly of a batch's fragments ----
 * The inverse of pkt_frag_batch: the fragments of a batch (or of a stream window) are grouped by datagram and joined
 * into whole packets in a second slab, which is an indexed batch again: pkt_parse_batch, pkt_l4_checksum_batch,
 * pkt_flow_key_batch, pkt_match_batch and pkt_pcap_write take it.  The reference defines nothing here, so this header
 * fixes the semantics; they follow RFC 791's reassembly, with overlaps refused rather than merged (as RFC 5722 does
 * for IPv6 and Linux does for IPv4).
 *
 * pkt_reasm_batch, per source packet i: the first test that applies gives status[i].
 *  1. select != NULL && select[i] == 0: PKT_REASM_SKIPPED.
 *  2. The IP entry is found exactly as in pkt_frag_batch step 2 (which_ip, PKT_FLOW_LAST included, over min(n_hdrs,
 *     PKT_MAX_HDRS) entries; a which_ip in 16..0xFE is refused).  No such entry: PKT_REASM_NO_IP.  Its 20 / 40 bytes
 *     not inside the packet's length (under the pkt_batch_t clamp rules): PKT_REASM_SPAN.
 *  3. The entry is IPv6, or IPv4 with (bytes 6..7 & 0x3FFF) == 0 (pkt_l4_checksum_batch's fragment test):
 *     PKT_REASM_WHOLE, with no other header check.  (The IPv6 fragment extension header is out of scope.)
 *  4. It is an IPv4 fragment.  L = bytes 2..3, w = bytes 6..7 (big-endian), s = 8 * (w & 0x1FFF), len = L - 20,
 *     e = s + len.  Byte 0 != 0x45, or L <= 20 (an empty fragment), or MF (w & 0x2000) set and len % 8 != 0:
 *     PKT_REASM_BAD_HDR.
 *  5. ip_off + L > the packet's length: PKT_REASM_TRUNC.
 *  6. Otherwise the packet is a MEMBER of the datagram with the key (src, dst, protocol, identification) = (bytes
 *     12..15, 16..19, 9, 4..5).  Nothing else belongs to the key: VLAN tags, outer headers and ip_off may differ
 *     between members.  Every member of a datagram gets the datagram's verdict.
 * The verdict of a datagram is defined on the set of its members in this batch, whatever their order:
 *  - PKT_REASM_JOINED iff exactly one member has MF clear, and the members, sorted by s and each used exactly once,
 *    tile [0, E): s_0 = 0, s_(k+1) = e_k, and the last in that order is the MF-clear member, with e = E;
 *  - PKT_REASM_TOO_BIG if that tiling holds but 20 + E > 65535;
 *  - PKT_REASM_PENDING otherwise: a hole, a duplicate, any overlap, two final fragments, a fragment past the end.
 * A SKIPPED, BAD_HDR or TRUNC packet is not a member; its datagram is then usually PENDING.
 * Outputs: WHOLE gives one output, the packet's bytes [0, len_i) verbatim as PKT_FRAG_FITS does (none with
 * PKT_REASM_ONLY_JOINED).  A JOINED datagram gives one output, owned by its member with the LARGEST source index: a
 * reassembler emits a datagram when its last fragment arrives, so the output keeps its causal place among the whole
 * packets.  Every other status gives none.  Outputs are ordered by owner index.  out_index[i] is the output that
 * carries packet i's bytes, the same value for every member of a datagram, PKT_REASM_NONE where there is none.
 * src_index[q] is the owner, nfrag[q] the number of source packets in output q (1 for WHOLE).  The result is exact and
 * byte-identical from run to run.
 * A joined output is
 *  - bytes [0, ip_off0 + 20) of the member with s = 0 (ip_off0: its ip_off), where bytes 2..3 of the IP header = 20 + E,
 *    bytes 6..7 = w0 & 0xC000, and bytes 10..11 are updated incrementally over those two words (RFC 1624 eq. 3, folded
 *    twice, exactly as pkt_frag_batch's fragment header: a checksum that was wrong stays wrong by the same amount);
 *  - then every member's payload, its own bytes [ip_off_m + 20, ip_off_m + L_m), at ip_off0 + 20 + s_m.
 * Source bytes past a member's ip_off + L go nowhere.  When which_ip selects an inner header the outer headers' length
 * fields are NOT corrected (pkt_frag_batch's caveat): reassemble the outer fragments, then pkt_tunnel_decap_batch.
 * Layout of dst, out_off / out_len, the 16-byte rounding with zero fill, the empty tail up to out_cap (out_off 0,
 * out_len 0, src_index PKT_REASM_NONE, nfrag 0, out_chain->n_hdrs 0), *bytes_out_total, *n_out, hits (device
 * uint64_t[PKT_REASM_STATUS_COUNT], ADDED to, exactly n per call), the overflow return (PKT_ERR_INVALID_ARG with both
 * totals, decided on the device; out_index is then unspecified too) and PKT_REASM_NO_WRITE as the sizing pass (only
 * status, out_index, hits and the totals) are pkt_frag_batch's.  status, out_index, src_index, nfrag, hits, out_chain
 * and each of its columns may be NULL.
 * out_chain: a WHOLE output gets the source's rows j < min(n_hdrs, PKT_MAX_HDRS) and that n_hdrs; a joined output gets
 * the s = 0 member's rows up to and including the IP entry (index e), n_hdrs = e + 1, as a fragment gets from
 * pkt_frag_batch.  The L4 header of a joined datagram is not walked here: pkt_parse_batch over the output batch gives
 * the full chain, now correctly.
 *  - PKT_ERR_INVALID_ARG before any launch, with a text starting "pkt_reasm" in pkt_ctx_last_error: pkt_frag_batch's
 *    refusals without the mtu ones; a second call on the ctx before pkt_reasm_result (the one-in-flight rule).
 *    n == 0 succeeds with both totals 0 and writes the empty tail.
 *  - pkt_reasm_batch waits for the two totals (one host wait); pkt_reasm_batch_async queues the same kernels and
 *    pkt_reasm_result takes the totals and the overflow verdict.  Scratch lives in the ctx and grows on demand.
 *  - On the device the cost is linear in n: classify (a lane owns a source packet), group (an open-addressed table of
 *    >= 2 n slots; one compare-and-swap per probed slot, adds and a max into the datagram's words, and the fragment
 *    start put into a second table used as a set), link (every MF-set member looks its end up in that set; a miss is a
 *    hole), count, a one-block scan that also decides the overflow, emit, and a source-driven copy.  No lane waits for
 *    another; the only loops over shared state are probe sequences bounded by the slot count; no atomics on packet
 *    bytes, and every destination byte is written exactly once.
 * pkt_reasm_host is the same operation on HOST pointers: no ctx, no device; the alignment rules hold for dst, hits and
 * out_off and are waived for the slab.
 * Out of scope: state across batches and timeouts (status == PKT_REASM_PENDING is the mask to carry fragments over
 * with, through pkt_reorder_batch or `select`); IPv6 fragment headers; IPv4 options; merging overlaps. */
typedef enum pkt_reasm_status {
    PKT_REASM_WHOLE   = 0, /* not a fragment: one output, the packet, whole */
    PKT_REASM_JOINED  = 1, /* a member of a datagram that is complete in this batch */
    PKT_REASM_PENDING = 2, /* a member of a datagram that is not (a hole, a duplicate, an overlap, two finals) */
    PKT_REASM_SKIPPED = 3, /* select[i] == 0 */
    PKT_REASM_NO_IP   = 4, /* the chain has no such IPv4 / IPv6 entry */
    PKT_REASM_SPAN    = 5, /* the IP entry's 20 / 40 bytes are not inside the packet */
    PKT_REASM_BAD_HDR = 6, /* a fragment with byte 0 != 0x45, no payload, or MF and a length that is no multiple of 8 */
    PKT_REASM_TRUNC   = 7, /* the fragment's total length does not lie inside the packet */
    PKT_REASM_TOO_BIG = 8  /* the members tile a datagram of more than 65535 bytes */
} pkt_reasm_status_t;
#define PKT_REASM_STATUS_COUNT 9
#define PKT_REASM_ONLY_JOINED 1u          /* flags: a WHOLE packet gives no output */
#define PKT_REASM_NO_WRITE    2u          /* flags: decide and total everything, store no packet byte and no per-output array */
#define PKT_REASM_NONE        0xFFFFFFFFu /* out_index[i] / src_index[q] when there is none */
int pkt_reasm_batch(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                    uint32_t flags, const uint8_t *select, uint8_t *status, uint32_t *out_index,
                    uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                    uint64_t *out_off, uint32_t *out_len, uint32_t *src_index, uint32_t *nfrag,
                    const pkt_chain_t *out_chain,
                    uint64_t *hits, uint64_t *bytes_out_total, uint64_t *n_out, void *stream);
int pkt_reasm_batch_async(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                          uint32_t flags, const uint8_t *select, uint8_t *status, uint32_t *out_index,
                          uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                          uint64_t *out_off, uint32_t *out_len, uint32_t *src_index, uint32_t *nfrag,
                          const pkt_chain_t *out_chain, uint64_t *hits, void *stream);
int pkt_reasm_result(pkt_ctx_t *ctx, uint64_t *bytes_out_total, uint64_t *n_out);
int pkt_reasm_host(const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                   uint32_t flags, const uint8_t *select, uint8_t *status, uint32_t *out_index,
                   uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                   uint64_t *out_off, uint32_t *out_len, uint32_t *src_index, uint32_t *nfrag,
                   const pkt_chain_t *out_chain,
                   uint64_t *hits, uint64_t *bytes_out_total, uint64_t *n_out);

/* ---- pkt_scan_*: multi-pattern byte search over a batch's payloads.  Every call above looks at headers; this one
 * answers whether a packet's bytes contain one of a set of byte strings (signature prefilters, protocol
 * identification by banner).  The reference defines nothing here, so this header fixes the semantics.  A pattern
 * set is up to PKT_SCAN_MAX_PATTERNS byte strings of 1..PKT_SCAN_MAX_LEN bytes, PKT_SCAN_MAX_BYTES in all; it is
 * compiled and uploaded once (pkt_scan_create) and searched by one kernel in a single pass over the packets' bytes.
 *  - The region [r0, r1) of packet i: r1 is the packet's length under the pkt_batch_t clamp rules.
 *    PKT_SCAN_PACKET: r0 = 0, and `chain` may be NULL.  PKT_SCAN_PAYLOAD: r0 is the first byte after every header of
 *    the list, the MAXIMUM over j < min(n_hdrs, PKT_MAX_HDRS) of hdr_off[j] + pkt_hdr_size(hdr_type[j]) (not the
 *    last entry: quirk Q2 puts a wire-earlier GRE option last); on a parse's chain that is its payload_off.
 *    n_hdrs == 0: PKT_SCAN_NO_CHAIN.  A hdr_type outside 1..21, or r0 > r1: PKT_SCAN_SPAN.  r0 == r1 is a scanned
 *    packet with no occurrence.
 *  - An occurrence is a pair (p, s) with r0 <= s, s + len_p <= r1 and every pattern byte equal to the packet's
 *    byte at its place; under PKT_SCAN_NOCASE both bytes are folded first (0x41..0x5A to 0x61..0x7A, nothing else
 *    changes).  Occurrences overlap in any way; identical patterns each count; a prefix of another pattern counts
 *    at the same s.  No byte outside [r0, r1) ever contributes: a string that straddles two packets of a packed
 *    slab is no occurrence.
 *  - Outputs, device [n] arrays, each may be NULL.  count[i]: the occurrences.  pat[i]: the lowest pattern index
 *    with one, else PKT_SCAN_NONE.  off[i]: the smallest s of that pattern, from the packet's first byte (the
 *    hdr_off convention), else 0.  matched[i]: bit g set iff a pattern of group g occurs.  action[i]: pattern
 *    pat[i]'s action; default_action for a scanned packet with no occurrence and for NO_CHAIN and SPAN; 0 for
 *    SKIPPED.  sel[i] = action[i] != 0 (the mask pkt_pcap_write and pkt_edit_batch take).  status[i]: HIT iff
 *    count[i] > 0, MISS for a scanned packet without one.  select[i] == 0 gives SKIPPED.  A packet that is not
 *    scanned has count 0, pat NONE, off 0, matched 0.
 *  - hits: a device uint64_t[npats + 1], 8-byte aligned, caller-owned, ADDED to as pkt_match_batch's counters are:
 *    hits[p] gains pattern p's occurrences, hits[npats] the number of MISS packets.  Exact: a call adds sum(count)
 *    to hits[0..npats).  With every output NULL, or n == 0, the call succeeds, launches nothing and leaves the
 *    counters untouched.
 *  - pkt_scan_create validates, compiles on the host and uploads; blocking, and the only allocation (the
 *    pkt_match_create pattern).  `bytes` and `pats` are HOST memory, captured at the call.  PKT_ERR_INVALID_ARG
 *    with a text starting "pkt_scan" in pkt_ctx_last_error: npats > PKT_SCAN_MAX_PATTERNS, the lengths' sum >
 *    PKT_SCAN_MAX_BYTES, a len of 0 or above PKT_SCAN_MAX_LEN, off + len > nbytes, an unknown flag bit, a group
 *    above 63, a non-zero reserved, a NULL pointer with a non-zero count.  npats == 0 is legal: every scanned
 *    packet is a MISS.  pkt_scan_info: what was built.  nstates: the states of the two tries (below), their roots
 *    included.  table_bytes: the compiled image.  placement: PKT_SCAN_PLACE_GLOBAL (the first-level filter in LDS,
 *    the deeper levels in device memory) or PKT_SCAN_PLACE_LDS (the whole automaton in LDS: sets whose deeper
 *    levels fit the kernel's budget); a host handle reports PKT_SCAN_PLACE_GLOBAL.
 *  - pkt_scan_batch is asynchronous on `stream`, keeps no per-call state in the handle and never writes the compiled
 *    set: several calls on one handle may be in flight on different streams.  PKT_ERR_INVALID_ARG before any launch,
 *    with a text starting "pkt_scan_batch" in pkt_scan_last_error: the batch and slab rules with their texts; a NULL
 *    chain, or with n > 0 a NULL chain column, when region is PAYLOAD; an unknown region; n >= 2^32; matched or
 *    hits not 8-byte aligned.  pkt_scan_destroy is the caller's to order after the calls in flight.
 *  - The compiled set: two failureless tries (exact patterns; NOCASE patterns, folded, walked over folded bytes),
 *    so mixing the two kinds never multiplies states.  A start position walks the patterns that begin there and
 *    stops at the first byte none continues with.  Level 1 is a 256-entry table per trie and a bitmap over the first
 *    two (folded) bytes; deeper edges sit in one open-addressed table keyed by (state, byte).  The kernel reads
 *    whole aligned 16-byte chunks only: at most 15 bytes past a packet's end, never past round_up(slab + slab_len,
 *    16).  Per-packet results are add / min / or reductions in LDS: identical from run to run.
 * pkt_scan_create_host gives the same handle type on HOST memory (the pkt_lpm_create_host pattern): pkt_scan_batch
 * then takes host pointers, ignores `stream`, and waives the slab's alignment.  Its create refusals' text:
 * pkt_scan_last_error(NULL).
 * Out of scope: regular expressions; patterns above 64 bytes; a per-occurrence event list; matches across packets
 * (pkt_reasm_batch first, then scan). */
#define PKT_SCAN_MAX_PATTERNS 8192
#define PKT_SCAN_MAX_LEN      64          /* bytes per pattern, 1..64 */
#define PKT_SCAN_MAX_BYTES    131072      /* sum of the patterns' lengths */
#define PKT_SCAN_NONE         0xFFFFFFFFu /* pat[i] when nothing occurs */
#define PKT_SCAN_NOCASE       1u          /* pattern flag: compare ASCII letters without case */
enum { PKT_SCAN_PACKET = 0, PKT_SCAN_PAYLOAD = 1 };                                  /* region */
enum { PKT_SCAN_MISS = 0, PKT_SCAN_HIT = 1, PKT_SCAN_SKIPPED = 2, PKT_SCAN_NO_CHAIN = 3, PKT_SCAN_SPAN = 4 }; /* status */
enum { PKT_SCAN_PLACE_GLOBAL = 0, PKT_SCAN_PLACE_LDS = 1 };                          /* pkt_scan_info_t.placement */
typedef struct pkt_scan_pattern {      /* 16 bytes */
    uint32_t off;                      /* the pattern is bytes[off, off + len) of the blob given to create */
    uint16_t len;                      /* 1..PKT_SCAN_MAX_LEN */
    uint8_t  flags;                    /* PKT_SCAN_NOCASE or 0 */
    uint8_t  group;                    /* 0..63: the bit of `matched` this pattern sets */
    uint32_t action;                   /* caller-defined; 0 means "not selected" */
    uint32_t reserved;                 /* 0 */
} pkt_scan_pattern_t;
typedef struct pkt_scan_info {         /* 24 bytes */
    uint32_t npatterns;
    uint32_t nstates;                  /* of both tries, their roots included */
    uint32_t max_len;                  /* the longest pattern */
    uint32_t placement;                /* PKT_SCAN_PLACE_* */
    uint64_t table_bytes;              /* the compiled image */
} pkt_scan_info_t;
typedef struct pkt_scan pkt_scan_t;
size_t pkt_sizeof_scan_pattern(void);
int pkt_scan_create(pkt_ctx_t *ctx, const uint8_t *bytes, uint64_t nbytes, const pkt_scan_pattern_t *pats,
                    uint32_t npats, uint32_t default_action, pkt_scan_t **s);
int pkt_scan_create_host(const uint8_t *bytes, uint64_t nbytes, const pkt_scan_pattern_t *pats,
                         uint32_t npats, uint32_t default_action, pkt_scan_t **s);
int pkt_scan_info(const pkt_scan_t *s, pkt_scan_info_t *info);
int pkt_scan_batch(pkt_scan_t *s, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t region,
                   const uint8_t *select, uint8_t *status, uint32_t *pat, uint16_t *off, uint32_t *action,
                   uint8_t *sel, uint32_t *count, uint64_t *matched, uint64_t *hits, void *stream);
int pkt_scan_destroy(pkt_scan_t *s);
const char *pkt_scan_last_error(const pkt_scan_t *s);

/* ---- ICMP errors for the packets a router refuses ----
 * What a router answers to the packets pkt_fwd_batch leaves at PKT_FWD_TTL / _MTU / _NO_ADJ and pkt_frag_batch at
 * PKT_FRAG_DF / _IPV6: for every source packet that may be answered one ICMP (IPv4) or ICMPv6 (IPv6) error packet,
 * packed into a second slab exactly as pkt_frag_batch packs its outputs, with the chain columns the following calls
 * need.  The reference defines nothing here, so this header fixes the semantics; they follow RFC 792, RFC 1191,
 * RFC 1122 3.2.2, RFC 1812 4.3.2 and RFC 4443 2.4.
 *
 * The code.  Packet i's code is c = code ? code[i] : code_all (code_all > 255 is refused), its reason r = map ?
 * map[c] : c.  `map` is a HOST array of 256 bytes that goes along with the launch (it need not outlive the call), so
 * pkt_fwd_batch's or pkt_frag_batch's device status array is `code` as it is, with no pass in between.  A reason
 * (pkt_icmp_reason_t) gives a (type, code) pair per IP version:
 *    reason          IPv4      IPv6
 *    TIME_EXCEEDED   11, 0     3, 0
 *    TOO_BIG          3, 4     2, 0     the next-hop mtu m = mtu ? mtu[i] : mtu_all goes into bytes 6..7 of the ICMP
 *    NET_UNREACH      3, 0     1, 0     header under IPv4 (RFC 1191) and bytes 4..7 under IPv6
 *    HOST_UNREACH     3, 1     1, 3
 *    PROHIBITED       3, 13    1, 1
 *    PORT_UNREACH     3, 3     1, 4
 *
 * pkt_icmp_err_batch, per source packet i: the first test that applies gives status[i].
 *  1. select != NULL && select[i] == 0, or r == 0: PKT_ICMPE_SKIPPED.
 *  2. r > 6: PKT_ICMPE_BAD_REASON.
 *  3. The IP entry is found exactly as in pkt_frag_batch step 2 (which_ip, PKT_FLOW_LAST included, over min(n_hdrs,
 *     PKT_MAX_HDRS) entries).  No such entry: PKT_ICMPE_NO_IP.  Its H = 20 / 40 bytes not inside the packet's length
 *     (under the pkt_batch_t clamp rules): PKT_ICMPE_SPAN.
 *  4. The Ether entry with the greatest index below the IP entry (pkt_fwd_batch's rule).  None: PKT_ICMPE_NO_ETHER.
 *     eth_off + 14 > ip_off (only a forged chain gives that): PKT_ICMPE_SPAN.  P = ip_off - eth_off.
 *  5. The cfg's source address for this IP version is all zero: PKT_ICMPE_NO_SRC.
 *  6. IPv4: byte 0 != 0x45, or L = bytes 2..3 < 20 (IPv4 options are out of scope, as in pkt_frag_batch); IPv6:
 *     byte 0 >> 4 != 6: PKT_ICMPE_BAD_HDR.
 *  7. IPv4 with (bytes 6..7 & 0x1FFF) != 0, a non-first fragment (RFC 1122 3.2.2): PKT_ICMPE_FRAGMENT.  A first
 *     fragment (MF set, offset 0) is answered.
 *  8. The packet's source address names no single host: IPv4 with first byte 0, 127 or >= 224; IPv6 all zero or with
 *     first byte 0xFF: PKT_ICMPE_BAD_SRC.
 *  9. The Ether destination's byte 0 has bit 0 set, or the IPv4 destination's first byte is >= 224, or the IPv6
 *     destination's first byte is 0xFF: PKT_ICMPE_MCAST.  The step does not apply to IPv6 with r == TOO_BIG (RFC 4443
 *     2.4 e.3).
 * 10. The packet is itself an ICMP error: PKT_ICMPE_ICMP_ERR.  IPv4 with protocol byte 1: the type byte at ip_off +
 *     20 lies outside min(len, ip_off + L), or it is one of 3, 4, 5, 11, 12.  IPv6 with next header 58: the type byte
 *     at ip_off + 40 lies outside min(len, ip_off + 40 + bytes 4..5), or it is < 128 or == 137.
 * 11. PKT_ICMPE_SENT: one output.
 * The output of a SENT packet, out_len = P + H + 8 + Q bytes (not padded to 60):
 *  - bytes [0, P): the source's [eth_off, ip_off) verbatim (VLAN tags, MPLS labels and all) with the two MAC
 *    addresses swapped: the reply leaves by the link it came in on, and pkt_fwd_batch over the output re-routes it if
 *    the caller wants that.  Outer tunnel headers before eth_off are NOT carried: an error for a VXLAN inner packet
 *    is a bare inner frame, for pkt_edit_batch to encapsulate;
 *  - IPv4 header: 45 tos, total length 28 + Q, identification (ident + q) & 0xFFFF with q the output's index, bytes
 *    6..7 zero, ttl, protocol 1, the RFC 1071 header checksum (the correct fold, not Packet::ipv4_checksum's), src4,
 *    the source packet's source address;
 *  - IPv6 header: version 6, traffic class tos, flow label 0, payload length 8 + Q, next header 58, hop limit ttl,
 *    src6, the source packet's source address;
 *  - ICMP header, 8 bytes: type, code, checksum, and four bytes that are zero but for TOO_BIG's mtu;
 *  - the quote: the source bytes [ip_off, ip_off + Q) verbatim (pkt_fwd_batch does not write a packet it refuses, so
 *    the ttl is as received).  Q = min(avail, max - H - 8), max = max4 / max6; avail = min(L, len - ip_off) under
 *    IPv4 and min(40 + bytes 4..5, len - ip_off) under IPv6: Ethernet padding is never quoted, and a truncated
 *    capture record is quoted as far as it goes;
 *  - the ICMP checksum: RFC 1071 over the ICMP message, under IPv6 with the pseudo-header (src, dst, the 32-bit
 *    length 8 + Q, next header 58); a computed 0 is stored as 0xFFFF under IPv6 and as 0 under IPv4, exactly the
 *    encodings pkt_l4_checksum_batch calls PKT_L4_OK.
 * Outputs are in source order, exact and the same from run to run.  Per source packet: status[i] and out_index[i],
 * the packet's output or PKT_ICMPE_NONE.  Per output q: out_off, out_len, src_index and out_chain; dst, out_off, the
 * layout rule (out_off[q + 1] = out_off[q] + round_up(out_len[q], 16), the rounded tail zeros), the empty tail
 * [*n_out, out_cap) (out_off 0, out_len 0, src_index PKT_ICMPE_NONE, out_chain->n_hdrs 0), PKT_ICMPE_NO_WRITE (the
 * sizing pass: only status, out_index, hits and the totals), the overflow return with both totals set and decided on
 * the device, and _async / _result with one call in flight per ctx are pkt_frag_batch's, word for word.  status,
 * out_index, src_index, hits, out_chain and each of its columns may be NULL.
 * out_chain: rows 0..(e_ip - e_eth) are the source's rows e_eth..e_ip (the Ether and the IP entry's indices) with
 * hdr_off - eth_off, then one row (PKT_HDR_ICMP, P + H); n_hdrs = min(e_ip - e_eth + 2, PKT_MAX_HDRS), and the ICMP row
 * is written only if its index is below PKT_MAX_HDRS.  pkt_l4_checksum_batch, pkt_flow_key_batch,
 * pkt_lpm_lookup_batch, pkt_fwd_batch (which routes the replies), pkt_dispatch_batch and pkt_pcap_write take the
 * result with no second parse.
 * hits: device uint64_t[PKT_ICMPE_STATUS_COUNT], 8-byte aligned, ADDED to; exact, every call adds exactly n.
 *  - PKT_ERR_INVALID_ARG before any launch, with a text starting "pkt_icmp_err" in pkt_ctx_last_error:
 *    pkt_frag_batch's batch, slab, chain, which_ip, flag, alignment (dst 16, hits 8, out_off 8, mtu 2) and capacity
 *    rules; a NULL cfg; a cfg with both addresses zero; max4 not 0 and below 56, max6 not 0 and below 96; code_all >
 *    255; mtu_all > 65535; a second call on the ctx before pkt_icmp_err_result.  n == 0 succeeds with both totals 0
 *    and writes the empty tail.
 *  - Scratch lives in the ctx and grows on demand.
 *  - On the device, three launches: a decision kernel (a lane owns a source packet: the chain, the header bytes the
 *    tests need by the aligned 16-byte chunks that hold them, a 32-byte plan; per tile of 256 the outputs and rounded
 *    bytes; per-status counts merged per block in LDS), a one-block scan that also decides the overflow, and a build
 *    kernel (a wave walks the 16-byte chunks of its 64 sources' outputs together; each chunk is built in registers
 *    from the swapped prefix, the header words and the two aligned source chunks that hold its quote bytes, and
 *    stored whole; the quote's 16-bit words are summed chunk by chunk into the output's LDS word, and the chunks that
 *    hold the ICMP checksum are stored once the wave's sums are complete).  No lane waits for another; no global
 *    atomics but the hits adds.
 * pkt_icmp_err_host is the same operation on HOST pointers: no ctx, no device; the alignment rules hold for dst,
 * hits, out_off and mtu and are waived for the slab.
 * Out of scope: rate limiting (RFC 1812 4.3.2.8: the caller's `select`); per-interface source addresses; redirects,
 * parameter problem, echo replies; IPv4 options and IPv6 extension headers; directed-broadcast destinations. */
typedef struct pkt_icmp_cfg {      /* 28 bytes */
    uint8_t  src4[4];              /* the router's IPv4 address, wire bytes; all zero = no IPv4 errors are sent */
    uint8_t  src6[16];             /* the same for IPv6 */
    uint16_t max4;                 /* greatest IPv4 datagram built (IP header on), 0 = 576 (RFC 1812 4.3.2.3); else 56..65535 */
    uint16_t max6;                 /* greatest IPv6 packet built, 0 = 1280 (RFC 4443 2.4 c); else 96..65535 */
    uint16_t ident;                /* IPv4 identification of output q is (ident + q) & 0xFFFF */
    uint8_t  ttl;                  /* ttl / hop limit of the outputs, 0 = 64 */
    uint8_t  tos;                  /* tos / traffic class of the outputs */
} pkt_icmp_cfg_t;
typedef enum pkt_icmp_reason {
    PKT_ICMP_R_NONE          = 0,  /* no answer: PKT_ICMPE_SKIPPED */
    PKT_ICMP_R_TIME_EXCEEDED = 1,
    PKT_ICMP_R_TOO_BIG       = 2,
    PKT_ICMP_R_NET_UNREACH   = 3,
    PKT_ICMP_R_HOST_UNREACH  = 4,
    PKT_ICMP_R_PROHIBITED    = 5,
    PKT_ICMP_R_PORT_UNREACH  = 6
} pkt_icmp_reason_t;
typedef enum pkt_icmpe_status {
    PKT_ICMPE_SENT       = 0,  /* one output */
    PKT_ICMPE_SKIPPED    = 1,  /* select[i] == 0, or reason 0 */
    PKT_ICMPE_BAD_REASON = 2,  /* reason above 6 */
    PKT_ICMPE_NO_IP      = 3,  /* the chain has no such IPv4 / IPv6 entry */
    PKT_ICMPE_SPAN       = 4,  /* the IP entry's bytes are not inside the packet, or the Ether entry runs into it */
    PKT_ICMPE_NO_ETHER   = 5,  /* no Ether entry before the IP entry */
    PKT_ICMPE_NO_SRC     = 6,  /* the cfg has no source address for this IP version */
    PKT_ICMPE_BAD_HDR    = 7,  /* IPv4 byte 0 != 0x45 or total length < 20; IPv6 version != 6 */
    PKT_ICMPE_FRAGMENT   = 8,  /* a non-first IPv4 fragment */
    PKT_ICMPE_BAD_SRC    = 9,  /* the source address names no single host */
    PKT_ICMPE_MCAST      = 10, /* sent to a link-layer or IP multicast / broadcast destination */
    PKT_ICMPE_ICMP_ERR   = 11  /* the packet is itself an ICMP error */
} pkt_icmpe_status_t;
#define PKT_ICMPE_STATUS_COUNT 12
#define PKT_ICMPE_NO_WRITE 1u          /* flags: decide and total everything, store no packet byte and no per-output array */
#define PKT_ICMPE_NONE     0xFFFFFFFFu /* out_index[i] / src_index[q] when there is none */
size_t pkt_sizeof_icmp_cfg(void);
int pkt_icmp_err_batch(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                       uint32_t flags, const pkt_icmp_cfg_t *cfg, const uint8_t *code, uint32_t code_all,
                       const uint8_t *map, const uint16_t *mtu, uint32_t mtu_all, const uint8_t *select,
                       uint8_t *status, uint32_t *out_index,
                       uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                       uint64_t *out_off, uint32_t *out_len, uint32_t *src_index,
                       const pkt_chain_t *out_chain,
                       uint64_t *hits, uint64_t *bytes_out_total, uint64_t *n_out, void *stream);
int pkt_icmp_err_batch_async(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                             uint32_t flags, const pkt_icmp_cfg_t *cfg, const uint8_t *code, uint32_t code_all,
                             const uint8_t *map, const uint16_t *mtu, uint32_t mtu_all, const uint8_t *select,
                             uint8_t *status, uint32_t *out_index,
                             uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                             uint64_t *out_off, uint32_t *out_len, uint32_t *src_index,
                             const pkt_chain_t *out_chain, uint64_t *hits, void *stream);
int pkt_icmp_err_result(pkt_ctx_t *ctx, uint64_t *bytes_out_total, uint64_t *n_out);
int pkt_icmp_err_host(const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                      uint32_t flags, const pkt_icmp_cfg_t *cfg, const uint8_t *code, uint32_t code_all,
                      const uint8_t *map, const uint16_t *mtu, uint32_t mtu_all, const uint8_t *select,
                      uint8_t *status, uint32_t *out_index,
                      uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                      uint64_t *out_off, uint32_t *out_len, uint32_t *src_index,
                      const pkt_chain_t *out_chain,
                      uint64_t *hits, uint64_t *bytes_out_total, uint64_t *n_out);

/* ---- pkt_nat_*: NAPT44 sessions and translation over a parsed batch ----
 * The step of an edge router between "parsed" and "routed": keep the sessions, allocate the outside ports, rewrite
 * addresses and ports in place and update the IPv4 and TCP / UDP / ICMP checksums incrementally.  The reference defines
 * nothing here, so this header fixes the semantics.
 *
 * Scope: NAT44 with port translation for TCP, UDP and ICMP echo (the echo identifier plays the port).  Mapping and
 * filtering are endpoint-independent (RFC 4787 REQ-1): a session is (proto, inside addr, inside port) <-> (proto,
 * outside addr, outside port), whatever the remote end.  Protocol indexes: p = 0 TCP (6), 1 UDP (17), 2 ICMP (1).
 *
 * pkt_nat_create: blocking, and the only allocating call.  pool: naddr (1..64) outside IPv4 addresses, 4 wire bytes
 * each, distinct.  The dynamic ports are port_lo..port_hi (1 <= lo <= hi <= 65535) for each of the three protocols,
 * nports = hi - lo + 1.  A pool entry is e in [0, E), E = naddr * nports: its address is pool[e / nports], its port
 * port_lo + e % nports.  slots: the forward table's size, a power of two in 64..2^26.  statics: nstatic (<= 4096)
 * permanent mappings (port forwards; ports in host byte order; the outside address may be any address).
 * PKT_ERR_INVALID_ARG with a text starting "pkt_nat" (pkt_ctx_last_error for pkt_nat_create, pkt_nat_last_error(NULL)
 * on the calling thread for pkt_nat_create_host): sizes out of range, NULL pool, NULL statics with nstatic > 0, duplicate
 * pool addresses, a static whose proto is not 6 / 17 / 1, a non-zero `zero`, a duplicate inside endpoint per proto, a
 * duplicate outside endpoint per proto, an outside endpoint that is a dynamic pool entry (a pool address with its port
 * in [lo, hi]), nstatic > slots / 2.  pkt_nat_create_host gives the same handle on host memory: every later call then
 * takes HOST pointers, runs sequentially and touches no device (the pkt_flow_table_create_host pattern; the slab's
 * alignment rule is waived).
 *
 * pkt_nat_batch: asynchronous on `stream`, one call at a time per handle, no host readback, no allocation.  dir: device
 * uint8_t[n] or NULL (every packet takes dir_all); PKT_NAT_OUT = 0 (inside to outside), PKT_NAT_IN = 1, any other value
 * skips the packet: a pkt_match_batch action maps onto it directly.  now: the caller's clock, seconds.
 * Per packet i the first test that applies gives status[i]; a packet whose status is not PKT_NAT_OK is not written.
 *  1. select != NULL && select[i] == 0, or its dir >= 2: PKT_NAT_SKIPPED.
 *  2. The IP entry is found exactly as in pkt_flow_key_batch (which_ip, PKT_FLOW_LAST included, over min(n_hdrs,
 *     PKT_MAX_HDRS) entries; a which_ip in 16..0xFE is refused).  None: PKT_NAT_NO_IP.  It is IPv6: PKT_NAT_IPV6.  Its 20
 *     bytes are not inside the packet (under the pkt_batch_t clamp rules): PKT_NAT_SPAN.
 *  3. Byte 0 != 0x45: PKT_NAT_BAD_HDR (pkt_frag_batch's rule: no options).
 *  4. (bytes 6..7 & 0x3FFF) != 0: PKT_NAT_FRAGMENT, the first fragment included (pkt_reasm_batch first).
 *  5. Byte 9 is 6 / 17 / 1 and the list entry right after the IP entry is PKT_HDR_TCP / _UDP / _ICMP respectively,
 *     otherwise PKT_NAT_NO_L4.  The L4 bytes needed are 20 (TCP), 8 (UDP), 8 (ICMP) from that entry's hdr_off; not
 *     inside the packet: PKT_NAT_SPAN.  ICMP whose type byte is neither 8 nor 0: PKT_NAT_NO_L4.  The "port" is bytes
 *     0..1 (source) / 2..3 (destination) of TCP and UDP, bytes 4..5 of ICMP in both directions.
 *  6. OUT: the key is (p, source address, source port).  A session or static with that inside endpoint exists:
 *     PKT_NAT_OK.  Otherwise a session is created: no room in the forward table: PKT_NAT_TABLE_FULL; no free pool entry
 *     of protocol p: PKT_NAT_EXHAUSTED; else PKT_NAT_OK.
 *  7. IN: the destination endpoint equals a static's outside endpoint: PKT_NAT_OK.  It is a dynamic pool entry that is
 *     mapped: PKT_NAT_OK; one that is free: PKT_NAT_NO_SESSION.  Anything else: PKT_NAT_NOT_OURS (the packet is for
 *     the router itself or for someone else; it is untouched).
 * Allocation is exact and the same from run to run.  The model is sequential: take the OUT packets of the call in index
 * order; a packet whose key has no session takes the first free entry of protocol p at or after cursor[p], circularly,
 * marks it, sets cursor[p] = (e + 1) mod E and last_seen = now.  With no free entry the packet is EXHAUSTED and no
 * session exists (a later packet of the key tries again and, within the call, fails again).  After all OUT packets the
 * IN packets are looked up: an IN packet sees the sessions this call's OUT packets created, whatever the two indices.
 * Every OK packet of either direction sets its session's last_seen = max(last_seen, now); statics have no clock.
 * The forward table holds the statics' inside endpoints, the sessions, and the keys that were EXHAUSTED since the last
 * pkt_nat_expire / pkt_nat_clear (those two drop them).  Once any packet of a call is TABLE_FULL, which keys lost is
 * unspecified (pkt_flow_table's rule), and so is which entries that call's new sessions got; every other rule holds and
 * the sessions of earlier calls stay exact.
 * The writes of an OK packet (none with PKT_NAT_NO_WRITE, which still creates and refreshes):
 *  - OUT: the source address (IP bytes 12..15) and the source port / id; IN: the destination address (bytes 16..19)
 *    and the destination port / id.
 *  - The IPv4 checksum (bytes 10..11) and the L4 checksum (TCP bytes 16..17, UDP 6..7, ICMP 2..3), by RFC 1624 eq. 3
 *    over the rewritten 16-bit words m_k -> m'_k: the two address words for the IPv4 checksum; the two address words
 *    (pseudo-header) and the port word for TCP and UDP; the id word alone for ICMP.  s = (~HC & 0xFFFF) +
 *    sum(~m_k & 0xFFFF) + sum(m'_k), folded twice (s = (s & 0xFFFF) + (s >> 16)), HC' = ~s & 0xFFFF.  The words are
 *    always these, whether or not a value differs.  As in pkt_fwd_batch a checksum that was wrong stays wrong by the
 *    same amount and no payload byte is read: a capture cut by snaplen translates correctly.
 *  - UDP: a stored checksum of 0 means none and stays 0; a computed HC' of 0 is stored as 0xFFFF (RFC 768).
 *  - Lengths do not change, so the chain columns stay valid: pkt_fwd_batch, pkt_l4_checksum_batch, pkt_flow_key_batch,
 *    pkt_dispatch_batch and pkt_pcap_write follow with no second parse.
 *  - Stores are narrow: only the bytes named above, in the packet's own IP header and L4 header, at any alignment.
 *    Packets of one batch must not overlap.  Columns that are not a parse of the batch give unspecified packet bytes,
 *    never an access outside the packet.
 * Outputs: device arrays of n elements, each may be NULL.  status: uint8_t.  entry: uint32_t, p * E + e for a dynamic
 * session, PKT_NAT_STATIC | index for a static, PKT_NAT_NONE for a packet that is not OK.  created: uint8_t, 1 iff the
 * packet is the lowest-index packet of a session this call created.  hits / bytes: uint64_t[PKT_NAT_STATUS_COUNT],
 * 8-byte aligned, ADDED to exactly as pkt_fwd_batch's are: every call adds exactly n to sum(hits).
 * PKT_ERR_INVALID_ARG before any launch (the text, starting "pkt_nat", in pkt_nat_last_error and, for a device handle,
 * in pkt_ctx_last_error of its ctx): pkt_fwd_batch's batch and slab rules, a NULL chain or, with n > 0, chain column,
 * n >= 2^32, a bad which_ip, unknown flag bits, dir_all >= 2 with dir == NULL, hits / bytes not 8-byte aligned.  n == 0
 * succeeds and launches nothing.
 *
 * pkt_nat_expire (blocking): a dynamic session of protocol p with idle[p] != 0 and last_seen + idle[p] <= now (64-bit
 * arithmetic) is removed and its pool entry freed; *n_expired (may be NULL) = how many.  Cursors stay where they are;
 * statics never expire.  The forward table is rebuilt from the survivors into a second buffer the handle owns, so its
 * probe chains stay sound and no tombstone is ever reused.  pkt_nat_count (blocking): the dynamic sessions per
 * protocol.  pkt_nat_export (blocking): min(cap, total) records written, *n_out = total: the dynamic sessions in
 * ascending (p, e), then the statics in array order (flags = PKT_NAT_REC_STATIC, last_seen = 0); the order is exact.
 * `records` is device memory for a device handle.  pkt_nat_clear (asynchronous): no dynamic session, cursors 0.
 * pkt_nat_destroy is the caller's to order after the queued calls.  idle, n_expired, counts and n_out are HOST memory.
 * On the device a lane owns a packet and no lane waits for another; kernel boundaries publish: (1) classify, find or
 * claim the key's forward slot by a 64-bit compare-and-swap and put the lowest index into the slot, (2) count the
 * creators per tile and protocol, (3) count the free pool entries per 1024-entry block in circular order from the
 * cursor, (4) one block scans both, (5) the j-th creator of a protocol takes the j-th free entry, (6) translate.
 * (3) to (5) exit at once when the call creates nothing; that is decided on the device.
 * Out of scope: NAT64 / NAT66; hairpinning; paired address pooling with more than one pool address (RFC 4787 REQ-2);
 * port preservation and parity; TCP state tracking and per-state timeouts; the packets quoted in ICMP errors (RFC
 * 5508); ALGs; per-session counters (a pkt_flow_table beside it); IPv4 options. */
typedef struct pkt_nat pkt_nat_t;
typedef struct pkt_nat_static {    /* 16 bytes */
    uint8_t  in_addr[4];           /* wire bytes */
    uint8_t  out_addr[4];
    uint16_t in_port;              /* host byte order; the echo identifier for ICMP */
    uint16_t out_port;
    uint8_t  proto;                /* 6, 17 or 1 */
    uint8_t  zero[3];
} pkt_nat_static_t;
typedef struct pkt_nat_record {    /* 20 bytes */
    uint8_t  in_addr[4];
    uint8_t  out_addr[4];
    uint16_t in_port;
    uint16_t out_port;
    uint8_t  proto;
    uint8_t  flags;                /* PKT_NAT_REC_STATIC */
    uint16_t zero;
    uint32_t last_seen;
} pkt_nat_record_t;
typedef enum pkt_nat_status {
    PKT_NAT_OK         = 0,
    PKT_NAT_SKIPPED    = 1,  /* select[i] == 0, or a dir that is neither OUT nor IN */
    PKT_NAT_NO_IP      = 2,  /* the chain has no such IP entry */
    PKT_NAT_SPAN       = 3,  /* the IP header or the L4 bytes do not lie inside the packet */
    PKT_NAT_IPV6       = 4,
    PKT_NAT_BAD_HDR    = 5,  /* IPv4 byte 0 != 0x45 */
    PKT_NAT_FRAGMENT   = 6,  /* any fragment */
    PKT_NAT_NO_L4      = 7,  /* not TCP / UDP / ICMP echo, or the chain's next entry is not that header */
    PKT_NAT_NO_SESSION = 8,  /* IN: a dynamic pool entry that is free */
    PKT_NAT_NOT_OURS   = 9,  /* IN: neither a static's outside endpoint nor a dynamic pool entry */
    PKT_NAT_EXHAUSTED  = 10, /* OUT: no free pool entry of the protocol */
    PKT_NAT_TABLE_FULL = 11  /* OUT: no room in the forward table */
} pkt_nat_status_t;
#define PKT_NAT_STATUS_COUNT 12
#define PKT_NAT_OUT        0u
#define PKT_NAT_IN         1u
#define PKT_NAT_NO_WRITE   1u            /* flags: create, refresh and decide, store nothing into the slab */
#define PKT_NAT_NONE       0xFFFFFFFFu   /* entry[i] of a packet that is not OK */
#define PKT_NAT_STATIC     0x80000000u   /* entry[i] = PKT_NAT_STATIC | the static's index */
#define PKT_NAT_REC_STATIC 1u
#define PKT_NAT_MAX_ADDR   64u
#define PKT_NAT_MAX_STATIC 4096u
size_t pkt_sizeof_nat_static(void);
size_t pkt_sizeof_nat_record(void);
int pkt_nat_create(pkt_ctx_t *ctx, const uint8_t *pool, uint32_t naddr, uint32_t port_lo, uint32_t port_hi,
                   uint64_t slots, const pkt_nat_static_t *statics, uint32_t nstatic, pkt_nat_t **nat);
int pkt_nat_create_host(const uint8_t *pool, uint32_t naddr, uint32_t port_lo, uint32_t port_hi, uint64_t slots,
                        const pkt_nat_static_t *statics, uint32_t nstatic, pkt_nat_t **nat);
int pkt_nat_batch(pkt_nat_t *nat, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                  uint32_t flags, uint32_t dir_all, const uint8_t *dir, const uint8_t *select, uint32_t now,
                  uint8_t *status, uint32_t *entry, uint8_t *created, uint64_t *hits, uint64_t *bytes,
                  void *stream);
int pkt_nat_expire(pkt_nat_t *nat, uint32_t now, const uint32_t idle[3], uint64_t *n_expired);
int pkt_nat_count(pkt_nat_t *nat, uint64_t counts[3]);
int pkt_nat_export(pkt_nat_t *nat, pkt_nat_record_t *records, uint64_t cap, uint64_t *n_out);
int pkt_nat_clear(pkt_nat_t *nat, void *stream);
int pkt_nat_destroy(pkt_nat_t *nat);
const char *pkt_nat_last_error(const pkt_nat_t *nat);

/* ---- pkt_tunnel_*: VXLAN, GRE and IP-in-IP encapsulation and decapsulation of a batch ----
 * What an overlay or edge router does before and after everything else: put every packet of a parsed batch into the
 * tunnel a table entry describes, or take the packets of terminated tunnels out again.  The outputs are packed into a
 * second slab exactly as pkt_frag_batch packs its own, with the chain columns the following calls need.  The wire
 * formats are RFC 7348 (VXLAN), RFC 2784 / 2890 (GRE, version 0, optional key) and RFC 2003 / 2473 (IP in IP); the
 * reference's builders (utils.rs create_vxlan_packet, create_gre_packet, create_ipv4ip_packet, create_ipv6ip_packet)
 * give the same bytes but for the outer IPv4 checksum they leave stale (Q9) and the 0xFFFF they store as the IPv6 UDP
 * checksum.
 *
 * The table.  pkt_tunnel_create: blocking, and the only allocating call; 1..PKT_TUN_MAX_ENTRIES entries.  An entry:
 *    kind    PKT_TUN_VXLAN: outer Ether / IP / UDP (destination 4789) / VXLAN around the whole source frame;
 *            PKT_TUN_GRE: outer IP / GRE around the source's IP packet; PKT_TUN_IPIP: outer IP around it.
 *    ipver   the outer IP version, 4 or 6; src / dst: the outer addresses, wire bytes, IPv4 in the first 4.
 *    ttl     the outer ttl / hop limit, 0 = 64; tos: the outer tos / traffic class.
 *    id      the VNI (at most 2^24 - 1), or the GRE key with PKT_TUN_F_KEY; otherwise ignored.
 *    sport_lo / sport_hi  VXLAN's UDP source port range (ignored by the other kinds, the order is still checked).
 *    eth_dst / eth_src    VXLAN's outer MACs; pkt_fwd_batch over the output rewrites them, so they may be zero.
 *    flags   PKT_TUN_F_KEY: GRE carries `id` as its key.  PKT_TUN_F_DF: the outer IPv4 header has DF set.
 *            PKT_TUN_F_INHERIT_TOS: the outer tos / traffic class is the inner IP header's (IPv4 byte 1, the IPv6 traffic
 *            class); for VXLAN that of the chain's first IPv4 / IPv6 entry if its first two bytes lie inside the packet,
 *            else the entry's tos.  PKT_TUN_F_UDP_CSUM: the outer UDP checksum is computed; without it an IPv4 outer
 *            stores 0 (RFC 7348) and an IPv6 outer stores 0 as well (RFC 6935 zero-checksum mode for tunnels).
 *            PKT_TUN_F_ANY_REMOTE: decap matches any outer source address.
 * On the host, create builds the decap lookup: open addressing with linear probing over the entries' keys (kind,
 * ipver, GRE key present, local = src, remote = dst or the wildcard with ANY_REMOTE, id as matched: the VNI, the key,
 * else 0), at least twice as many slots as entries, read-only afterwards: encap and decap calls on several streams
 * share a handle.  PKT_ERR_INVALID_ARG with a text starting "pkt_tunnel" (pkt_ctx_last_error for pkt_tunnel_create,
 * pkt_tunnel_last_error(NULL) on the calling thread for pkt_tunnel_create_host): NULL entries; a count of 0 or above
 * PKT_TUN_MAX_ENTRIES; an unknown kind; an ipver that is neither 4 nor 6; unknown flag bits; a VNI above 2^24 - 1;
 * sport_lo > sport_hi; KEY on an entry that is not GRE; UDP_CSUM on an entry that is not VXLAN; a non-zero `zero`; two
 * entries with the same decap key.  pkt_tunnel_create_host gives the same handle on host memory for the _host calls.
 *
 * pkt_tunnel_encap_batch, per source packet i: the first test that applies gives status[i].  t = tunnel ? tunnel[i] :
 * tunnel_all (pkt_lpm_lookup_batch's nexthop or pkt_fwd_batch's adj_index / port as they are); E = entry t.
 *  1. select != NULL && select[i] == 0: PKT_TUNE_SKIPPED.
 *  2. t >= the table's size: PKT_TUNE_NO_TUNNEL.
 *  Steps 3 to 7 are for GRE and IPIP alone (VXLAN wraps the frame whatever it holds; which_ip is not used):
 *  3. The IP entry is found exactly as in pkt_fwd_batch step 2 (which_ip, PKT_FLOW_LAST included, over min(n_hdrs,
 *     PKT_MAX_HDRS) entries).  None: PKT_TUNE_NO_IP.  Its 20 / 40 bytes not inside the packet's length (under the
 *     pkt_batch_t clamp rules): PKT_TUNE_SPAN.  P = ip_off.
 *  4. The IP entry is not entry 0 and the entry just before it is neither Ether nor VLAN nor MPLS: PKT_TUNE_BAD_L2.
 *  5. That entry is Ether or VLAN and ip_off < 2 (only a forged chain gives that): PKT_TUNE_SPAN.
 *  6. IPv4: byte 0 != 0x45 or L = bytes 2..3 < 20; IPv6: byte 0 >> 4 != 6 (L = 40 + bytes 4..5): PKT_TUNE_BAD_HDR.
 *  7. ip_off + L > the packet's length: PKT_TUNE_TRUNC.
 *  8. The outer IP length field would pass 65535: PKT_TUNE_TOO_BIG.  VXLAN: 36 + len under IPv4, 16 + len under IPv6;
 *     GRE / IPIP: 20 + G + L under IPv4, G + L under IPv6, G = 0 (IPIP), 4 or 8 (GRE without / with the key).
 *  9. min(n_hdrs, PKT_MAX_HDRS) plus the added rows (VXLAN 4, IPIP 1, GRE 2 or 3) exceeds PKT_MAX_HDRS: PKT_TUNE_DEPTH.
 * 10. PKT_TUNE_OK: one output.
 * The output of an OK packet:
 *  - VXLAN, 50 / 70 + len bytes: Ether (eth_dst, eth_src, 0x0800 / 0x86DD), the outer IP, UDP (source port sport_lo +
 *    entropy[i] % (sport_hi - sport_lo + 1), sport_lo without `entropy`; destination 4789; length 16 + len; checksum),
 *    VXLAN (08 00 00 00, VNI, 00), then the source packet's bytes [0, len).
 *  - GRE / IPIP, P + H + G + L bytes: the source's [0, P) verbatim, the two bytes before P set to the outer version's
 *    ethertype when the entry before the IP entry is Ether or VLAN (MPLS has none to set); the outer IP; GRE (flags
 *    0x2000 with the key else 0, protocol 0x0800 / 0x86DD by the inner version, then the key); the inner bytes [P, P +
 *    L).  Source bytes past P + L (Ethernet padding) go nowhere, as in pkt_frag_batch.
 *  - Outer IPv4: 45, tos, the total length, identification (ident + q) & 0xFFFF with q the output's index
 *    (pkt_icmp_err_batch's rule), bytes 6..7 = 0x4000 with DF else 0, ttl, protocol 17 / 47 / 4 or 41 by the inner
 *    version, the RFC 1071 checksum of the 20 bytes, src, dst.  The checksum is the correct fold (as in
 *    pkt_icmp_err_batch); Packet::ipv4_checksum gives the same value except where its single fold drops a carry.
 *  - Outer IPv6: version 6, traffic class tos, flow label 0, the payload length, next header as above, hop limit, src, dst.
 *  - The UDP checksum with PKT_TUN_F_UDP_CSUM: RFC 1071 over the pseudo-header and the whole datagram; a computed 0 is
 *    stored as 0xFFFF: what pkt_l4_checksum_batch (which = 0) calls PKT_L4_OK, and PKT_L4_UNCHECKED without the flag.
 * out_chain: VXLAN: (Ether, 0), (IPv4 / IPv6, 14), (UDP, 14 + H), (VXLAN, 22 + H), then the source's rows with hdr_off
 * + 50 / 70.  GRE / IPIP: the source's rows before the IP entry as they are, (IPv4 / IPv6, P), for GRE (GRE, P + H) and
 * with the key (GRE_KEY, P + H + 4) (the reference's list order), then the source's rows from the IP entry on with
 * hdr_off + H + G.  That is what a parse of the output gives for a source that starts with an Ether entry, so
 * pkt_fwd_batch with which_ip = 0 (it routes on the outer header), pkt_frag_batch (it splits the OUTER datagram: encap
 * first, then fragment, is the order in which no outer length is left to fix), pkt_l4_checksum_batch,
 * pkt_flow_key_batch, pkt_dispatch_batch and pkt_pcap_write take the result with no second parse.
 *
 * pkt_tunnel_decap_batch, per source packet i: the first test that applies gives status[i].
 *  1. select != NULL && select[i] == 0: PKT_TUND_SKIPPED.
 *  2. The outer IP entry is the which_ip-th IP entry (step 3 above).  None: PKT_TUND_NO_IP.
 *  3. Its H = 20 / 40 bytes not inside the packet's length: PKT_TUND_SPAN.  A = ip_off + H.
 *  4. IPv4 byte 0 != 0x45; IPv6 byte 0 >> 4 != 6: PKT_TUND_BAD_HDR.
 *  5. IPv4 with (bytes 6..7 & 0x3FFF) != 0, any fragment: PKT_TUND_FRAGMENT (pkt_reasm_batch first).
 *  6. The kind is read from the chain entries behind the IP entry: (UDP, A) and (VXLAN, A + 8): VXLAN, T = 16; (GRE,
 *     A): GRE, T = 4; (IPv4 / IPv6, A): IPIP, T = 0.  Anything else, a differing hdr_off included: PKT_TUND_NOT_TUNNEL.
 *  7. A + T > the packet's length: PKT_TUND_SPAN.  Lo = IPv4 bytes 2..3, or 40 + IPv6 bytes 4..5.
 *  8. VXLAN: the UDP length != Lo - H: PKT_TUND_BAD_HDR.  GRE: byte 0 & 0xD0 (checksum, routing, sequence), byte 1 & 7
 *     (version), a protocol that is neither 0x0800 nor 0x86DD, or a GRE_CHKSUM_OFFSET / GRE_SEQUENCE_NUM entry among
 *     the two entries behind the GRE entry: PKT_TUND_BAD_GRE.  GRE with the key bit: T = 8, and A + 8 > the length:
 *     PKT_TUND_SPAN.
 *  9. The lookup: (kind, outer version, key present, local = the outer destination, remote = the outer source, id =
 *     the VNI / the key / 0), the exact key first, then the ANY_REMOTE key.  No entry: PKT_TUND_NO_MATCH.
 * 10. ip_off + Lo > the packet's length: PKT_TUND_TRUNC.
 * 11. I = Lo - H - T (0 if that is negative).  VXLAN: no chain entry behind the VXLAN entry, or I < 14; GRE / IPIP: I <
 *     20 / 40 by the inner version (GRE's protocol, IPIP's chain entry): PKT_TUND_NO_INNER.
 * 12. PKT_TUND_OK: one output.  VXLAN: the source's [A + 16, ip_off + Lo), I bytes; out_chain = the source's rows behind
 *     the VXLAN entry with hdr_off - (A + 16).  GRE / IPIP: the source's [0, ip_off) with the two bytes before ip_off set
 *     to the inner version's ethertype when the entry before the IP entry is Ether or VLAN, then [A + T, ip_off + Lo);
 *     out_chain = the rows before the IP entry, then the rows behind the outer ones (IP, GRE, GRE_KEY) with hdr_off -
 *     (H + T).  Rows whose hdr_off a forged chain put below what is subtracted wrap modulo 2^16.
 * tunnel_out[i] = the matched entry from step 9 on, PKT_TUN_NONE before.  Checksums are NOT verified:
 * pkt_l4_checksum_batch before this call if that is wanted.
 *
 * Both calls.  Outputs are in source order, exact and the same from run to run.  Per source packet: status[i] and
 * out_index[i] (PKT_TUN_NONE without an output).  dst, out_off, out_len, src_index, out_chain, the layout rule
 * (out_off[q + 1] = out_off[q] + round_up(out_len[q], 16), the rounded tail zeros), the empty tail [*n_out, out_cap),
 * PKT_TUN_NO_WRITE (the sizing pass: only status, out_index, tunnel_out, hits and the totals), the overflow return with
 * both totals set and decided on the device, and _async / _result with one call in flight per ctx AND entry (an encap
 * and a decap may be in flight together) are pkt_frag_batch's, word for word.  status, out_index, tunnel_out,
 * src_index, hits, out_chain and each of its columns may be NULL.  Chain columns that are not a parse of the batch give
 * a status or unspecified output bytes, never an access outside [slab, slab + round_up(slab_len, 16)).
 * hits: device uint64_t[PKT_TUNE_STATUS_COUNT / PKT_TUND_STATUS_COUNT], 8-byte aligned, ADDED to; every call adds exactly n.
 *  - PKT_ERR_INVALID_ARG before any launch, with a text starting "pkt_tunnel" in pkt_ctx_last_error: pkt_frag_batch's
 *    batch, slab, chain, which_ip, flag, alignment (dst 16, hits 8, out_off 8) and capacity rules; a NULL table; a host
 *    handle (a device handle for the _host calls); a table of another device; tunnel / entropy / tunnel_out not 4-byte
 *    aligned; a second call of the same entry on the ctx before its _result.  n == 0 succeeds with both totals 0.
 *  - Scratch lives in the ctx and grows on demand.
 *  - On the device, three launches: a decision kernel (a lane owns a source packet: the chain, the entry by four
 *    16-byte loads, the header bytes the tests need by the aligned 16-byte chunks that hold them, for decap the lookup,
 *    a 32-byte plan; per tile of 256 the outputs and rounded bytes; per-status counts merged per block in LDS), the
 *    one-block scan pkt_frag_batch uses, and one build kernel for both calls (a wave walks the 16-byte chunks of its 64
 *    sources' outputs together; each chunk is built in registers from the prefix, the header words and the two aligned
 *    source chunks that hold its payload bytes, and stored whole; with UDP_CSUM the payload's 16-bit words are summed
 *    chunk by chunk into the output's LDS word and the chunk that holds the checksum is stored once the wave's sums
 *    are complete; the lane writes its output's out_chain rows).  No lane waits for another; no global atomics but hits.
 * pkt_tunnel_encap_host / _decap_host are the same operations on HOST pointers with a pkt_tunnel_create_host handle: no
 * ctx, no device; the slab's alignment rule is waived.
 * Out of scope: Geneve; NVGRE / GRE transparent bridging (the parser does not walk 0x6558); MPLS push; IPv6 extension
 * headers and IPv4 options; the ECN decapsulation rules of RFC 6040; outer checksum verification; per-tunnel counters
 * (a bincount of tunnel_out). */
typedef struct pkt_tunnel pkt_tunnel_t;
typedef struct pkt_tunnel_entry {  /* 64 bytes */
    uint8_t  kind;                 /* pkt_tunnel_kind_t */
    uint8_t  ipver;                /* 4 or 6 */
    uint8_t  ttl;                  /* 0 = 64 */
    uint8_t  tos;
    uint32_t flags;                /* PKT_TUN_F_* */
    uint32_t id;                   /* the VNI or the GRE key */
    uint16_t sport_lo;
    uint16_t sport_hi;
    uint8_t  src[16];              /* wire bytes, IPv4 in the first 4 */
    uint8_t  dst[16];
    uint8_t  eth_dst[6];
    uint8_t  eth_src[6];
    uint32_t zero;
} pkt_tunnel_entry_t;
typedef enum pkt_tunnel_kind {
    PKT_TUN_VXLAN = 0,
    PKT_TUN_GRE   = 1,
    PKT_TUN_IPIP  = 2
} pkt_tunnel_kind_t;
typedef enum pkt_tune_status {
    PKT_TUNE_OK        = 0,  /* one output */
    PKT_TUNE_SKIPPED   = 1,  /* select[i] == 0 */
    PKT_TUNE_NO_TUNNEL = 2,  /* the index is at or above the table's size */
    PKT_TUNE_NO_IP     = 3,  /* GRE / IPIP: the chain has no such IP entry */
    PKT_TUNE_SPAN      = 4,  /* its bytes are not inside the packet */
    PKT_TUNE_BAD_L2    = 5,  /* the entry before it is neither Ether nor VLAN nor MPLS */
    PKT_TUNE_BAD_HDR   = 6,  /* IPv4 byte 0 != 0x45 or total length < 20; IPv6 version != 6 */
    PKT_TUNE_TRUNC     = 7,  /* the inner L3 length runs past the packet */
    PKT_TUNE_TOO_BIG   = 8,  /* the outer length would pass 65535 */
    PKT_TUNE_DEPTH     = 9   /* more than PKT_MAX_HDRS rows */
} pkt_tune_status_t;
#define PKT_TUNE_STATUS_COUNT 10
typedef enum pkt_tund_status {
    PKT_TUND_OK         = 0,  /* one output */
    PKT_TUND_SKIPPED    = 1,
    PKT_TUND_NO_IP      = 2,
    PKT_TUND_SPAN       = 3,  /* the outer IP or tunnel header is not inside the packet */
    PKT_TUND_BAD_HDR    = 4,  /* IPv4 byte 0 != 0x45, IPv6 version != 6, or a UDP length that disagrees with the IP length */
    PKT_TUND_FRAGMENT   = 5,  /* any outer IPv4 fragment */
    PKT_TUND_NOT_TUNNEL = 6,  /* the chain entries behind the IP entry are no tunnel's */
    PKT_TUND_BAD_GRE    = 7,  /* checksum, sequence or routing, a version other than 0, an unknown protocol */
    PKT_TUND_NO_MATCH   = 8,  /* no table entry */
    PKT_TUND_TRUNC      = 9,  /* the outer length field runs past the packet */
    PKT_TUND_NO_INNER   = 10  /* nothing (or too little) inside */
} pkt_tund_status_t;
#define PKT_TUND_STATUS_COUNT 11
#define PKT_TUN_F_KEY         1u
#define PKT_TUN_F_DF          2u
#define PKT_TUN_F_INHERIT_TOS 4u
#define PKT_TUN_F_UDP_CSUM    8u
#define PKT_TUN_F_ANY_REMOTE  16u
#define PKT_TUN_NO_WRITE      1u          /* call flags: decide and total everything, store no packet byte and no per-output array */
#define PKT_TUN_NONE          0xFFFFFFFFu /* out_index[i] / src_index[q] / tunnel_out[i] when there is none */
#define PKT_TUN_MAX_ENTRIES   65536u
size_t pkt_sizeof_tunnel_entry(void);
int pkt_tunnel_create(pkt_ctx_t *ctx, const pkt_tunnel_entry_t *entries, uint32_t count, pkt_tunnel_t **tun);
int pkt_tunnel_create_host(const pkt_tunnel_entry_t *entries, uint32_t count, pkt_tunnel_t **tun);
int pkt_tunnel_destroy(pkt_tunnel_t *tun);
const char *pkt_tunnel_last_error(const pkt_tunnel_t *tun);
int pkt_tunnel_encap_batch(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                           uint32_t flags, const pkt_tunnel_t *tun, const uint32_t *tunnel, uint32_t tunnel_all,
                           const uint32_t *entropy, uint32_t ident, const uint8_t *select,
                           uint8_t *status, uint32_t *out_index,
                           uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                           uint64_t *out_off, uint32_t *out_len, uint32_t *src_index,
                           const pkt_chain_t *out_chain,
                           uint64_t *hits, uint64_t *bytes_out_total, uint64_t *n_out, void *stream);
int pkt_tunnel_encap_batch_async(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                                 uint32_t flags, const pkt_tunnel_t *tun, const uint32_t *tunnel, uint32_t tunnel_all,
                                 const uint32_t *entropy, uint32_t ident, const uint8_t *select,
                                 uint8_t *status, uint32_t *out_index,
                                 uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                                 uint64_t *out_off, uint32_t *out_len, uint32_t *src_index,
                                 const pkt_chain_t *out_chain, uint64_t *hits, void *stream);
int pkt_tunnel_encap_result(pkt_ctx_t *ctx, uint64_t *bytes_out_total, uint64_t *n_out);
int pkt_tunnel_encap_host(const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                          uint32_t flags, const pkt_tunnel_t *tun, const uint32_t *tunnel, uint32_t tunnel_all,
                          const uint32_t *entropy, uint32_t ident, const uint8_t *select,
                          uint8_t *status, uint32_t *out_index,
                          uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                          uint64_t *out_off, uint32_t *out_len, uint32_t *src_index,
                          const pkt_chain_t *out_chain,
                          uint64_t *hits, uint64_t *bytes_out_total, uint64_t *n_out);
int pkt_tunnel_decap_batch(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                           uint32_t flags, const pkt_tunnel_t *tun, const uint8_t *select,
                           uint8_t *status, uint32_t *out_index, uint32_t *tunnel_out,
                           uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                           uint64_t *out_off, uint32_t *out_len, uint32_t *src_index,
                           const pkt_chain_t *out_chain,
                           uint64_t *hits, uint64_t *bytes_out_total, uint64_t *n_out, void *stream);
int pkt_tunnel_decap_batch_async(pkt_ctx_t *ctx, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                                 uint32_t flags, const pkt_tunnel_t *tun, const uint8_t *select,
                                 uint8_t *status, uint32_t *out_index, uint32_t *tunnel_out,
                                 uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                                 uint64_t *out_off, uint32_t *out_len, uint32_t *src_index,
                                 const pkt_chain_t *out_chain, uint64_t *hits, void *stream);
int pkt_tunnel_decap_result(pkt_ctx_t *ctx, uint64_t *bytes_out_total, uint64_t *n_out);
int pkt_tunnel_decap_host(const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                          uint32_t flags, const pkt_tunnel_t *tun, const uint8_t *select,
                          uint8_t *status, uint32_t *out_index, uint32_t *tunnel_out,
                          uint8_t *dst, uint64_t dst_len, uint64_t out_cap,
                          uint64_t *out_off, uint32_t *out_len, uint32_t *src_index,
                          const pkt_chain_t *out_chain,
                          uint64_t *hits, uint64_t *bytes_out_total, uint64_t *n_out);

/* ---- pkt_meter_*: srTCM (RFC 2697) and trTCM (RFC 2698) token-bucket policers over a batch ----
 * The reference defines nothing here; this section fixes the semantics.  A meter table handle owns the state of
 * nmeters (1..PKT_METER_MAX_METERS) meters; one call takes a batch, colours every packet green, yellow or red against
 * the meter its index names (a flow_id of pkt_flow_table_update, a rule id of pkt_match_batch, a port of
 * pkt_fwd_batch), and passes, drops or remarks it.  The ABI stays v5 (additions only).
 *
 * pkt_meter_create: blocking, and the only allocating call.  cfg: HOST array of nmeters pkt_meter_cfg_t (32 bytes, every
 * byte a checked field: the struct has no padding).  cir / pir: bytes per second, at most PKT_METER_MAX_RATE (2^40); pir
 * is ignored by srTCM.  cbs / xbs: bytes, at most PKT_METER_MAX_BURST (2^26); xbs is EBS for srTCM and PBS for trTCM.
 * mode: PKT_METER_SRTCM or PKT_METER_TRTCM.  flags: PKT_METER_F_COLOR_AWARE.  action[c] for colour c = green, yellow,
 * red: PKT_METER_PASS / _DROP / _REMARK; dscp[c] (0..63) is what REMARK writes.  adjust is added to every packet's
 * length (+20: preamble and gap; -14: L3 bytes); the sum is clamped at 0.  Anything out of range is
 * PKT_ERR_INVALID_ARG with a text starting "pkt_meter" (pkt_ctx_last_error for pkt_meter_create,
 * pkt_meter_last_error(NULL) on the calling thread for pkt_meter_create_host).  pkt_meter_create_host gives the same
 * handle on host memory: every later call then takes HOST pointers and runs the sequential model itself.
 *
 * State per meter (pkt_meter_state_t, 72 bytes): the buckets c and x in units of 10^-9 byte, `last` in ns, and six
 * exact counters: packets and bytes (the packet's length, without adjust) per colour.  Create and pkt_meter_reset
 * (asynchronous on `stream`) set the buckets full (cbs * 10^9, xbs * 10^9), last = 0 and the counters to 0.
 * pkt_meter_export (blocking): the state of meters [first, first + count) into `out`, device memory for a device handle.
 *
 * pkt_meter_batch: asynchronous on `stream`, one call at a time per handle, no host readback, no allocation.  meter:
 * uint32_t[n] or NULL (every packet takes meter_all).  time_ns: uint64_t[n] or NULL (every packet takes now_ns).
 * in_color, select: uint8_t[n] or NULL.  The model is sequential and in unbounded integers: the packets in index
 * order, for packet i:
 *  1. select != NULL && select[i] == 0, or k = (meter ? meter[i] : meter_all) >= nmeters (a flow_id of 0xFFFFFFFF falls
 *     out here): color[i] = PKT_METER_UNMETERED (3), pass[i] = 1, marked[i] = 0, and nothing else happens.
 *  2. t = time_ns ? time_ns[i] : now_ns.  B = max(0, len_i + adjust) * 10^9, len_i the packet's length under the
 *     pkt_batch_t clamp rules.
 *  3. Refill, only if t > last_k: dt = t - last_k, last_k = t (a time that runs backwards refills nothing and leaves
 *     last).  srTCM: a = cir * dt, c' = min(cbs * 10^9, c + a), x' = min(xbs * 10^9, x + (c + a - c')).
 *     trTCM: c' = min(cbs * 10^9, c + cir * dt), x' = min(xbs * 10^9, x + pir * dt).
 *  4. ic = in_color[i] if in_color != NULL and the meter has PKT_METER_F_COLOR_AWARE, else green; above 2 counts as red.
 *     srTCM: ic == green && c >= B: green, c -= B; else ic <= yellow && x >= B: yellow, x -= B; else red.
 *     trTCM: ic == red || x < B: red; else ic == yellow || c < B: yellow, x -= B; else green, c -= B and x -= B.
 *  5. color[i]; pass[i] = action[color] != PKT_METER_DROP.  The meter's counters and the call's hits[4] / bytes[4]
 *     (index 3: the unmetered packets) take the packet; bytes counts len_i.  hits / bytes are ADDED to, as
 *     pkt_fwd_batch's are: exactly n per call.
 *  6. With the call flag PKT_METER_MARK and action[color] == PKT_METER_REMARK: the IP entry is found as in pkt_fwd_batch
 *     step 2 (which_ip); if its 20 / 40 bytes lie inside the packet, the DSCP is written and marked[i] = 1.  IPv4:
 *     byte 1's upper six bits, bytes 10..11 updated by RFC 1624 eq. 3 over that one word (a wrong checksum stays wrong
 *     by as much).  IPv6: the six bits straddling bytes 0..1.  The ECN bits and everything else are kept; the stores
 *     are byte stores.  Otherwise marked[i] = 0.  The colour and `pass` never depend on headers.  Forged chain columns
 *     give unspecified packet bytes, never an access outside the packet.
 * So a batch split at any index into two calls gives what the one call gives, meters are independent of each other,
 * and the results are the same from run to run.  Every output may be NULL.
 * PKT_ERR_INVALID_ARG before any launch (the text, starting "pkt_meter", in pkt_meter_last_error and, for a device
 * handle, pkt_ctx_last_error): the batch and slab rules of pkt_fwd_batch, n >= 2^32, unknown flag bits, PKT_METER_MARK
 * with a NULL chain (or a NULL chain column) or a which_ip in 16..0xFE, hits / bytes / time_ns not 8-byte aligned,
 * meter not 4-byte aligned.  Without PKT_METER_MARK chain may be NULL and which_ip is not looked at.  n == 0 succeeds
 * and launches nothing.  pkt_meter_destroy is the caller's to order after the queued calls.
 * The worst case is one meter's long run: its packets are walked in order, 64 at a step, by one wave.
 * Out of scope: RFC 4115; the DSCP-to-colour mapping of the incoming packet (a pkt_match_batch program's action gives
 * in_color); hierarchical policers; shapers and queues; reconfiguring a live table; packet-rate (pps) meters. */
typedef struct pkt_meter pkt_meter_t;
typedef struct pkt_meter_cfg {     /* 32 bytes */
    uint64_t cir;                  /* bytes per second */
    uint64_t pir;
    uint32_t cbs;                  /* bytes */
    uint32_t xbs;
    uint8_t  mode;                 /* PKT_METER_SRTCM / PKT_METER_TRTCM */
    uint8_t  flags;                /* PKT_METER_F_COLOR_AWARE */
    uint8_t  action[3];            /* for green, yellow, red */
    uint8_t  dscp[3];              /* for green, yellow, red: what PKT_METER_REMARK writes */
} pkt_meter_cfg_t;
typedef struct pkt_meter_state {   /* 72 bytes */
    uint64_t c;                    /* 10^-9 byte */
    uint64_t x;
    uint64_t last;                 /* ns */
    uint64_t packets[3];           /* per colour */
    uint64_t bytes[3];
} pkt_meter_state_t;
#define PKT_METER_GREEN     0u
#define PKT_METER_YELLOW    1u
#define PKT_METER_RED       2u
#define PKT_METER_UNMETERED 3u
#define PKT_METER_COLORS    4
#define PKT_METER_SRTCM     0u
#define PKT_METER_TRTCM     1u
#define PKT_METER_F_COLOR_AWARE 1u
#define PKT_METER_PASS      0u
#define PKT_METER_DROP      1u
#define PKT_METER_REMARK    2u
#define PKT_METER_MARK      1u            /* call flags: do the REMARK stores */
#define PKT_METER_MAX_METERS (1u << 24)
#define PKT_METER_MAX_RATE   (1ull << 40)
#define PKT_METER_MAX_BURST  (1u << 26)
size_t pkt_sizeof_meter_cfg(void);
size_t pkt_sizeof_meter_state(void);
int pkt_meter_create(pkt_ctx_t *ctx, const pkt_meter_cfg_t *cfg, uint32_t nmeters, int32_t adjust, pkt_meter_t **m);
int pkt_meter_create_host(const pkt_meter_cfg_t *cfg, uint32_t nmeters, int32_t adjust, pkt_meter_t **m);
int pkt_meter_batch(pkt_meter_t *m, const pkt_batch_t *batch, const pkt_chain_t *chain, uint32_t which_ip,
                    uint32_t flags, uint32_t meter_all, const uint32_t *meter, uint64_t now_ns, const uint64_t *time_ns,
                    const uint8_t *in_color, const uint8_t *select, uint8_t *color, uint8_t *pass, uint8_t *marked,
                    uint64_t *hits, uint64_t *bytes, void *stream);
int pkt_meter_reset(pkt_meter_t *m, void *stream);
int pkt_meter_export(pkt_meter_t *m, uint32_t first, uint32_t count, pkt_meter_state_t *out);
int pkt_meter_destroy(pkt_meter_t *m);
const char *pkt_meter_last_error(const pkt_meter_t *m);

/* Packet::ipv4_checksum on the host (same arithmetic as the device kernel). */
uint16_t pkt_ipv4_checksum_host(const uint8_t *hdr, size_t len);

/* The largest n_hdrs[i] over n packets (`n_hdrs`: a device column from pkt_parse_batch): the slot
 * rows of hdr_type / hdr_off that hold data — a PacketSlice holds exactly its headers (lib.rs:136-140),
 * so a copy or gather of a batch's chain moves rows [0, *max_out) only.  Blocking (waits for
 * `stream`).  One such call at a time per ctx. */
int pkt_chain_max_hdrs(pkt_ctx_t *ctx, const uint8_t *n_hdrs, uint64_t n, uint32_t *max_out, void *stream);

/* PacketSlice of packet i of a parsed batch whose chain columns are in HOST memory (pkt_parse_host's
 * output, or device columns copied back): for k < *n_hdrs, types[k] / offs[k] = the k-th header of
 * the PacketSlice's list (its type id and its byte offset in the packet: the Slice the reference's
 * `insert` put at position k, lib.rs:136-140, packet.rs:724-726), and the payload is packet bytes
 * [*payload_off, *payload_off + *payload_len) (`set_payload`, packet.rs:728-731).  `out` must hold
 * status, n_hdrs, hdr_type, hdr_off, payload_off and payload_len (slot columns strided by n).  Returns
 * the packet's pkt_status_t (>= 0; on a status other than PKT_OK the reference panicked, there is no
 * PacketSlice, and *n_hdrs = *payload_off = *payload_len = 0), or PKT_ERR_INVALID_ARG.  Host only. */
int pkt_view(const pkt_out_t *out, uint64_t n, uint64_t i, uint8_t types[PKT_MAX_HDRS],
             uint16_t offs[PKT_MAX_HDRS], uint32_t *n_hdrs, uint16_t *payload_off, uint16_t *payload_len);

/* ---- packed output buffers (host only, no device needed) ----
 * A column mask selects pkt_out_t members: bit k = the k-th pointer of pkt_out_t (0 = status,
 * ..., 48 = udp_checksum).  The packed layout puts every selected column of an n-packet output in
 * one buffer, each column starting on a 256-byte boundary: the per-packet columns in pkt_out_t
 * order, then the slot columns hdr_type and hdr_off ([PKT_MAX_HDRS][n] each) last.  One buffer per
 * shard is what the multi-GPU gather moves; with only the used slot rows (pkt_out_packed_pieces)
 * that is at most two contiguous pieces. */
#define PKT_COL(k)      (1ull << (k))
#define PKT_COLS_ALL    ((1ull << 49) - 1)
#define PKT_COLS_CHAIN  0x7Full               /* status .. hdr_mask */
#define PKT_COLS_ETHER  (0x7ull << 7)
#define PKT_COLS_VLAN   (0xFull << 10)
#define PKT_COLS_IPV4   (0x1FFFull << 14)
#define PKT_COLS_IPV6   (0xFFull << 27)
#define PKT_COLS_TCP    (0x3FFull << 35)
#define PKT_COLS_UDP    (0xFull << 45)
/* Fills `out` with the selected columns' pointers inside `base` (NULL columns elsewhere; `base`
 * may be NULL to size only) and sets *bytes to the buffer size. */
int pkt_out_packed(uint64_t col_mask, uint64_t n, void *base, pkt_out_t *out, uint64_t *bytes);
/* The byte ranges of an n-packet packed buffer that hold every selected column with only the first
 * `rows` (<= PKT_MAX_HDRS) slot rows of hdr_type / hdr_off: piece k = [off[k], off[k] + len[k]),
 * k < *npieces (2 when both slot columns are selected: the head through hdr_type's used rows, then
 * hdr_off's used rows; else 1).  C2's chain + Ether/IPv4/UDP at rows = 3 is 69 B per packet. */
int pkt_out_packed_pieces(uint64_t col_mask, uint64_t n, uint32_t rows, uint64_t off[2], uint64_t len[2],
                          int *npieces);
/* The column mask of a pkt_out_t (bit k set iff its k-th pointer is non-NULL). */
uint64_t pkt_out_mask(const pkt_out_t *out);
/* [lo, hi) of shard i of n packets split into `nshards` contiguous blocks whose sizes differ by
 * at most one (the lower shards take the remainder). */
int pkt_shard_range(uint64_t n, int nshards, int i, uint64_t *lo, uint64_t *hi);

/* The gather plan of pkt_mgpu_parse_gather (host only): one piece per message — `bytes` bytes from
 * offset `src` of shard `shard`'s packed buffer to offset `dst` of the root's receive buffer — for
 * `nshards` shards of n[i] packets whose batches use rows[i] (<= PKT_MAX_HDRS; rows NULL = all 16)
 * slot rows.  merge = 0: shard i's packed buffer (its used slot rows only, pkt_out_packed_pieces) at
 * the next 256-byte boundary of recv; merge = 1: recv is ONE packed output of sum(n) packets (each
 * column of shard i at packets [lo_i, lo_i + n_i), one piece per column and per used slot row — the
 * pieces the root's repack places after the merge = 0 transfer, see pkt_mgpu_parse_gather).
 * Writes min(cap, count) pieces, *npieces = count, *recv_bytes = the receive buffer size. */
typedef struct pkt_gather_piece {
    uint64_t src;
    uint64_t dst;
    uint64_t bytes;
    int32_t  shard;
    uint32_t reserved;
} pkt_gather_piece_t;
size_t pkt_sizeof_gather_piece(void);
int pkt_gather_plan(uint64_t col_mask, int nshards, const uint64_t *n, const uint32_t *rows, int merge,
                    pkt_gather_piece_t *pieces, uint64_t cap, uint64_t *npieces, uint64_t *recv_bytes);

/* ---- a capture that arrives in pieces (a NIC ring drained into host memory, a file read as it grows) ----
 * The capture path of tests/pcap.rs:7-37 as a stream: bytes are pushed as they arrive and the device
 * indexes and parses the records they complete while later bytes are still in flight.  Each step
 * indexes only the new bytes: the device keeps the first record start a step could not count yet (a
 * record running past the bytes so far) and the record count, and the next step starts the device
 * indexer from them (no re-walk from offset 24: the window is indexed once however many steps).
 *
 * THE WINDOW.  The stream holds a WINDOW of the capture in one device buffer of max_bytes: the 24-byte
 * global header, then the capture's bytes from the first unreleased record header onward.  Window
 * offset w is capture offset w + released_bytes, window record i is capture record i +
 * released_records (pkt_pcap_stream_released gives both totals); before any release the window is the
 * capture.  Every count, offset, len and column the calls below report is the window's, as if its bytes
 * were a capture of their own: the records, counts and errors are pkt_pcap_index's over the window.  A
 * consumer that releases the records it is done with runs an unbounded capture in O(max_bytes) device
 * memory: push -> poll -> use the columns and the packets (pkt_pcap_stream_batch) -> release.  A stream
 * that never releases is one capture of at most max_bytes held whole.
 * open: a stream on `device` (its own ctx; pkt_pcap_stream_ctx gives it for the tuning knobs) with a
 * window of at most max_bytes (one device buffer) and `cap` records (<= 2^26; more are counted, not
 * parsed, until a release brings them below cap); `out` = the requested columns for cap records (slot
 * columns strided by cap), either all device memory of `device` (the parse writes them) or all pinned
 * host memory from pkt_host_alloc (each step's columns are exported over the link while the next bytes
 * copy in); step_bytes = new bytes that start a step at a push (0 = 4 MiB).
 * push: append n bytes (host memory; the caller may reuse it when push returns).  Pushes under 1 MiB
 * are gathered in a pinned staging ring of the stream and copied in 1 MiB pieces (or earlier, when a
 * step is due), without a wait per push; larger ones are copied from `bytes` and waited for.  A push of
 * more than pkt_pcap_stream_room bytes is refused (PKT_ERR_INVALID_ARG, nothing changes, the stream
 * goes on working).
 * room: *bytes = what a push can take now: max_bytes minus the window's bytes, staged ones included.
 * A record whose 16 + incl_len exceeds max_bytes - 24 can never complete inside the window: sizing
 * max_bytes above the largest record is the caller's business, and the stream does not detect it.
 * poll: a step over the bytes not yet indexed, then wait: *n_records = the window's records wholly inside
 * the bytes so far (a record running past them is not an error yet), their columns written; offsets /
 * lens (HOST, [cap], may be NULL) receive their (data offset in the window, incl_len).
 * finish: the capture is complete: a last step, the tail taken as pkt_pcap_index takes it (a record
 * running past the end = PKT_ERR_INVALID_ARG; a partial record header is ignored), then as poll.
 * release: the consumer is done with window records [0, n_records).  n_records <= min(c, cap), c = the
 * count the last poll returned (0 when there was none since open or since the last release that cut
 * anything); more, or any release after finish, is PKT_ERR_INVALID_ARG: nothing changes and the error
 * is not sticky.  n_records = 0 changes nothing and succeeds.  Otherwise the window is cut at p =
 * (offset + len) of window record n_records - 1 — the first uncounted record start when n_records = c,
 * the header of the first record counted but not parsed when n_records = cap < c: the new window is the
 * global header, then the old window's bytes [p, end); released_records += n_records, released_bytes +=
 * p - 24 (the capture's bytes, not the repeated global header); the index and the
 * columns restart at window record 0 and the next poll / finish reports the new window, records that
 * were past cap included (open with cap = B, poll, consume, release(B): cap is a batch size).  The
 * caller's column arrays are rewritten from index 0 and every pointer taken from pkt_pcap_stream_batch
 * is stale, as data, after a release: consume first, then release.  Blocking: it waits for the stream's
 * queued copies, steps and exports, moves the kept bytes down and leaves them to be indexed and parsed
 * again by the next step, so its cost grows with the bytes KEPT (one partial record when everything
 * polled is released), not with the bytes released.
 * batch: *batch = the window as of the last poll / finish, an indexed DEVICE batch: slab = the stream's
 * buffer, slab_len = the bytes that poll had indexed, offsets / lens = the device index, n = min(c, cap)
 * (n = 0 and slab_len = 0, pointers valid, before any poll and after a release).  The pointers stay
 * valid and their contents stable until the next push that starts a step, poll, release, finish or
 * close on the stream.  With the stream's device columns as chain columns this batch feeds
 * pkt_pcap_write, pkt_compare_batch, pkt_edit_batch, pkt_to_vec_batch, pkt_extract_fields and
 * pkt_set_fields* with no copy and no second parse.
 * Errors name the call in pkt_pcap_stream_last_error; after a HIP or capture error, every later call
 * returns it. */
typedef struct pkt_pcap_stream pkt_pcap_stream_t;
int         pkt_pcap_stream_open(int device, uint64_t max_bytes, uint64_t cap, int entry, const pkt_out_t *out,
                                 uint64_t step_bytes, pkt_pcap_stream_t **st);
int         pkt_pcap_stream_push(pkt_pcap_stream_t *st, const uint8_t *bytes, uint64_t n);
int         pkt_pcap_stream_poll(pkt_pcap_stream_t *st, uint64_t *n_records, uint64_t *offsets, uint32_t *lens);
int         pkt_pcap_stream_finish(pkt_pcap_stream_t *st, uint64_t *n_records, uint64_t *offsets, uint32_t *lens);
int         pkt_pcap_stream_release(pkt_pcap_stream_t *st, uint64_t n_records);
int         pkt_pcap_stream_room(const pkt_pcap_stream_t *st, uint64_t *bytes);
int         pkt_pcap_stream_released(const pkt_pcap_stream_t *st, uint64_t *records, uint64_t *bytes);
int         pkt_pcap_stream_batch(pkt_pcap_stream_t *st, pkt_batch_t *batch);
pkt_ctx_t  *pkt_pcap_stream_ctx(pkt_pcap_stream_t *st);
const char *pkt_pcap_stream_last_error(const pkt_pcap_stream_t *st);
int         pkt_pcap_stream_close(pkt_pcap_stream_t *st);

/* ---- multi-GPU: one process drives several devices ----
 * Every fast::parse_* is a pure function of one packet (fast.rs:5-227), so a batch splits into
 * contiguous shards, one per device, with no exchange inside the parse.  The only collective is
 * the gather of the per-packet tuples to a root device over RCCL (xGMI): one grouped
 * ncclSend / ncclRecv per shard (ncclCommInitAll over the device list; one communicator per
 * device, owned by the handle).  Each device has its own pkt_ctx and work stream; every call
 * below is asynchronous on those streams and returns after the launches (pkt_mgpu_synchronize
 * waits).  One host thread at a time per handle. */
typedef struct pkt_mgpu pkt_mgpu_t;
/* `devices`: ndev distinct HIP device ids; index 0..ndev-1 into this list is the "shard" id. */
int         pkt_mgpu_create(const int *devices, int ndev, pkt_mgpu_t **mg);
/* TEST MODE (not a transport to measure): a handle whose device list may repeat a device (e.g. device 0
 * listed 8 times: 8 shards, each with its own ctx and streams) and which holds no RCCL communicator:
 * every gather message that pkt_mgpu_create's handle sends by ncclSend/ncclRecv is a hipMemcpyAsync on
 * the sending shard's stream, ordered after the root's queued work and before the root's later work by
 * events.  It runs the N-shard code paths (per-shard issuing threads, shard offsets, multi-shard gather
 * plans and repack) on a one-GPU box; every other call behaves as for pkt_mgpu_create's handle. */
int         pkt_mgpu_create_virtual(const int *devices, int ndev, pkt_mgpu_t **mg);
int         pkt_mgpu_is_virtual(const pkt_mgpu_t *mg);
int         pkt_mgpu_destroy(pkt_mgpu_t *mg);
int         pkt_mgpu_ndev(const pkt_mgpu_t *mg);
/* The handle's last error; pkt_mgpu_last_error(NULL) = why this thread's last pkt_mgpu_create failed. */
const char *pkt_mgpu_last_error(const pkt_mgpu_t *mg);
/* The per-device ctx (tuning knobs, other batched calls) and work stream (a hipStream_t). */
pkt_ctx_t  *pkt_mgpu_ctx(pkt_mgpu_t *mg, int shard);
void       *pkt_mgpu_stream(pkt_mgpu_t *mg, int shard);
/* Parse shard i: batches[i] (resident on devices[i]) -> the packed output buffer shard_out[i]
 * (device memory of devices[i], pkt_out_packed(col_mask, batches[i].n) bytes). */
int pkt_mgpu_parse(pkt_mgpu_t *mg, const pkt_batch_t *batches, int entry, uint64_t col_mask,
                   void *const *shard_out);
/* `steps` consecutive pkt_mgpu_parse calls in one: step k parses batches[k*ndev + i] into the packed
 * buffer shard_out[k*ndev + i] on device i.  One host thread per device issues its device's launches,
 * round-robin over `streams` (1..4) streams of that device which start after, and are joined back
 * into, its work stream (steps are independent: different inputs, different outputs), so the launch
 * rate scales with the device count.  Asynchronous: returns after the launches. */
int pkt_mgpu_parse_steps(pkt_mgpu_t *mg, const pkt_batch_t *batches, int steps, int entry, uint64_t col_mask,
                         void *const *shard_out, int streams);
/* How the root's own pieces move in pkt_mgpu_gather / pkt_mgpu_parse_gather: 1 (default) = device
 * copies on the root's stream (an RCCL send to itself moved ~1 TB/s, the copy ~2 TB/s), 0 = RCCL
 * ncclSend / ncclRecv to itself inside the group like every other shard. */
int pkt_mgpu_set_root_copy(pkt_mgpu_t *mg, int enable);
/* Slot rows pkt_mgpu_parse_gather moves per shard: 0 (default) = each shard's largest n_hdrs, reduced
 * inside its parse kernel — the host waits once per device for it before issuing the gather; 1..16 =
 * that many rows for every shard (the caller's bound, >= every packet's n_hdrs; 16 always holds), so the
 * parse and the gather are queued with no host wait at all.  The largest n_hdrs is still reduced (when
 * n_hdrs is among the columns) and the next pkt_mgpu_synchronize returns PKT_ERR_GATHER_ROWS if the last
 * parse_gather had a packet with more headers than the fixed rows (its rows past them are unspecified in
 * recv although its n_hdrs counts them). */
int pkt_mgpu_set_gather_rows(pkt_mgpu_t *mg, int rows);
/* Gather bytes[i] of send[i] (device memory of devices[i]) into `recv` on devices[root] at
 * recv_off[i] (recv_off NULL: consecutive blocks, each rounded up to 256 B), `recv_len` bytes.
 * Grouped ncclSend/ncclRecv from the other devices; the root's own block per pkt_mgpu_set_root_copy. */
int pkt_mgpu_gather(pkt_mgpu_t *mg, int root, const void *const *send, const uint64_t *bytes,
                    void *recv, uint64_t recv_len, const uint64_t *recv_off);
/* pkt_mgpu_parse, then the gather of pkt_gather_plan(col_mask, ndev, n, rows, merge) into `recv` on
 * the root (recv_len >= its recv_bytes with rows NULL), where rows[i] = pkt_mgpu_set_gather_rows' count,
 * or by default shard i's largest n_hdrs when n_hdrs is among the columns (reduced inside each shard's
 * parse kernel; the host waits once per device, after every parse is queued), else all 16.  merge = 0
 * sends the plan's pieces as they are (<= 2 per shard).  merge = 1 sends the same <= 2 messages per
 * shard into a staging area the handle keeps on the root, then one repack kernel on the root's stream
 * places the merge = 1 plan's pieces (with the root copy on, the root's own pieces straight from its
 * shard buffer).  root_views (host array of ndev pkt_out_t, may be NULL) receives the column pointers
 * of each shard's tuples inside `recv` (merge = 0), or root_views[0] the single view of the whole batch
 * (merge = 1: what pkt_parse_batch over the whole batch would write). */
int pkt_mgpu_parse_gather(pkt_mgpu_t *mg, const pkt_batch_t *batches, int entry, uint64_t col_mask,
                          void *const *shard_out, int root, void *recv, uint64_t recv_len,
                          int merge, pkt_out_t *root_views);
int pkt_mgpu_synchronize(pkt_mgpu_t *mg);

#ifdef __cplusplus
}
#endif

#endif /* PKTGPU_H */
