"""What every entry point that takes a pkt_batch_t says to a malformed one: the return code and the exact
pkt_ctx_last_error text, per entry point (parse, extract_fields, set_fields, to_vec, compare, pcap_write,
edit) and per malformed form of one 4-packet, 64-byte-stride batch on one ctx:

    offsets without lens, stride 0 with no offsets, a slab pointer off by one byte, a NULL slab with a
    non-zero slab_len.

The texts are the ones each entry point has always given; they differ between entry points (the rewrite
entry points say "null slab/chain column" and take an unaligned slab) and must go on doing so.  No call
here reaches a launch but one: pkt_to_vec_batch has no check after the batch's, so that it accepts an
unaligned slab can only be seen by its success (four packets whose status is not PKT_OK: nothing is
copied).  extract_fields and set_fields show the same by failing at the NEXT check, the field spec's."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

INVALID = -1
FORMS = ("offsets_without_lens", "stride_0", "slab_off_by_one", "null_slab")
REWRITE = {"offsets_without_lens": "offsets without lens", "stride_0": "stride 0",
           "slab_off_by_one": None, "null_slab": "null slab/chain column"}     # None: accepted
STRICT = {"offsets_without_lens": "offsets without lens", "stride_0": "stride 0",
          "slab_off_by_one": "slab not 16-byte aligned", "null_slab": "null slab"}
WANT = {"parse": STRICT, "compare": STRICT, "pcap_write": STRICT, "edit": STRICT,
        "extract_fields": REWRITE, "set_fields": REWRITE, "to_vec": REWRITE}


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    import pktgpu
    P = pktgpu.Parser(0)
    lib, n = P._lib, 4
    z8 = lambda k: torch.zeros(k, dtype=torch.uint8, device="cuda")  # noqa: E731
    t = dict(slab=z8(64 * n + 16), offsets=torch.zeros(n, dtype=torch.int64, device="cuda"),
             status=torch.ones(n, dtype=torch.uint8, device="cuda"),   # PKT_TRUNCATED: nothing to copy
             n_hdrs=z8(n), hdr_type=z8(16 * n), hdr_off=torch.zeros(16 * n, dtype=torch.int16, device="cuda"),
             payload_off=torch.zeros(n, dtype=torch.int16, device="cuda"),
             payload_len=torch.zeros(n, dtype=torch.int16, device="cuda"),
             dst=z8(64 * n), values=torch.zeros(n, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    return P, lib, t


def batch(lib, t, form):
    b = lib.PktBatch()
    b.slab, b.slab_len, b.stride, b.n = t["slab"].data_ptr(), 256, 64, 4
    if form == "offsets_without_lens":
        b.offsets = t["offsets"].data_ptr()
    elif form == "stride_0":
        b.stride = 0
    elif form == "slab_off_by_one":
        b.slab = t["slab"].data_ptr() + 1
    elif form == "null_slab":
        b.slab = None
    return b


def call(P, lib, t, entry, b, bad_spec=False):
    L, ctx, s, ref = P._L, P._ctx, P._stream(None), ctypes.byref
    good = batch(lib, t, None)
    out = lib.PktOut()
    parsed = lib.PktOut()
    for k in ("status", "n_hdrs", "hdr_type", "hdr_off", "payload_off", "payload_len"):
        setattr(parsed, k, t[k].data_ptr())
    chain = lib.PktChain(t["n_hdrs"].data_ptr(), t["hdr_type"].data_ptr(), t["hdr_off"].data_ptr())
    # Ether.etype, or (bad_spec) a field that ends past the header
    spec = (lib.PktFieldSpec * 1)(lib.PktFieldSpec(1, 0, 96, 200 if bad_spec else 111, 0))
    values = (ctypes.c_void_p * 1)(t["values"].data_ptr())
    if entry == "parse":
        return L.pkt_parse_batch(ctx, ref(b), 0, ref(out), s)
    if entry == "extract_fields":
        return L.pkt_extract_fields(ctx, ref(b), ref(chain), spec, 1, values, None, s)
    if entry == "set_fields":
        return L.pkt_set_fields(ctx, ref(b), ref(chain), spec, 1, values, s)
    if entry == "to_vec":
        return L.pkt_to_vec_batch(ctx, ref(b), ref(parsed), t["dst"].data_ptr(), 256, None, None, s)
    if entry == "compare":
        return L.pkt_compare_batch(ctx, ref(b), ref(good), None, None, 0, None, None, None, None, s)
    if entry == "pcap_write":
        return L.pkt_pcap_write(ctx, ref(b), None, 0, 0, 0, None, None, None, 0, None, None, None, None, None, s)
    assert entry == "edit"
    return L.pkt_edit_batch(ctx, ref(b), ref(parsed), None, 0, None, 0, None, t["dst"].data_ptr(), 256, None, 64,
                            None, None, None, s)


@pytest.mark.parametrize("entry", sorted(WANT))
def test_refusals(env, entry):
    P, lib, t = env
    for form in FORMS:
        want = WANT[entry][form]
        b = batch(lib, t, form)
        if want is not None:
            assert call(P, lib, t, entry, b) == INVALID, (entry, form)
            assert P._L.pkt_ctx_last_error(P._ctx) == want.encode(), (entry, form)
        elif entry == "to_vec":
            assert call(P, lib, t, entry, b) == 0, (entry, form)
            import torch
            torch.cuda.synchronize()
            assert not t["dst"].any()
        else:  # accepted: the next check refuses
            assert call(P, lib, t, entry, b, bad_spec=True) == INVALID, (entry, form)
            assert P._L.pkt_ctx_last_error(P._ctx) == b"bad field spec", (entry, form)


def test_second_side_of_compare(env):
    """pkt_compare_batch applies the same rules to b after a."""
    P, lib, t = env
    good = batch(lib, t, None)
    for form in FORMS:
        bad = batch(lib, t, form)
        rc = P._L.pkt_compare_batch(P._ctx, ctypes.byref(good), ctypes.byref(bad), None, None, 0, None, None, None,
                                    None, P._stream(None))
        assert rc == INVALID and P._L.pkt_ctx_last_error(P._ctx) == STRICT[form].encode(), form
