"""Every type a prototype or a struct field of INTEGRATION.md's Rust block names is declared in the block (or is a
primitive): an opaque handle such as PktMeter that is used as `*mut PktMeter` but never declared would not compile, and
tests/test_rust_binding.py, which skips the `_p` structs, would not see it."""
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))
import rust_binding as rb  # noqa: E402

PRIMITIVES = {"u8", "u16", "u32", "u64", "i32", "f32", "usize", "c_int", "c_char", "c_void"}


def _used(types):
    out = set()
    for t in types:
        out |= set(re.findall(r"[A-Za-z_]\w*", t)) - {"const", "mut"}
    return out


def _check(code):
    declared = set(re.findall(r"pub struct (\w+)", code))
    fns, sts = rb.rust_functions(code), rb.rust_structs(code)
    used = _used(t for args, ret in fns.values() for t in [a[1] for a in args] + ([ret] if ret else []))
    used |= _used(t for fields in sts.values() for _, t in fields)
    missing = {t for t in used if not t.isdigit()} - PRIMITIVES - declared
    assert not missing, f"used but never declared: {sorted(missing)}"
    return declared


def test_every_type_of_the_integration_block_is_declared():
    md = open(os.path.join(REPO, "INTEGRATION.md")).read()
    declared = _check(rb.RUST_BLOCK.findall(md)[0])
    assert "PktMeter" in declared and "PktTunnel" in declared


def test_every_type_of_the_generated_block_is_declared():
    _check(rb.generate())
