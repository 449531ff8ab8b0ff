"""The parameter block of a user-defined curve (csrc/fp_rt.h RtField, built by csrc/rt_define.h) is
compared byte for byte when a definition is registered, so the bytes are part of the contract.
tests/golden/rt_blocks.json records them -- before the definition code left the engine's class
template -- for every curve of the custom fixtures (short, Edwards, wire, ECDSA domains and their
plain curves) and for a plain curve over each modulus of rt_field_checks.MODULI_P; the blocks built
today must equal them.  `PYTHONPATH=. python tests/test_rt_blocks_hostsim.py` writes the fixture again."""
import ctypes
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import custom_domain_checks as CD  # noqa: E402
import custom_wire_checks as CW  # noqa: E402
import parity_checks as PC  # noqa: E402
import rt_field_checks as RT  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rt_blocks.json")
I = CD.I


def cases():
    """label -> (Context method, its arguments)"""
    out = {}
    for s in PC.custom_curves():
        out["short:" + s["name"]] = ("define_short", (I(s["p"]), I(s["a"]), I(s["b"])))
    for s in PC.custom_edwards_curves():
        out["edwards:" + s["name"]] = ("define_edwards", (I(s["p"]), I(s["a"]), I(s["d"])))
    for s in CW.curves():
        out["wire:" + s["name"]] = ("define_short_domain", tuple(CD.params(s))) if CW.is_domain(s) else ("define_short", CW.pab(s))
    for s in CD.curves():
        out["ecdsa:" + s["name"]] = ("define_short_domain", tuple(CD.params(s)))
        out["ecdsa-plain:" + s["name"]] = ("define_short", tuple(CD.params(s)[:3]))
    for p in RT.MODULI_P:                                  # a = -3, 0 and 2 in turn: the three a_kind values
        out["modulus:%x" % p] = ("define_short", (p, (p - 3, 0, 2)[len(out) % 3] % p, 7 % p))
    return out


def blocks(hs):
    fn = hs.hs_rt_block
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    got = {}
    for label, (method, args) in cases().items():
        c = elliptic_amd.Context(0, lib_path=hs)           # (a context holds sixteen definitions)
        cid = getattr(c, method)(*args)
        buf = ctypes.create_string_buffer(4096)
        size = fn(c._ctx, cid, buf, len(buf))
        assert 0 < size <= len(buf), label
        got[label] = buf.raw[:size].hex()
        c.close()
    return got


@pytest.fixture(scope="module")
def hs():
    return _lib.load(build_hostsim(), optional=("ellgpu_probe_valu", "ellgpu_ctx_set_timing",
                                                "ellgpu_ctx_get_timing", "ellgpu_debug_field_op"))


def test_rt_blocks_are_the_recorded_bytes(hs):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = blocks(hs)
    assert sorted(got) == sorted(want)
    assert len(got) >= 40 and any(len(set(b)) > 2 for b in got.values())
    for label in want:
        assert got[label] == want[label], label


if __name__ == "__main__":
    lib = _lib.load(build_hostsim(), optional=("ellgpu_probe_valu", "ellgpu_ctx_set_timing",
                                               "ellgpu_ctx_get_timing", "ellgpu_debug_field_op"))
    with open(GOLDEN, "w") as fh:
        json.dump(blocks(lib), fh, indent=0, sort_keys=True)
        fh.write("\n")
