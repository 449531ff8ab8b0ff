"""The calls of tests/test_entry_forms_hostsim.py, shared with tools/record_entry_forms.py (which
wrote tests/golden/entry_forms.json from them): every exported batch entry point, host and device
form, on every kind of curve id, in the cases that run no kernel -- and a few calls of n = 20 whose
per-kernel launch counts are compared."""
import ctypes
import glob
import os
import re

import numpy as np

from elliptic_amd import _lib

import custom_domain_checks as CD
import custom_ed_checks as CK
import custom_ed_ecdsa_checks as CE
import custom_mont_checks as CM

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "entry_forms.json")

# argument kinds: C curve id, N item count, I / i required / optional input buffer, O / o required /
# optional output buffer, (name, value) an integer argument -- hash_len, enc_len, stride, pub_len
# and der_stride are the lengths the zero-length cases set to 0
HL, MB = ("hash_len", 32), ("msg_bits", 0)
ENTRIES = {
    "mul_fixed": "CNIOO",
    "mul_var": "CNIIOO",
    "mul_add2": "CNIiIIOO",
    "ecdsa_verify": ["C", "N", "I", HL, MB, "I", "I", "I", "O", "o"],
    "ecdsa_sign": ["C", "N", "I", HL, MB, "I", "I", ("canonical", 1), "O", "O", "O", "O"],
    "ecdsa_sign_det": ["C", "N", "I", HL, MB, "I", ("canonical", 1), "O", "O", "O", "O"],
    "ecdsa_recover": ["C", "N", "I", HL, "I", "I", "I", "O", "O"],
    "decompress": "CNIIOO",
    "decode_points": ["C", "N", "I", ("enc_len", 33), "O", "O"],
    "encode_points": ["C", "N", "I", ("compact", 0), "O"],
    "validate": ["C", "N", "I", "i", ("check_order", 1), "O"],
    "point_add": "CNIiIiOO",
    "sig_from_der": ["C", "N", "I", ("stride", 80), "I", "O", "O", "O"],
    "sig_to_der": ["C", "N", "I", "I", "O", ("stride", 80), "O"],
    "ecdsa_verify_wire": ["C", "N", "I", HL, MB, "I", ("der_stride", 80), "I", "I", ("pub_len", 65), "O", "o"],
    "custom_decompress": "CNIIOO",
    "custom_decode_points": ["C", "N", "I", ("enc_len", 33), "O", "O"],
    "custom_verify_wire": ["C", "N", "I", HL, MB, "I", ("der_stride", 80), "I", "I", ("pub_len", 65), "O", "o"],
    "custom_recover": ["C", "N", "I", HL, "I", "I", "I", "O", "O"],
    "custom_sign": ["C", "N", "I", HL, MB, "I", "I", ("canonical", 1), "O", "O", "O", "O"],
    "custom_sign_det": ["C", "N", "I", HL, MB, "I", ("drbg_hash", 0), ("canonical", 1), "O", "O", "O", "O"],
    "custom_derive": "CNIIOO",
    "custom_derive_wire": ["C", "N", "I", "I", ("pub_len", 65), "O", "O", "o"],
    "custom_validate": ["C", "N", "I", "i", ("check_order", 1), "O"],
    "custom_encode_points": ["C", "N", "I", ("compact", 0), "O"],
    "custom_ed_decompress": ["C", "N", "I", "I", ("from_y", 0), "O", "O"],
    "custom_ed_decode_points": ["C", "N", "I", ("enc_len", 33), "O", "O"],
    "custom_ed_validate": ["C", "N", "I", ("order", None), "O"],      # (the order is a parameter, not a batch operand)
    "custom_ed_derive": "CNIIOO",
    "custom_ed_derive_wire": ["C", "N", "I", "I", ("pub_len", 65), "O", "O", "o"],
    "custom_ed_encode_points": ["C", "N", "I", ("compact", 0), "O"],
    "custom_ed_verify": ["C", "N", "I", HL, MB, "I", "I", "I", "O", "o"],
    "custom_ed_sign": ["C", "N", "I", HL, MB, "I", "I", ("canonical", 1), "O", "O", "O", "O"],
    "custom_ed_sign_det": ["C", "N", "I", HL, MB, "I", ("drbg_hash", 0), ("canonical", 1), "O", "O", "O", "O"],
    "custom_mont_ladder": "CNIIOO",
    "custom_mont_validate": "CNIO",
    "custom_mont_derive": "CNIIOO",
    # (the messages of EdDSA are optional: an empty batch of empty messages has none)
    "eddsa_verify": ["N", "i", "i", ("msg_len", 0), "I", "I", "O", "o"],
    "eddsa_sign": ["N", "I", "i", "i", ("msg_len", 0), "O", "o"],
    "x25519_ladder": "NIIOO",
}
ZERO = ("hash_len", "enc_len", "stride", "der_stride", "pub_len")


def load(path):
    """the CPU build with its launch probe bound"""
    lib = _lib.load(path, optional=("ellgpu_probe_valu", "ellgpu_ctx_set_timing", "ellgpu_ctx_get_timing",
                                    "ellgpu_debug_field_op"))
    lib.hs_launches.restype = ctypes.c_int
    lib.hs_launches.argtypes = [ctypes.c_char_p]
    lib.hs_launches_reset.restype = None
    return lib


def define_curves(ctx):
    """label -> curve id, in a fixed order of definition (user-defined ids count up from 16)"""
    spec = next(s for s in CD.curves() if s["name"] == "brainpoolP256r1")
    ids = {"secp256k1": 0, "ed25519": 6, "curve25519": 7}
    ids["short"] = ctx.define_short(*CD.params(spec)[:3])
    ids["short_domain"] = CD.define(ctx, spec)
    ids["edwards"] = CK.define(ctx, CK.spec_of("p13_d4"))
    ids["edwards_domain"] = CE.define(ctx, CE.spec_of("toy_p65521"))
    ids["mont"] = CM.define(ctx, CM.spec_of("toy_p23"))
    ids["unknown_preset"] = 99
    ids["unknown_custom"] = 31
    return ids


def _args(kinds, curve, n, null=(), zero=None):
    """the argument list of one call: buffers of 256 zero bytes (all of them absent at n = 0)"""
    out, nbuf = [], 0
    for k in kinds:
        if k == "C":
            out.append(curve)
        elif k == "N":
            out.append(n)
        elif k in ("I", "i", "O", "o"):
            out.append(None if n == 0 or nbuf in null else np.zeros(256, np.uint8))
            nbuf += 1
        else:
            out.append(0 if k[0] == zero else k[1])
    return out


def error_calls(ids):
    """(key, entry point, args) of every case: n = 0 with null buffers, n = 1 with the first required
    buffer null, n = 1 with one length set to 0"""
    calls = []
    for name, kinds in ENTRIES.items():
        kinds = list(kinds)
        for label, cid in (ids.items() if "C" in kinds else [("-", None)]):
            bufs = [k for k in kinds if k in ("I", "i", "O", "o")]
            cases = [("n0", _args(kinds, cid, 0)), ("null", _args(kinds, cid, 1, null=(bufs.index("I"),)))]
            cases += [("zero " + k[0], _args(kinds, cid, 1, zero=k[0])) for k in kinds if k[0] in ZERO]
            for case, args in cases:
                calls.append(("%s|%s|%s" % (name, label, case), name, args))
    return calls


def run(lib, ctx, name, form, args):
    """ellgpu_<name><form>(ctx, *args): (rc, message)"""
    cargs = [a.ctypes.data if isinstance(a, np.ndarray) else a for a in args]
    if form:
        cargs.append(None)                       # the stream
    rc = getattr(lib, "ellgpu_" + name + form)(ctx._ctx, *cargs)
    return rc, lib.ellgpu_last_error().decode() if rc else ""


def error_table(lib, ctx, ids):
    got = {}
    for key, name, args in error_calls(ids):
        for form in ("", "_dev"):
            got[key + ("|dev" if form else "|host")] = list(run(lib, ctx, name, form, args))
    return got


# ---- launch counts -------------------------------------------------------------------------------

def kernel_names():
    """every kernel's timing name: the NAME of the launch functors in elliptic_amd/csrc"""
    names = set()
    for path in glob.glob(os.path.join(os.path.dirname(HERE), "elliptic_amd", "csrc", "*.h")):
        with open(path) as f:
            for line in f:
                if "char* NAME =" in line:
                    names.update(re.findall(r'"(\w+)"', line))
    return sorted(names)


N_LAUNCH = 20        # above the CPU build's pipeline quantum of 8: several pipeline steps, a short tail


def launch_calls(ids):
    """(label, entry point, args, indices of the outputs): one call per family, n = 20, random
    operands (what a kernel computes on them is not the point: the two forms must agree on it)"""
    rng = np.random.default_rng(20)
    n = N_LAUNCH
    b = lambda w: rng.integers(0, 256, (n, w), dtype=np.uint8)          # noqa: E731
    out = lambda w=1: np.zeros((n, w), np.uint8)                        # noqa: E731
    der_len = np.full(n, 70, np.uint32)
    k1, k2, h, r, s, q, q2 = b(32), b(32), b(32), b(32), b(32), b(64), b(64)
    return [
        ("ecdsa_verify preset", "ecdsa_verify", [0, n, h, 32, 0, r, s, q, out(), out()]),
        ("ecdsa_verify domain", "ecdsa_verify", [ids["short_domain"], n, h, 32, 0, r, s, q, out(), out()]),
        ("mul_add2 p1", "mul_add2", [0, n, k1, q2, k2, q, out(64), out()]),
        ("mul_add2 no p1", "mul_add2", [0, n, k1, None, k2, q, out(64), out()]),
        ("custom_sign_det", "custom_sign_det", [ids["short_domain"], n, h, 32, 0, k1, 0, 1, out(32), out(32), out(), out()]),
        ("custom_ed_verify", "custom_ed_verify", [ids["edwards_domain"], n, h, 32, 0, r, s, q, out(), out()]),
        ("custom_mont_derive", "custom_mont_derive", [ids["mont"], n, k1, r, out(32), out()]),
        ("ecdsa_verify_wire", "ecdsa_verify_wire", [0, n, h, 32, 0, b(80), 80, der_len, b(65), 65, out(), out()]),
        ("eddsa_verify", "eddsa_verify", [n, b(17), None, 17, b(64), b(32), out(), out()]),
    ]


def launch_table(lib, ctx, ids):
    """label -> {form -> {kernel: launches}}, the host form first (its first call builds the curve's
    tables); and label -> the two forms' output bytes"""
    names = kernel_names()
    counts, results = {}, {}
    for label, name, args in launch_calls(ids):
        nin = len(ENTRIES[name]) - sum(1 for k in ENTRIES[name] if k in ("O", "o"))
        counts[label], results[label] = {}, {}
        for form in ("", "_dev"):
            call = [a.copy() if isinstance(a, np.ndarray) else a for a in args]
            lib.hs_launches_reset()
            rc, msg = run(lib, ctx, name, form, call)
            assert rc == 0, (label, form, msg)
            got = {k: lib.hs_launches(k.encode()) for k in names}
            counts[label]["dev" if form else "host"] = {k: v for k, v in got.items() if v}
            results[label]["dev" if form else "host"] = b"".join(a.tobytes() for a in call[nin:])
    return counts, results
