"""The two forms of every batch entry point on the CPU build (tests/hostsim): the host-buffer form
(ellgpu_X, staged and pipelined by the engine) and the device-pointer form (ellgpu_X_dev, which
takes host memory on this build) must compute the same bytes, with every optional operand present
and absent, on the small-call path (n <= 8, the hostsim quantum) and the pipelined one.  And the
(rc, ellgpu_last_error()) pair of each invalid call, host and device form, is pinned."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import custom_domain_checks as CD  # noqa: E402

SIZES = [1, 8, 9, 41, 203]          # as test_host_pipeline_chunks: small call, its edge, 1..several chunks
P25519 = 2 ** 255 - 19


@pytest.fixture(scope="module")
def hs():
    return _lib.load(build_hostsim(), optional=("ellgpu_probe_valu", "ellgpu_ctx_set_timing",
                                                "ellgpu_ctx_get_timing", "ellgpu_debug_field_op"))


@pytest.fixture(scope="module")
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    spec = next(s for s in CD.curves() if s["name"] == "brainpoolP256r1")
    c.domain = CD.define(c, spec)
    c.plain = c.define_short(*CD.params(spec)[:3])    # the same (p, a, b) without n and G
    yield c
    c.close()


class Out:
    """an output buffer of the call, pre-filled so that bytes left unwritten show"""
    def __init__(self, *shape, dtype=np.uint8):
        self.shape, self.dtype = shape, dtype


def call(hs, ctx, name, args):
    """hs.name(ctx, *args) with every Out replaced by a fresh buffer: (rc, last_error, outputs)"""
    outs, cargs = [], []
    for a in args:
        if isinstance(a, Out):
            buf = np.full(a.shape, 0xA5, a.dtype)
            outs.append(buf)
            cargs.append(buf.ctypes.data)
        elif isinstance(a, np.ndarray):
            cargs.append(a.ctypes.data)
        else:
            cargs.append(a)
    rc = getattr(hs, name)(ctx._ctx, *cargs)
    return rc, hs.ellgpu_last_error().decode(), outs


def rnd_bytes(rng, n, w):
    return rng.integers(0, 256, (n, w), dtype=np.uint8)


def short_cases(ctx, curve, n, rng):
    """(label, entry point, args) for a preset short curve; inputs partly valid, partly not"""
    cid = elliptic_amd.CURVE_ID[curve]
    B, NB = elliptic_amd.FIELD_BYTES[curve], elliptic_amd.ORDER_BYTES[curve]
    d, k, k2, hsh = (rnd_bytes(rng, n, NB) for _ in range(4))
    if curve == "p521":
        d[:, 0] &= 1
    pts, _ = ctx.mul_fixed(curve, d)
    rev = pts[::-1].copy()
    inf = (rng.integers(0, 4, n) == 0).astype(np.uint8)
    inf2 = (rng.integers(0, 4, n) == 0).astype(np.uint8)
    r, s, recid, ok = ctx.ecdsa_sign(curve, hsh, d, k2)
    h2 = hsh.copy()
    h2[::3, 0] ^= 1
    r2 = r.copy()
    r2[1::5, 0] ^= 0x80
    stride = 2 * NB + 9
    der = np.zeros((n, stride), np.uint8)
    der_len = np.zeros(n, np.uint32)
    assert hs_call(ctx, "ellgpu_sig_to_der", cid, n, r2, s, der, stride, der_len) == 0
    der_len[2::7] -= 1
    enc = np.concatenate([np.full((n, 1), 4, np.uint8), pts], axis=1)
    enc[3::4, 0] = 2 + (pts[3::4, 2 * B - 1] & 1)
    enc[5::6, 1] ^= 1
    EL = 2 * B + 1
    odd = (pts[:, 2 * B - 1] & 1).copy()
    odd[::4] ^= 1
    xs = np.ascontiguousarray(pts[:, :B])
    cases = [
        ("mul_fixed", (cid, n, k, Out(n, 2 * B), Out(n))),
        ("mul_var", (cid, n, k, pts, Out(n, 2 * B), Out(n))),
        ("mul_add2", (cid, n, k, rev, k2, pts, Out(n, 2 * B), Out(n))),
        ("mul_add2", (cid, n, k, None, k2, pts, Out(n, 2 * B), Out(n))),
        ("ecdsa_verify", (cid, n, h2, NB, 0, r2, s, pts, Out(n), Out(n))),
        ("ecdsa_verify", (cid, n, h2, NB, 0, r2, s, pts, Out(n), None)),
        ("ecdsa_verify", (cid, n, h2, NB, 8 * NB - 3, r2, s, pts, Out(n), Out(n))),
        ("ecdsa_sign", (cid, n, hsh, NB, 0, d, k2, 1, Out(n, NB), Out(n, NB), Out(n), Out(n))),
        ("ecdsa_sign", (cid, n, hsh, NB, 0, d, k2, 0, Out(n, NB), Out(n, NB), Out(n), Out(n))),
        ("ecdsa_sign_det", (cid, n, hsh, NB, 0, d, 1, Out(n, NB), Out(n, NB), Out(n), Out(n))),
        ("ecdsa_recover", (cid, n, h2, NB, r2, s, recid, Out(n, 2 * B), Out(n))),
        ("decompress", (cid, n, xs, odd, Out(n, 2 * B), Out(n))),
        ("decode_points", (cid, n, enc, EL, Out(n, 2 * B), Out(n))),
        ("encode_points", (cid, n, pts, 0, Out(n, EL))),
        ("encode_points", (cid, n, pts, 1, Out(n, B + 1))),
        ("validate", (cid, n, pts, inf, 1, Out(n))),
        ("validate", (cid, n, rev, None, 0, Out(n))),
        ("point_add", (cid, n, pts, inf, rev, inf2, Out(n, 2 * B), Out(n))),
        ("point_add", (cid, n, pts, None, rev, inf2, Out(n, 2 * B), Out(n))),
        ("point_add", (cid, n, pts, inf, rev, None, Out(n, 2 * B), Out(n))),
        ("point_add", (cid, n, pts, None, pts, None, Out(n, 2 * B), Out(n))),
        ("sig_from_der", (cid, n, der, stride, der_len, Out(n, NB), Out(n, NB), Out(n))),
        ("sig_to_der", (cid, n, r2, s, Out(n, stride), stride, Out(n, dtype=np.uint32))),
        ("ecdsa_verify_wire", (cid, n, h2, NB, 0, der, stride, der_len, enc, EL, Out(n), Out(n))),
        ("ecdsa_verify_wire", (cid, n, h2, NB, 0, der, stride, der_len, enc, EL, Out(n), None)),
    ]
    return cases


def hs_call(ctx, name, *args):
    return getattr(ctx._lib, name)(ctx._ctx, *[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args])


def domain_cases(ctx, n, rng):
    """a user-defined ECDSA domain (brainpoolP256r1's) and the plain curve with its (p, a, b)"""
    spec = next(s for s in CD.curves() if s["name"] == "brainpoolP256r1")
    h, r, s, q, _ = CD.random_batch(spec, n, seed=int(rng.integers(1 << 30)))
    k, k2 = rnd_bytes(rng, n, 32), rnd_bytes(rng, n, 32)
    rev = q[::-1].copy()
    inf = (rng.integers(0, 4, n) == 0).astype(np.uint8)
    dom, plain = ctx.domain, ctx.plain
    return [
        ("mul_fixed", (dom, n, k, Out(n, 64), Out(n))),
        ("mul_add2", (dom, n, k, None, k2, q, Out(n, 64), Out(n))),
        ("mul_add2", (dom, n, k, rev, k2, q, Out(n, 64), Out(n))),
        ("mul_var", (dom, n, k, q, Out(n, 64), Out(n))),
        ("ecdsa_verify", (dom, n, h, 32, 0, r, s, q, Out(n), Out(n))),
        ("ecdsa_verify", (dom, n, h, 20, 0, r, s, q, Out(n), None)),
        ("mul_var", (plain, n, k, q, Out(n, 64), Out(n))),
        ("mul_add2", (plain, n, k, rev, k2, q, Out(n, 64), Out(n))),
        ("point_add", (plain, n, q, inf, rev, None, Out(n, 64), Out(n))),
        ("point_add", (dom, n, q, None, rev, inf, Out(n, 64), Out(n))),
    ]


def ed_cases(ctx, n, rng):
    """ed25519 points and EdDSA (uniform and offset messages), curve25519's ladder"""
    ed = elliptic_amd.CURVE_ID["ed25519"]
    k, k2, sec = (rnd_bytes(rng, n, 32) for _ in range(3))
    pts, _ = ctx.mul_fixed("ed25519", k2)
    rev = pts[::-1].copy()
    inf = (rng.integers(0, 4, n) == 0).astype(np.uint8)
    enc = np.zeros((n, 32), np.uint8)
    assert hs_call(ctx, "ellgpu_encode_points", ed, n, pts, 0, enc) == 0
    enc[::5, 3] ^= 1
    ys = np.ascontiguousarray(pts[:, 32:])
    odd = (pts[:, 31] & 1).copy()
    odd[::3] ^= 1
    lens = rng.integers(0, 90, n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    msgs = rng.integers(0, 256, max(int(off[-1]), 1), dtype=np.uint8)
    L = 17
    umsgs = rng.integers(0, 256, n * L, dtype=np.uint8)
    sig, pub = np.zeros((n, 64), np.uint8), np.zeros((n, 32), np.uint8)
    assert hs_call(ctx, "ellgpu_eddsa_sign", n, sec, msgs, off, 0, sig, pub) == 0
    sig[1::4, 5] ^= 1
    usig, upub = np.zeros((n, 64), np.uint8), np.zeros((n, 32), np.uint8)
    assert hs_call(ctx, "ellgpu_eddsa_sign", n, sec, umsgs, None, L, usig, upub) == 0
    umsgs[2::3] ^= 1
    xk = rnd_bytes(rng, n, 32)
    xs = rnd_bytes(rng, n, 32)
    return [
        ("mul_fixed", (ed, n, k, Out(n, 64), Out(n))),
        ("mul_var", (ed, n, k, pts, Out(n, 64), Out(n))),
        ("mul_add2", (ed, n, k, None, k2, pts, Out(n, 64), Out(n))),
        ("mul_add2", (ed, n, k, rev, k2, pts, Out(n, 64), Out(n))),
        ("decompress", (ed, n, ys, odd, Out(n, 64), Out(n))),
        ("decode_points", (ed, n, enc, 32, Out(n, 64), Out(n))),
        ("encode_points", (ed, n, pts, 0, Out(n, 32))),
        ("validate", (ed, n, pts, inf, 1, Out(n))),
        ("validate", (ed, n, pts, None, 0, Out(n))),
        ("point_add", (ed, n, pts, inf, rev, None, Out(n, 64), Out(n))),
        ("point_add", (ed, n, pts, None, rev, inf, Out(n, 64), Out(n))),
        ("eddsa_sign", (n, sec, msgs, off, 0, Out(n, 64), Out(n, 32))),
        ("eddsa_sign", (n, sec, umsgs, None, L, Out(n, 64), None)),
        ("eddsa_verify", (n, msgs, off, 0, sig, pub, Out(n), Out(n))),
        ("eddsa_verify", (n, umsgs, None, L, usig, upub, Out(n), None)),
        ("x25519_ladder", (n, xk, xs, Out(n, 32), Out(n))),
    ]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["secp256k1", "p224", "domain", "ed25519"])
def test_host_form_equals_dev_form(hs, ctx, kind, n):
    rng = np.random.default_rng(4321 + n + 1000 * len(kind))
    if kind == "domain":
        cases = domain_cases(ctx, n, rng)
    elif kind == "ed25519":
        cases = ed_cases(ctx, n, rng)
    else:
        cases = short_cases(ctx, kind, n, rng)
    for name, args in cases:
        rc_h, err_h, out_h = call(hs, ctx, "ellgpu_" + name, args)
        rc_d, err_d, out_d = call(hs, ctx, "ellgpu_" + name + "_dev", args + (None,))
        assert (rc_h, err_h) == (rc_d, err_d), (name, kind, n)
        assert rc_h == 0, (name, kind, n, err_h)
        for i, (a, b) in enumerate(zip(out_h, out_d)):
            assert a.tobytes() == b.tobytes(), (name, kind, n, "output %d" % i)


def _is_x25519_abscissa(x):
    u = int.from_bytes(bytes(x), "big") % P25519
    v = (u * u * u + 486662 * u * u + u) % P25519
    return v == 0 or pow(v, (P25519 - 1) // 2, P25519) == 1


@pytest.mark.parametrize("n", SIZES)
def test_x25519_derive_equals_ladder_dev(hs, ctx, n):
    """ellgpu_x25519_derive stages the optional out_bad operand: its points equal the device form's
    ladder, its status 1 marks the inputs that are no abscissa, 2 the infinities"""
    rng = np.random.default_rng(77 + n)
    k, x = rnd_bytes(rng, n, 32), rnd_bytes(rng, n, 32)
    x[::4, 1:] = 0                                     # small-order / low inputs among them
    rc, err, (ox, st) = call(hs, ctx, "ellgpu_x25519_derive", (n, k, x, Out(n, 32), Out(n)))
    assert rc == 0, err
    rc, err, (dx, dinf) = call(hs, ctx, "ellgpu_x25519_ladder_dev", (n, k, x, Out(n, 32), Out(n), None))
    assert rc == 0, err
    assert ox.tobytes() == dx.tobytes()
    bad = np.array([0 if _is_x25519_abscissa(x[i]) else 1 for i in range(n)], np.uint8)
    want = np.where(bad == 1, 1, np.where(dinf != 0, 2, 0)).astype(np.uint8)
    assert st.tobytes() == want.tobytes()


def error_cases(ctx):
    """(label, entry point, args) of invalid calls at n = 1 (n = 0 for 'n0'): an unknown curve id,
    refused curves, an unregistered custom id, each buffer NULL, all buffers NULL at n = 0, bad
    lengths.  The buffers are wide enough for every width tried (32-byte curves, hashes up to 72)."""
    rng = np.random.default_rng(99)
    b = lambda w: rnd_bytes(rng, 1, w)            # noqa: E731
    h, k, xy, der = b(72), b(32), b(64), b(80)
    dl = np.full(1, 8, np.uint32)
    off = np.array([0, 5], np.uint64)
    base = {
        "mul_fixed": (0, 1, k, Out(1, 64), Out(1)),
        "mul_var": (0, 1, k, xy, Out(1, 64), Out(1)),
        "mul_add2": (0, 1, k, xy, k, xy, Out(1, 64), Out(1)),
        "ecdsa_verify": (0, 1, h, 32, 0, k, k, xy, Out(1), Out(1)),
        "ecdsa_sign": (0, 1, h, 32, 0, k, k, 1, Out(1, 32), Out(1, 32), Out(1), Out(1)),
        "ecdsa_sign_det": (0, 1, h, 32, 0, k, 1, Out(1, 32), Out(1, 32), Out(1), Out(1)),
        "ecdsa_recover": (0, 1, h, 32, k, k, b(1), Out(1, 64), Out(1)),
        "decompress": (0, 1, k, b(1), Out(1, 64), Out(1)),
        "decode_points": (0, 1, der, 33, Out(1, 64), Out(1)),
        "encode_points": (0, 1, xy, 0, Out(1, 80)),
        "validate": (0, 1, xy, b(1), 1, Out(1)),
        "point_add": (0, 1, xy, b(1), xy, b(1), Out(1, 64), Out(1)),
        "sig_from_der": (0, 1, der, 80, dl, Out(1, 32), Out(1, 32), Out(1)),
        "sig_to_der": (0, 1, k, k, Out(1, 80), 80, Out(1, dtype=np.uint32)),
        "ecdsa_verify_wire": (0, 1, h, 32, 0, der, 80, dl, der, 65, Out(1), Out(1)),
        "eddsa_verify": (1, der, off, 0, xy, k, Out(1), Out(1)),
        "eddsa_sign": (1, k, der, off, 0, Out(1, 64), Out(1, 32)),
        "x25519_ladder": (1, k, k, Out(1, 32), Out(1)),
    }
    bad = {                                       # argument index: values
        "ecdsa_verify": {3: [0, -1, 40], 4: [-1, 8]},
        "ecdsa_sign": {3: [0, -1, 40], 4: [-1, 8]},
        "ecdsa_sign_det": {3: [0, -1, 40], 4: [-1, 8]},
        "ecdsa_recover": {3: [0, -1, 72]},
        "decode_points": {3: [0, 32, 65]},
        "sig_from_der": {3: [0]},
        "sig_to_der": {5: [0, 72]},
        "ecdsa_verify_wire": {3: [0, -1], 4: [-1], 6: [0], 9: [0]},
        "eddsa_verify": {3: [5]},
        "eddsa_sign": {4: [5]},
    }
    cases = []
    for name, args in base.items():
        curved = not name.startswith(("eddsa", "x25519"))
        ni = 1 if curved else 0
        cases.append(("ok", name, args))
        if curved:
            for cv in (99, -1, 6, 7, ctx.plain, ctx.domain, 31):
                cases.append(("curve %d" % cv if cv < 16 or cv > 30 else ("plain" if cv == ctx.plain else "domain"),
                              name, (cv,) + args[1:]))
        for i, a in enumerate(args):
            if isinstance(a, (np.ndarray, Out)):
                cases.append(("null %d" % i, name, args[:i] + (None,) + args[i + 1:]))
        cases.append(("n0", name, tuple(None if isinstance(a, (np.ndarray, Out)) else (0 if i == ni else a)
                                        for i, a in enumerate(args))))
        for i, vals in bad.get(name, {}).items():
            for v in vals:
                cases.append(("arg %d = %d" % (i, v), name, args[:i] + (v,) + args[i + 1:]))
    return cases


def test_error_table(hs, ctx):
    """the exact (rc, ellgpu_last_error()) of every case of error_cases, host and device form: which
    check wins where several fail, and where the two forms differ (a host call with n = 0 never
    reaches the device form's checks, except EdDSA's)"""
    got = {}
    for label, name, args in error_cases(ctx):
        for form, extra in (("", ()), ("_dev", (None,))):
            rc, err, _ = call(hs, ctx, "ellgpu_" + name + form, args + extra)
            got["%s%s: %s" % (name, form, label)] = (rc, err if rc else "")
    assert got == ERRORS


# recorded from the engine before its host-buffer wrappers shared one staging helper; kept as is
ERRORS = {
    'mul_fixed: ok': (0, ''),
    'mul_fixed_dev: ok': (0, ''),
    'mul_fixed: curve 99': (-2, 'unknown curve id'),
    'mul_fixed_dev: curve 99': (-2, 'unknown curve id'),
    'mul_fixed: curve -1': (-2, 'unknown curve id'),
    'mul_fixed_dev: curve -1': (-2, 'unknown curve id'),
    'mul_fixed: curve 6': (0, ''),
    'mul_fixed_dev: curve 6': (0, ''),
    'mul_fixed: curve 7': (-5, 'curve25519 has no affine fixed-base form; use x25519_ladder'),
    'mul_fixed_dev: curve 7': (-5, 'curve25519 has no affine fixed-base form; use x25519_ladder'),
    'mul_fixed: plain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'mul_fixed_dev: plain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'mul_fixed: domain': (0, ''),
    'mul_fixed_dev: domain': (0, ''),
    'mul_fixed: curve 31': (-2, 'unknown curve id'),
    'mul_fixed_dev: curve 31': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'mul_fixed: null 2': (-2, 'null pointer'),
    'mul_fixed_dev: null 2': (-2, 'null pointer'),
    'mul_fixed: null 3': (-2, 'null pointer'),
    'mul_fixed_dev: null 3': (-2, 'null pointer'),
    'mul_fixed: null 4': (-2, 'null pointer'),
    'mul_fixed_dev: null 4': (-2, 'null pointer'),
    'mul_fixed: n0': (0, ''),
    'mul_fixed_dev: n0': (0, ''),
    'mul_var: ok': (0, ''),
    'mul_var_dev: ok': (0, ''),
    'mul_var: curve 99': (-2, 'unknown curve id'),
    'mul_var_dev: curve 99': (-2, 'unknown curve id'),
    'mul_var: curve -1': (-2, 'unknown curve id'),
    'mul_var_dev: curve -1': (-2, 'unknown curve id'),
    'mul_var: curve 6': (0, ''),
    'mul_var_dev: curve 6': (0, ''),
    'mul_var: curve 7': (-5, 'curve25519 is x-only; use x25519_ladder'),
    'mul_var_dev: curve 7': (-5, 'curve25519 is x-only; use x25519_ladder'),
    'mul_var: plain': (0, ''),
    'mul_var_dev: plain': (0, ''),
    'mul_var: domain': (0, ''),
    'mul_var_dev: domain': (0, ''),
    'mul_var: curve 31': (-2, 'unknown curve id'),
    'mul_var_dev: curve 31': (-2, 'unknown curve id'),
    'mul_var: null 2': (-2, 'null pointer'),
    'mul_var_dev: null 2': (-2, 'null pointer'),
    'mul_var: null 3': (-2, 'null pointer'),
    'mul_var_dev: null 3': (-2, 'null pointer'),
    'mul_var: null 4': (-2, 'null pointer'),
    'mul_var_dev: null 4': (-2, 'null pointer'),
    'mul_var: null 5': (-2, 'null pointer'),
    'mul_var_dev: null 5': (-2, 'null pointer'),
    'mul_var: n0': (0, ''),
    'mul_var_dev: n0': (0, ''),
    'mul_add2: ok': (0, ''),
    'mul_add2_dev: ok': (0, ''),
    'mul_add2: curve 99': (-2, 'unknown curve id'),
    'mul_add2_dev: curve 99': (-2, 'unknown curve id'),
    'mul_add2: curve -1': (-2, 'unknown curve id'),
    'mul_add2_dev: curve -1': (-2, 'unknown curve id'),
    'mul_add2: curve 6': (0, ''),
    'mul_add2_dev: curve 6': (0, ''),
    'mul_add2: curve 7': (-5, 'Not supported on Montgomery curve'),
    'mul_add2_dev: curve 7': (-5, 'Not supported on Montgomery curve'),
    'mul_add2: plain': (0, ''),
    'mul_add2_dev: plain': (0, ''),
    'mul_add2: domain': (0, ''),
    'mul_add2_dev: domain': (0, ''),
    'mul_add2: curve 31': (-2, 'unknown curve id'),
    'mul_add2_dev: curve 31': (-2, 'unknown curve id'),
    'mul_add2: null 2': (-2, 'null pointer'),
    'mul_add2_dev: null 2': (-2, 'null pointer'),
    'mul_add2: null 3': (0, ''),
    'mul_add2_dev: null 3': (0, ''),
    'mul_add2: null 4': (-2, 'null pointer'),
    'mul_add2_dev: null 4': (-2, 'null pointer'),
    'mul_add2: null 5': (-2, 'null pointer'),
    'mul_add2_dev: null 5': (-2, 'null pointer'),
    'mul_add2: null 6': (-2, 'null pointer'),
    'mul_add2_dev: null 6': (-2, 'null pointer'),
    'mul_add2: null 7': (-2, 'null pointer'),
    'mul_add2_dev: null 7': (-2, 'null pointer'),
    'mul_add2: n0': (0, ''),
    'mul_add2_dev: n0': (0, ''),
    'ecdsa_verify: ok': (0, ''),
    'ecdsa_verify_dev: ok': (0, ''),
    'ecdsa_verify: curve 99': (-2, 'unknown curve id'),
    'ecdsa_verify_dev: curve 99': (-2, 'unknown curve id'),
    'ecdsa_verify: curve -1': (-2, 'unknown curve id'),
    'ecdsa_verify_dev: curve -1': (-2, 'unknown curve id'),
    'ecdsa_verify: curve 6': (-5, 'ECDSA verify is implemented for the short Weierstrass presets'),
    'ecdsa_verify_dev: curve 6': (-5, 'ECDSA verify is implemented for the short Weierstrass presets'),
    'ecdsa_verify: curve 7': (-5, 'ECDSA verify is implemented for the short Weierstrass presets'),
    'ecdsa_verify_dev: curve 7': (-5, 'ECDSA verify is implemented for the short Weierstrass presets'),
    'ecdsa_verify: plain': (-5, 'ECDSA verify on a user-defined curve needs its domain (ellgpu_curve_define_short_domain)'),
    'ecdsa_verify_dev: plain': (-5, 'ECDSA verify on a user-defined curve needs its domain (ellgpu_curve_define_short_domain)'),
    'ecdsa_verify: domain': (0, ''),
    'ecdsa_verify_dev: domain': (0, ''),
    'ecdsa_verify: curve 31': (-2, 'unknown curve id'),
    'ecdsa_verify_dev: curve 31': (-5, 'ECDSA verify on a user-defined curve needs its domain (ellgpu_curve_define_short_domain)'),
    'ecdsa_verify: null 2': (-2, 'null pointer'),
    'ecdsa_verify_dev: null 2': (-2, 'null pointer'),
    'ecdsa_verify: null 5': (-2, 'null pointer'),
    'ecdsa_verify_dev: null 5': (-2, 'null pointer'),
    'ecdsa_verify: null 6': (-2, 'null pointer'),
    'ecdsa_verify_dev: null 6': (-2, 'null pointer'),
    'ecdsa_verify: null 7': (-2, 'null pointer'),
    'ecdsa_verify_dev: null 7': (-2, 'null pointer'),
    'ecdsa_verify: null 8': (-2, 'null pointer'),
    'ecdsa_verify_dev: null 8': (-2, 'null pointer'),
    'ecdsa_verify: null 9': (0, ''),
    'ecdsa_verify_dev: null 9': (0, ''),
    'ecdsa_verify: n0': (0, ''),
    'ecdsa_verify_dev: n0': (0, ''),
    'ecdsa_verify: arg 3 = 0': (-2, 'bad hash_len'),
    'ecdsa_verify_dev: arg 3 = 0': (-2, 'bad hash_len / msg_bits'),
    'ecdsa_verify: arg 3 = -1': (-2, 'bad hash_len'),
    'ecdsa_verify_dev: arg 3 = -1': (-2, 'bad hash_len / msg_bits'),
    'ecdsa_verify: arg 3 = 40': (0, ''),
    'ecdsa_verify_dev: arg 3 = 40': (0, ''),
    'ecdsa_verify: arg 4 = -1': (-2, 'bad hash_len / msg_bits'),
    'ecdsa_verify_dev: arg 4 = -1': (-2, 'bad hash_len / msg_bits'),
    'ecdsa_verify: arg 4 = 8': (0, ''),
    'ecdsa_verify_dev: arg 4 = 8': (0, ''),
    'ecdsa_sign: ok': (0, ''),
    'ecdsa_sign_dev: ok': (0, ''),
    'ecdsa_sign: curve 99': (-2, 'unknown curve id'),
    'ecdsa_sign_dev: curve 99': (-2, 'unknown curve id'),
    'ecdsa_sign: curve -1': (-2, 'unknown curve id'),
    'ecdsa_sign_dev: curve -1': (-2, 'unknown curve id'),
    'ecdsa_sign: curve 6': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_dev: curve 6': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign: curve 7': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_dev: curve 7': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign: plain': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_dev: plain': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign: domain': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_dev: domain': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign: curve 31': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_dev: curve 31': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign: null 2': (-2, 'null pointer'),
    'ecdsa_sign_dev: null 2': (-2, 'null pointer'),
    'ecdsa_sign: null 5': (-2, 'null pointer'),
    'ecdsa_sign_dev: null 5': (-2, 'null pointer'),
    'ecdsa_sign: null 6': (-2, 'null pointer'),
    'ecdsa_sign_dev: null 6': (-2, 'null pointer'),
    'ecdsa_sign: null 8': (-2, 'null pointer'),
    'ecdsa_sign_dev: null 8': (-2, 'null pointer'),
    'ecdsa_sign: null 9': (-2, 'null pointer'),
    'ecdsa_sign_dev: null 9': (-2, 'null pointer'),
    'ecdsa_sign: null 10': (-2, 'null pointer'),
    'ecdsa_sign_dev: null 10': (-2, 'null pointer'),
    'ecdsa_sign: null 11': (-2, 'null pointer'),
    'ecdsa_sign_dev: null 11': (-2, 'null pointer'),
    'ecdsa_sign: n0': (0, ''),
    'ecdsa_sign_dev: n0': (0, ''),
    'ecdsa_sign: arg 3 = 0': (-2, 'bad hash_len'),
    'ecdsa_sign_dev: arg 3 = 0': (-2, 'bad hash_len / msg_bits'),
    'ecdsa_sign: arg 3 = -1': (-2, 'bad hash_len'),
    'ecdsa_sign_dev: arg 3 = -1': (-2, 'bad hash_len / msg_bits'),
    'ecdsa_sign: arg 3 = 40': (0, ''),
    'ecdsa_sign_dev: arg 3 = 40': (0, ''),
    'ecdsa_sign: arg 4 = -1': (-2, 'bad hash_len / msg_bits'),
    'ecdsa_sign_dev: arg 4 = -1': (-2, 'bad hash_len / msg_bits'),
    'ecdsa_sign: arg 4 = 8': (0, ''),
    'ecdsa_sign_dev: arg 4 = 8': (0, ''),
    'ecdsa_sign_det: ok': (0, ''),
    'ecdsa_sign_det_dev: ok': (0, ''),
    'ecdsa_sign_det: curve 99': (-2, 'unknown curve id'),
    'ecdsa_sign_det_dev: curve 99': (-2, 'unknown curve id'),
    'ecdsa_sign_det: curve -1': (-2, 'unknown curve id'),
    'ecdsa_sign_det_dev: curve -1': (-2, 'unknown curve id'),
    'ecdsa_sign_det: curve 6': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_det_dev: curve 6': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_det: curve 7': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_det_dev: curve 7': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_det: plain': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_det_dev: plain': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_det: domain': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_det_dev: domain': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_det: curve 31': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_det_dev: curve 31': (-5, 'ECDSA sign is implemented for the short Weierstrass presets'),
    'ecdsa_sign_det: null 2': (-2, 'null pointer'),
    'ecdsa_sign_det_dev: null 2': (-2, 'null pointer'),
    'ecdsa_sign_det: null 5': (-2, 'null pointer'),
    'ecdsa_sign_det_dev: null 5': (-2, 'null pointer'),
    'ecdsa_sign_det: null 7': (-2, 'null pointer'),
    'ecdsa_sign_det_dev: null 7': (-2, 'null pointer'),
    'ecdsa_sign_det: null 8': (-2, 'null pointer'),
    'ecdsa_sign_det_dev: null 8': (-2, 'null pointer'),
    'ecdsa_sign_det: null 9': (-2, 'null pointer'),
    'ecdsa_sign_det_dev: null 9': (-2, 'null pointer'),
    'ecdsa_sign_det: null 10': (-2, 'null pointer'),
    'ecdsa_sign_det_dev: null 10': (-2, 'null pointer'),
    'ecdsa_sign_det: n0': (0, ''),
    'ecdsa_sign_det_dev: n0': (0, ''),
    'ecdsa_sign_det: arg 3 = 0': (-2, 'bad hash_len'),
    'ecdsa_sign_det_dev: arg 3 = 0': (-2, 'bad hash_len / msg_bits'),
    'ecdsa_sign_det: arg 3 = -1': (-2, 'bad hash_len'),
    'ecdsa_sign_det_dev: arg 3 = -1': (-2, 'bad hash_len / msg_bits'),
    'ecdsa_sign_det: arg 3 = 40': (0, ''),
    'ecdsa_sign_det_dev: arg 3 = 40': (0, ''),
    'ecdsa_sign_det: arg 4 = -1': (-2, 'bad hash_len / msg_bits'),
    'ecdsa_sign_det_dev: arg 4 = -1': (-2, 'bad hash_len / msg_bits'),
    'ecdsa_sign_det: arg 4 = 8': (0, ''),
    'ecdsa_sign_det_dev: arg 4 = 8': (0, ''),
    'ecdsa_recover: ok': (0, ''),
    'ecdsa_recover_dev: ok': (0, ''),
    'ecdsa_recover: curve 99': (-2, 'unknown curve id'),
    'ecdsa_recover_dev: curve 99': (-2, 'unknown curve id'),
    'ecdsa_recover: curve -1': (-2, 'unknown curve id'),
    'ecdsa_recover_dev: curve -1': (-2, 'unknown curve id'),
    'ecdsa_recover: curve 6': (-5, 'public-key recovery is an ECDSA (short Weierstrass) operation'),
    'ecdsa_recover_dev: curve 6': (-5, 'public-key recovery is an ECDSA (short Weierstrass) operation'),
    'ecdsa_recover: curve 7': (-5, 'public-key recovery is an ECDSA (short Weierstrass) operation'),
    'ecdsa_recover_dev: curve 7': (-5, 'public-key recovery is an ECDSA (short Weierstrass) operation'),
    'ecdsa_recover: plain': (-5, 'public-key recovery is an ECDSA (short Weierstrass) operation'),
    'ecdsa_recover_dev: plain': (-5, 'public-key recovery is an ECDSA (short Weierstrass) operation'),
    'ecdsa_recover: domain': (-5, 'public-key recovery is an ECDSA (short Weierstrass) operation'),
    'ecdsa_recover_dev: domain': (-5, 'public-key recovery is an ECDSA (short Weierstrass) operation'),
    'ecdsa_recover: curve 31': (-5, 'public-key recovery is an ECDSA (short Weierstrass) operation'),
    'ecdsa_recover_dev: curve 31': (-5, 'public-key recovery is an ECDSA (short Weierstrass) operation'),
    'ecdsa_recover: null 2': (-2, 'null pointer'),
    'ecdsa_recover_dev: null 2': (-2, 'null pointer'),
    'ecdsa_recover: null 4': (-2, 'null pointer'),
    'ecdsa_recover_dev: null 4': (-2, 'null pointer'),
    'ecdsa_recover: null 5': (-2, 'null pointer'),
    'ecdsa_recover_dev: null 5': (-2, 'null pointer'),
    'ecdsa_recover: null 6': (-2, 'null pointer'),
    'ecdsa_recover_dev: null 6': (-2, 'null pointer'),
    'ecdsa_recover: null 7': (-2, 'null pointer'),
    'ecdsa_recover_dev: null 7': (-2, 'null pointer'),
    'ecdsa_recover: null 8': (-2, 'null pointer'),
    'ecdsa_recover_dev: null 8': (-2, 'null pointer'),
    'ecdsa_recover: n0': (0, ''),
    'ecdsa_recover_dev: n0': (0, ''),
    'ecdsa_recover: arg 3 = 0': (-2, 'bad hash_len'),
    'ecdsa_recover_dev: arg 3 = 0': (-2, 'hash_len must be 1 .. twice the order width'),
    'ecdsa_recover: arg 3 = -1': (-2, 'bad hash_len'),
    'ecdsa_recover_dev: arg 3 = -1': (-2, 'hash_len must be 1 .. twice the order width'),
    'ecdsa_recover: arg 3 = 72': (-2, 'hash_len must be 1 .. twice the order width'),
    'ecdsa_recover_dev: arg 3 = 72': (-2, 'hash_len must be 1 .. twice the order width'),
    'decompress: ok': (0, ''),
    'decompress_dev: ok': (0, ''),
    'decompress: curve 99': (-2, 'unknown curve id'),
    'decompress_dev: curve 99': (-2, 'unknown curve id'),
    'decompress: curve -1': (-2, 'unknown curve id'),
    'decompress_dev: curve -1': (-2, 'unknown curve id'),
    'decompress: curve 6': (0, ''),
    'decompress_dev: curve 6': (0, ''),
    'decompress: curve 7': (-5, 'curve25519 points are x-only'),
    'decompress_dev: curve 7': (-5, 'curve25519 points are x-only'),
    'decompress: plain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'decompress_dev: plain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'decompress: domain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'decompress_dev: domain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'decompress: curve 31': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'decompress_dev: curve 31': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'decompress: null 2': (-2, 'null pointer'),
    'decompress_dev: null 2': (-2, 'null pointer'),
    'decompress: null 3': (-2, 'null pointer'),
    'decompress_dev: null 3': (-2, 'null pointer'),
    'decompress: null 4': (-2, 'null pointer'),
    'decompress_dev: null 4': (-2, 'null pointer'),
    'decompress: null 5': (-2, 'null pointer'),
    'decompress_dev: null 5': (-2, 'null pointer'),
    'decompress: n0': (0, ''),
    'decompress_dev: n0': (0, ''),
    'decode_points: ok': (0, ''),
    'decode_points_dev: ok': (0, ''),
    'decode_points: curve 99': (-2, 'unknown curve id'),
    'decode_points_dev: curve 99': (-2, 'unknown curve id'),
    'decode_points: curve -1': (-2, 'unknown curve id'),
    'decode_points_dev: curve -1': (-2, 'unknown curve id'),
    'decode_points: curve 6': (-2, 'ed25519 encodings are 32 bytes'),
    'decode_points_dev: curve 6': (-2, 'ed25519 encodings are 32 bytes'),
    'decode_points: curve 7': (-5, 'curve25519 points are x-only'),
    'decode_points_dev: curve 7': (-5, 'curve25519 points are x-only'),
    'decode_points: plain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'decode_points_dev: plain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'decode_points: domain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'decode_points_dev: domain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'decode_points: curve 31': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'decode_points_dev: curve 31': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'decode_points: null 2': (-2, 'null pointer'),
    'decode_points_dev: null 2': (-2, 'null pointer'),
    'decode_points: null 4': (-2, 'null pointer'),
    'decode_points_dev: null 4': (-2, 'null pointer'),
    'decode_points: null 5': (-2, 'null pointer'),
    'decode_points_dev: null 5': (-2, 'null pointer'),
    'decode_points: n0': (0, ''),
    'decode_points_dev: n0': (0, ''),
    'decode_points: arg 3 = 0': (-2, 'enc_len must be positive'),
    'decode_points_dev: arg 3 = 0': (-2, 'enc_len must be positive'),
    'decode_points: arg 3 = 32': (0, ''),
    'decode_points_dev: arg 3 = 32': (0, ''),
    'decode_points: arg 3 = 65': (0, ''),
    'decode_points_dev: arg 3 = 65': (0, ''),
    'encode_points: ok': (0, ''),
    'encode_points_dev: ok': (0, ''),
    'encode_points: curve 99': (-2, 'unknown curve id'),
    'encode_points_dev: curve 99': (-2, 'unknown curve id'),
    'encode_points: curve -1': (-2, 'unknown curve id'),
    'encode_points_dev: curve -1': (-2, 'unknown curve id'),
    'encode_points: curve 6': (0, ''),
    'encode_points_dev: curve 6': (0, ''),
    'encode_points: curve 7': (-5, 'curve25519 points are x-only'),
    'encode_points_dev: curve 7': (-5, 'curve25519 points are x-only'),
    'encode_points: plain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'encode_points_dev: plain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'encode_points: domain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'encode_points_dev: domain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'encode_points: curve 31': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'encode_points_dev: curve 31': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'encode_points: null 2': (-2, 'null pointer'),
    'encode_points_dev: null 2': (-2, 'null pointer'),
    'encode_points: null 4': (-2, 'null pointer'),
    'encode_points_dev: null 4': (-2, 'null pointer'),
    'encode_points: n0': (0, ''),
    'encode_points_dev: n0': (0, ''),
    'validate: ok': (0, ''),
    'validate_dev: ok': (0, ''),
    'validate: curve 99': (-2, 'unknown curve id'),
    'validate_dev: curve 99': (-2, 'unknown curve id'),
    'validate: curve -1': (-2, 'unknown curve id'),
    'validate_dev: curve -1': (-2, 'unknown curve id'),
    'validate: curve 6': (0, ''),
    'validate_dev: curve 6': (0, ''),
    'validate: curve 7': (-5, 'curve25519 points are x-only'),
    'validate_dev: curve 7': (-5, 'curve25519 points are x-only'),
    'validate: plain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'validate_dev: plain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'validate: domain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'validate_dev: domain': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'validate: curve 31': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'validate_dev: curve 31': (-5, 'not available on user-defined curves (scalar multiplication and point addition only)'),
    'validate: null 2': (-2, 'null pointer'),
    'validate_dev: null 2': (-2, 'null pointer'),
    'validate: null 3': (0, ''),
    'validate_dev: null 3': (0, ''),
    'validate: null 5': (-2, 'null pointer'),
    'validate_dev: null 5': (-2, 'null pointer'),
    'validate: n0': (0, ''),
    'validate_dev: n0': (0, ''),
    'point_add: ok': (0, ''),
    'point_add_dev: ok': (0, ''),
    'point_add: curve 99': (-2, 'unknown curve id'),
    'point_add_dev: curve 99': (-2, 'unknown curve id'),
    'point_add: curve -1': (-2, 'unknown curve id'),
    'point_add_dev: curve -1': (-2, 'unknown curve id'),
    'point_add: curve 6': (0, ''),
    'point_add_dev: curve 6': (0, ''),
    'point_add: curve 7': (-5, 'Not supported on Montgomery curve'),
    'point_add_dev: curve 7': (-5, 'Not supported on Montgomery curve'),
    'point_add: plain': (0, ''),
    'point_add_dev: plain': (0, ''),
    'point_add: domain': (0, ''),
    'point_add_dev: domain': (0, ''),
    'point_add: curve 31': (-2, 'unknown curve id'),
    'point_add_dev: curve 31': (-2, 'unknown curve id'),
    'point_add: null 2': (-2, 'null pointer'),
    'point_add_dev: null 2': (-2, 'null pointer'),
    'point_add: null 3': (0, ''),
    'point_add_dev: null 3': (0, ''),
    'point_add: null 4': (-2, 'null pointer'),
    'point_add_dev: null 4': (-2, 'null pointer'),
    'point_add: null 5': (0, ''),
    'point_add_dev: null 5': (0, ''),
    'point_add: null 6': (-2, 'null pointer'),
    'point_add_dev: null 6': (-2, 'null pointer'),
    'point_add: null 7': (-2, 'null pointer'),
    'point_add_dev: null 7': (-2, 'null pointer'),
    'point_add: n0': (0, ''),
    'point_add_dev: n0': (0, ''),
    'sig_from_der: ok': (0, ''),
    'sig_from_der_dev: ok': (0, ''),
    'sig_from_der: curve 99': (-2, 'unknown curve id'),
    'sig_from_der_dev: curve 99': (-2, 'unknown curve id'),
    'sig_from_der: curve -1': (-2, 'unknown curve id'),
    'sig_from_der_dev: curve -1': (-2, 'unknown curve id'),
    'sig_from_der: curve 6': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_from_der_dev: curve 6': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_from_der: curve 7': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_from_der_dev: curve 7': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_from_der: plain': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_from_der_dev: plain': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_from_der: domain': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_from_der_dev: domain': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_from_der: curve 31': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_from_der_dev: curve 31': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_from_der: null 2': (-2, 'null pointer'),
    'sig_from_der_dev: null 2': (-2, 'null pointer'),
    'sig_from_der: null 4': (-2, 'null pointer'),
    'sig_from_der_dev: null 4': (-2, 'null pointer'),
    'sig_from_der: null 5': (-2, 'null pointer'),
    'sig_from_der_dev: null 5': (-2, 'null pointer'),
    'sig_from_der: null 6': (-2, 'null pointer'),
    'sig_from_der_dev: null 6': (-2, 'null pointer'),
    'sig_from_der: null 7': (-2, 'null pointer'),
    'sig_from_der_dev: null 7': (-2, 'null pointer'),
    'sig_from_der: n0': (0, ''),
    'sig_from_der_dev: n0': (0, ''),
    'sig_from_der: arg 3 = 0': (-2, 'stride must be positive'),
    'sig_from_der_dev: arg 3 = 0': (-2, 'stride must be positive'),
    'sig_to_der: ok': (0, ''),
    'sig_to_der_dev: ok': (0, ''),
    'sig_to_der: curve 99': (-2, 'unknown curve id'),
    'sig_to_der_dev: curve 99': (-2, 'unknown curve id'),
    'sig_to_der: curve -1': (-2, 'unknown curve id'),
    'sig_to_der_dev: curve -1': (-2, 'unknown curve id'),
    'sig_to_der: curve 6': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_to_der_dev: curve 6': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_to_der: curve 7': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_to_der_dev: curve 7': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_to_der: plain': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_to_der_dev: plain': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_to_der: domain': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_to_der_dev: domain': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_to_der: curve 31': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_to_der_dev: curve 31': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'sig_to_der: null 2': (-2, 'null pointer'),
    'sig_to_der_dev: null 2': (-2, 'null pointer'),
    'sig_to_der: null 3': (-2, 'null pointer'),
    'sig_to_der_dev: null 3': (-2, 'null pointer'),
    'sig_to_der: null 4': (-2, 'null pointer'),
    'sig_to_der_dev: null 4': (-2, 'null pointer'),
    'sig_to_der: null 6': (-2, 'null pointer'),
    'sig_to_der_dev: null 6': (-2, 'null pointer'),
    'sig_to_der: n0': (0, ''),
    'sig_to_der_dev: n0': (0, ''),
    'sig_to_der: arg 5 = 0': (-2, 'stride must be at least 2 * order_bytes + 9'),
    'sig_to_der_dev: arg 5 = 0': (-2, 'stride must be at least 2 * order_bytes + 9'),
    'sig_to_der: arg 5 = 72': (-2, 'stride must be at least 2 * order_bytes + 9'),
    'sig_to_der_dev: arg 5 = 72': (-2, 'stride must be at least 2 * order_bytes + 9'),
    'ecdsa_verify_wire: ok': (0, ''),
    'ecdsa_verify_wire_dev: ok': (0, ''),
    'ecdsa_verify_wire: curve 99': (-2, 'unknown curve id'),
    'ecdsa_verify_wire_dev: curve 99': (-2, 'unknown curve id'),
    'ecdsa_verify_wire: curve -1': (-2, 'unknown curve id'),
    'ecdsa_verify_wire_dev: curve -1': (-2, 'unknown curve id'),
    'ecdsa_verify_wire: curve 6': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'ecdsa_verify_wire_dev: curve 6': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'ecdsa_verify_wire: curve 7': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'ecdsa_verify_wire_dev: curve 7': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'ecdsa_verify_wire: plain': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'ecdsa_verify_wire_dev: plain': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'ecdsa_verify_wire: domain': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'ecdsa_verify_wire_dev: domain': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'ecdsa_verify_wire: curve 31': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'ecdsa_verify_wire_dev: curve 31': (-5, 'ECDSA signatures belong to the short Weierstrass presets'),
    'ecdsa_verify_wire: null 2': (-2, 'null pointer'),
    'ecdsa_verify_wire_dev: null 2': (-2, 'null pointer'),
    'ecdsa_verify_wire: null 5': (-2, 'null pointer'),
    'ecdsa_verify_wire_dev: null 5': (-2, 'null pointer'),
    'ecdsa_verify_wire: null 7': (-2, 'null pointer'),
    'ecdsa_verify_wire_dev: null 7': (-2, 'null pointer'),
    'ecdsa_verify_wire: null 8': (-2, 'null pointer'),
    'ecdsa_verify_wire_dev: null 8': (-2, 'null pointer'),
    'ecdsa_verify_wire: null 10': (-2, 'null pointer'),
    'ecdsa_verify_wire_dev: null 10': (-2, 'null pointer'),
    'ecdsa_verify_wire: null 11': (0, ''),
    'ecdsa_verify_wire_dev: null 11': (0, ''),
    'ecdsa_verify_wire: n0': (0, ''),
    'ecdsa_verify_wire_dev: n0': (0, ''),
    'ecdsa_verify_wire: arg 3 = 0': (-2, 'bad hash_len'),
    'ecdsa_verify_wire_dev: arg 3 = 0': (-2, 'bad hash_len / stride / pub_len'),
    'ecdsa_verify_wire: arg 3 = -1': (-2, 'bad hash_len'),
    'ecdsa_verify_wire_dev: arg 3 = -1': (-2, 'bad hash_len / stride / pub_len'),
    'ecdsa_verify_wire: arg 4 = -1': (-2, 'bad hash_len / msg_bits'),
    'ecdsa_verify_wire_dev: arg 4 = -1': (-2, 'bad hash_len / msg_bits'),
    'ecdsa_verify_wire: arg 6 = 0': (-2, 'bad hash_len / stride / pub_len'),
    'ecdsa_verify_wire_dev: arg 6 = 0': (-2, 'bad hash_len / stride / pub_len'),
    'ecdsa_verify_wire: arg 9 = 0': (-2, 'bad hash_len / stride / pub_len'),
    'ecdsa_verify_wire_dev: arg 9 = 0': (-2, 'bad hash_len / stride / pub_len'),
    'eddsa_verify: ok': (0, ''),
    'eddsa_verify_dev: ok': (0, ''),
    'eddsa_verify: null 1': (-2, 'null message pointer'),
    'eddsa_verify_dev: null 1': (-2, 'null pointer'),
    'eddsa_verify: null 2': (0, ''),
    'eddsa_verify_dev: null 2': (0, ''),
    'eddsa_verify: null 4': (-2, 'null pointer'),
    'eddsa_verify_dev: null 4': (-2, 'null pointer'),
    'eddsa_verify: null 5': (-2, 'null pointer'),
    'eddsa_verify_dev: null 5': (-2, 'null pointer'),
    'eddsa_verify: null 6': (-2, 'null pointer'),
    'eddsa_verify_dev: null 6': (-2, 'null pointer'),
    'eddsa_verify: null 7': (0, ''),
    'eddsa_verify_dev: null 7': (0, ''),
    'eddsa_verify: n0': (-4, 'staging allocation failed'),
    'eddsa_verify_dev: n0': (0, ''),
    'eddsa_verify: arg 3 = 5': (0, ''),
    'eddsa_verify_dev: arg 3 = 5': (0, ''),
    'eddsa_sign: ok': (0, ''),
    'eddsa_sign_dev: ok': (0, ''),
    'eddsa_sign: null 1': (-2, 'null pointer'),
    'eddsa_sign_dev: null 1': (-2, 'null pointer'),
    'eddsa_sign: null 2': (-2, 'null message pointer'),
    'eddsa_sign_dev: null 2': (-2, 'null pointer'),
    'eddsa_sign: null 3': (0, ''),
    'eddsa_sign_dev: null 3': (0, ''),
    'eddsa_sign: null 5': (-2, 'null pointer'),
    'eddsa_sign_dev: null 5': (-2, 'null pointer'),
    'eddsa_sign: null 6': (0, ''),
    'eddsa_sign_dev: null 6': (0, ''),
    'eddsa_sign: n0': (-4, 'staging allocation failed'),
    'eddsa_sign_dev: n0': (0, ''),
    'eddsa_sign: arg 4 = 5': (0, ''),
    'eddsa_sign_dev: arg 4 = 5': (0, ''),
    'x25519_ladder: ok': (0, ''),
    'x25519_ladder_dev: ok': (0, ''),
    'x25519_ladder: null 1': (-2, 'null pointer'),
    'x25519_ladder_dev: null 1': (-2, 'null pointer'),
    'x25519_ladder: null 2': (-2, 'null pointer'),
    'x25519_ladder_dev: null 2': (-2, 'null pointer'),
    'x25519_ladder: null 3': (-2, 'null pointer'),
    'x25519_ladder_dev: null 3': (-2, 'null pointer'),
    'x25519_ladder: null 4': (-2, 'null pointer'),
    'x25519_ladder_dev: null 4': (-2, 'null pointer'),
    'x25519_ladder: n0': (0, ''),
    'x25519_ladder_dev: n0': (0, ''),
}
