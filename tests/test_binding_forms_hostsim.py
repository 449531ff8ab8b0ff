"""Every `_dev` method of elliptic_amd.Context against its host-buffer sibling, on the CPU build of
the device code (tests/hostsim), where device memory is host memory.

The binding writes each operation's argument list once, for both forms.  This runs the two public
methods of every pair on the same five items and asks for byte-equal results: an operand in the
wrong place, a missing `None` for an absent optional operand or a wrong width shows here, not on a
GPU.  A `_dev` method needs a tensor and a stream; the tensor is the stand-in `Dev` below (a shape
and an address, nothing else: a method that reads anything more fails here), the stream is the
null stream, as in the `dev_np` forms of the *_checks.py modules.

Items come from the generators of the *_checks.py modules on the user-defined curves (one short
domain, one Edwards domain, one Montgomery curve); on the presets (secp256k1, and p384 for a width
above 32 bytes) the engine's own host methods make keys and signatures.  Each call holds an item on
either side of its status wherever the operation has one, results are pre-filled with 0xA5, and
every optional operand (inf, inf1 / inf2, p1, out_err, out_status, out_pub, msg_off) is absent in
at least one call."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib, ints_to_be  # noqa: E402
from elliptic_amd.engine import FIELD_BYTES  # noqa: E402
import custom_domain_checks as CD  # noqa: E402
import custom_ecdh_checks as CH  # noqa: E402
import custom_ed_checks as CK  # noqa: E402
import custom_ed_ecdsa_checks as CE  # noqa: E402
import custom_mont_checks as CM  # noqa: E402
import custom_recover_checks as CR  # noqa: E402
import custom_sign_checks as CS  # noqa: E402
import custom_wire_checks as CW  # noqa: E402

N = 5
FILL = CW.FILL
PRESETS = ("secp256k1", "p384")
PRIME = {"secp256k1": 2 ** 256 - 2 ** 32 - 977, "p384": 2 ** 384 - 2 ** 128 - 2 ** 96 + 2 ** 32 - 1}
SHORT, EDWARDS, MONT = "brainpoolP256r1", "curve1174", "m221"
DEV_METHODS = sorted(name for name in dir(elliptic_amd.Context) if name.endswith("_dev"))


class Dev:
    """what a `_dev` method may read of a tensor: its shape and its address"""

    def __init__(self, a):
        assert isinstance(a, np.ndarray) and a.flags.c_contiguous
        self._a = a
        self.shape = a.shape

    def data_ptr(self):
        return self._a.ctypes.data


def T(a):
    return None if a is None else Dev(a)


def filled(*shapes):
    return [np.full(sh, FILL, np.uint8) for sh in shapes]


def mixed(st):
    """the call has an item on either side of its status"""
    assert len(set(np.asarray(st).reshape(-1).tolist())) > 1, st
    return st


def pick(st, must=()):
    """indices of N items of a larger batch, at least one with status 0 and one without"""
    st = np.asarray(st)
    zero, non = np.nonzero(st == 0)[0], np.nonzero(st != 0)[0]
    assert zero.size and non.size
    idx = []
    for i in list(must) + [zero[0], non[0]] + list(range(len(st))):
        if int(i) not in idx and len(idx) < N:
            idx.append(int(i))
    assert len(idx) == N
    return np.array(idx)


def take(bt, idx, *names):
    return [np.ascontiguousarray(bt[k][idx]) for k in names]


# ---- the items ------------------------------------------------------------------------------------

def preset_items(ctx, curve):
    """keys, signatures and encodings on a preset curve, made by the host methods: item 1 has a key
    off the curve, item 2 a wrong signature, item 3 a DER signature with a wrong tag (and a set
    infinity flag), item 4 a key with an unknown prefix"""
    B = FIELD_BYTES[curve]
    rng = np.random.default_rng(B)

    def scalars():
        a = rng.integers(0, 256, (N, B), dtype=np.uint8)
        a[:, 0] = 0                                     # below the order
        a[:, -1] |= 1                                   # and not zero
        return a
    d = types.SimpleNamespace(B=B, k=scalars(), k2=scalars(), nonce=scalars())
    d.h = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    d.pub, inf = ctx.mul_fixed(curve, d.k)
    d.pub2, inf2 = ctx.mul_fixed(curve, d.k2)
    assert not inf.any() and not inf2.any()
    d.bad = d.pub.copy()
    d.bad[1, -1] ^= 1
    d.flags = np.array([0, 0, 0, 1, 0], np.uint8)
    d.r, s, d.rec, ok = ctx.ecdsa_sign(curve, d.h, d.k, d.nonce)
    assert ok.all()
    d.s = s.copy()
    d.s[2, -1] ^= 1
    sigs = ctx.sig_to_der(curve, d.r, d.s)
    sigs[3] = b"\x31" + sigs[3][1:]
    d.der, d.lens = elliptic_amd.Context._pack_records(sigs)
    d.keys = {c: ctx.encode_points(curve, d.pub, compact=c) for c in (False, True)}
    for k in d.keys.values():
        k[4, 0] = 5
    d.r0 = d.r.copy()
    d.r0[1] = 0                                         # recovery: outside the engine's domain
    cand = ints_to_be(range(1, 33), B)                  # an abscissa without a point
    no_y = cand[np.nonzero(ctx.decompress(curve, cand, np.zeros(32, np.uint8))[1] == 0)[0][0]]
    d.v = np.ascontiguousarray(d.pub[:, :B])
    d.v[1] = no_y
    d.odd = np.ascontiguousarray(d.pub[:, -1] & 1)
    return d


def ed25519_items(ctx):
    rng = np.random.default_rng(25519)
    d = types.SimpleNamespace(secrets=rng.integers(0, 256, (N, 32), dtype=np.uint8))
    d.msgs2d = rng.integers(0, 256, (N, 17), dtype=np.uint8)
    d.ragged = [rng.integers(0, 256, 7 * i, dtype=np.uint8).tobytes() for i in range(N)]     # the first one empty
    d.flat = np.frombuffer(b"".join(d.ragged), np.uint8).copy()
    d.off = np.zeros(N + 1, np.uint64)
    d.off[1:] = np.cumsum([len(m) for m in d.ragged])
    d.sig2d, d.pub = ctx.eddsa_sign(d.msgs2d, d.secrets)
    d.sig_r, pub_r = ctx.eddsa_sign(d.ragged, d.secrets)
    assert (pub_r == d.pub).all()
    for sig in (d.sig2d, d.sig_r):
        sig[2, 5] ^= 1                                  # item 2: a wrong signature
    d.k = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    d.x = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    d.x[1] = 0                                          # the ladder ends at infinity
    return d


def short_items():
    spec = CD.curves()
    spec = next(s for s in spec if s["name"] == SHORT)
    d = types.SimpleNamespace(spec=spec, pl=CW.spec_of(SHORT)["pl"])
    xs, odd = CW.random_xs(CW.spec_of(SHORT), 12, 3)
    d.xs, d.odd = np.stack([CD.b32(x) for x in xs]), np.array(odd, np.uint8)
    d.wire = CW.wire_batch(CW.spec_of(SHORT), 40, 5)
    d.rec = CR.random_batch(CR.spec_of(SHORT), 20, 6)
    d.sup = CS.sup_batch(CS.spec_of(SHORT), 8, 7, 32, 0)
    d.det = CS.det_batch(CS.spec_of(SHORT), N, 8, "sha256", 32, 1)
    d.ecdh = CH.random_batch(CH.spec_of(SHORT), 20, 9)
    d.ecdh_wire = {c: CH.wire_batch(CH.spec_of(SHORT), d.ecdh, 20, c) for c in (False, True)}
    return d


def edwards_items():
    d = types.SimpleNamespace(spec=CE.spec_of(EDWARDS))
    d.key = CK.random_batch(CK.spec_of(EDWARDS), 8, 11, distinct=8)
    d.ver = CE.verify_batch(d.spec, 16, 12, distinct=16)
    d.sup = CE.sup_batch(d.spec, 8, 13, 32, 0, distinct=8)
    d.det = CE.det_batch(d.spec, N, 14, "sha256", 32, 1, distinct=N)
    return d


@pytest.fixture(scope="module")
def env():
    lib = _lib.load(build_hostsim(), optional=("ellgpu_probe_valu", "ellgpu_ctx_set_timing",
                                               "ellgpu_ctx_get_timing", "ellgpu_debug_field_op"))
    ctx = elliptic_amd.Context(0, lib_path=lib)
    ctx._stream = lambda: None                          # on this instance only: the null stream
    e = types.SimpleNamespace(ctx=ctx)
    e.presets = {c: preset_items(ctx, c) for c in PRESETS}
    e.ed = ed25519_items(ctx)
    e.short = short_items()
    e.short.cid = CD.define(ctx, e.short.spec)
    e.edw = edwards_items()
    e.edw.cid = CE.define(ctx, e.edw.spec)
    e.mont = CM.random_batch(CM.spec_of(MONT), N, 15)
    e.mont_cid = CM.define(ctx, CM.spec_of(MONT))
    yield e
    ctx.close()


# ---- one generator per _dev method: (label, the host method's results, the _dev method's) ------------

def case_mul_fixed_dev(e):
    for c, d in e.presets.items():
        o = filled((N, 2 * d.B), (N,))
        e.ctx.mul_fixed_dev(c, T(d.k), T(o[0]), T(o[1]))
        yield c, e.ctx.mul_fixed(c, d.k, out=filled((N, 2 * d.B), (N,))), o
    o = filled((N, 64), (N,))
    e.ctx.mul_fixed_dev(e.short.cid, T(e.short.det["d"]), T(o[0]), T(o[1]))
    yield SHORT, e.ctx.mul_fixed(e.short.cid, e.short.det["d"]), o


def case_mul_var_dev(e):
    for c, d in e.presets.items():
        o = filled((N, 2 * d.B), (N,))
        e.ctx.mul_var_dev(c, T(d.k2), T(d.bad), T(o[0]), T(o[1]))
        h = e.ctx.mul_var(c, d.k2, d.bad, out=filled((N, 2 * d.B), (N,)))
        mixed(h[1])
        yield c, h, o


def case_mul_add2_dev(e):
    for c, d in e.presets.items():
        for p1 in (d.bad, None):
            o = filled((N, 2 * d.B), (N,))
            e.ctx.mul_add2_dev(c, T(d.k), T(p1), T(d.k2), T(d.pub2), T(o[0]), T(o[1]))
            h = e.ctx.mul_add2(c, d.k, p1, d.k2, d.pub2)
            if p1 is not None:
                mixed(h[1])
            yield (c, p1 is None), h, o


def case_ecdsa_verify_dev(e):
    for c, d in e.presets.items():
        for status in (True, False):
            o = filled((N,), (N,))[:2 if status else 1]
            e.ctx.ecdsa_verify_dev(c, T(d.h), T(d.r), T(d.s), T(d.bad), T(o[0]), out_status=T(o[1]) if status else None)
            h = e.ctx.ecdsa_verify(c, d.h, d.r, d.s, d.bad, status=status)
            h = list(h) if status else [h]
            mixed(h[0])
            if status:
                assert h[1][1] == elliptic_amd.STATUS_OFF_CURVE
            yield (c, status), h, o
    d = e.short.wire
    args = take(d, pick(1 - d["known"].astype(np.uint8)), "h", "r", "s", "q")      # valid by construction, and disturbed
    o = filled((N,))
    e.ctx.ecdsa_verify_dev(e.short.cid, *map(T, args), T(o[0]), msg_bits=0)
    yield SHORT, [mixed(e.ctx.ecdsa_verify(e.short.cid, *args))], o


def case_ecdsa_sign_dev(e):
    for c, d in e.presets.items():
        nonce = d.nonce.copy()
        nonce[1] = 0                                    # the reference goes on to its next nonce
        for canonical in (False, True):
            o = filled((N, d.B), (N, d.B), (N,), (N,))
            e.ctx.ecdsa_sign_dev(c, T(d.h), T(d.k), T(nonce), *map(T, o), canonical=canonical)
            h = e.ctx.ecdsa_sign(c, d.h, d.k, nonce, canonical=canonical)
            mixed(h[3])
            yield (c, canonical), h, o


def case_ecdsa_sign_det_dev(e):
    for c, d in e.presets.items():
        o = filled((N, d.B), (N, d.B), (N,), (N,))
        e.ctx.ecdsa_sign_det_dev(c, T(d.h), T(d.k), *map(T, o), canonical=True)
        yield c, e.ctx.ecdsa_sign_det(c, d.h, d.k, canonical=True), o


def case_ecdsa_recover_dev(e):
    for c, d in e.presets.items():
        o = filled((N, 2 * d.B), (N,))
        e.ctx.ecdsa_recover_dev(c, T(d.h), T(d.r0), T(d.s), T(d.rec), T(o[0]), T(o[1]))
        h = e.ctx.ecdsa_recover(c, d.h, d.r0, d.s, d.rec)
        mixed(h[1])
        yield c, h, o


def case_decompress_dev(e):
    for c, d in e.presets.items():
        o = filled((N, 2 * d.B), (N,))
        e.ctx.decompress_dev(c, T(d.v), T(d.odd), T(o[0]), T(o[1]))
        h = e.ctx.decompress(c, d.v, d.odd)
        mixed(h[1])
        yield c, h, o


def case_decode_points_dev(e):
    for c, d in e.presets.items():
        for compact, keys in d.keys.items():
            o = filled((N, 2 * d.B), (N,))
            e.ctx.decode_points_dev(c, T(keys), T(o[0]), T(o[1]))
            h = e.ctx.decode_points(c, keys)
            mixed(h[1])
            yield (c, compact), h, o


def case_encode_points_dev(e):
    for c, d in e.presets.items():
        for compact in (False, True):
            o = filled((N, 1 + d.B if compact else 1 + 2 * d.B))
            e.ctx.encode_points_dev(c, T(d.pub), compact, T(o[0]))
            yield (c, compact), [e.ctx.encode_points(c, d.pub, compact)], o


def case_validate_dev(e):
    for c, d in e.presets.items():
        for inf, check_order in ((d.flags, True), (None, False)):
            o = filled((N,))
            e.ctx.validate_dev(c, T(d.bad), T(inf), check_order, T(o[0]))
            yield (c, inf is None), [mixed(e.ctx.validate(c, d.bad, inf, check_order))], o


def case_point_add_dev(e):
    for c, d in e.presets.items():
        xy2 = d.pub2.copy()
        xy2[0] = d.bad[0]                               # a doubling
        y = int.from_bytes(d.bad[2, d.B:].tobytes(), "big")
        xy2[2] = d.bad[2]                               # P + (-P): the point at infinity
        xy2[2, d.B:] = np.frombuffer((PRIME[c] - y).to_bytes(d.B, "big"), np.uint8)
        for inf1, inf2 in ((None, None), (d.flags, None), (None, d.flags[::-1].copy())):
            o = filled((N, 2 * d.B), (N,))
            e.ctx.point_add_dev(c, T(d.bad), T(xy2), T(o[0]), T(o[1]), inf1=T(inf1), inf2=T(inf2))
            h = e.ctx.point_add(c, d.bad, xy2, inf1, inf2)
            mixed(h[1])
            yield (c, inf1 is None, inf2 is None), h, o


def case_ecdsa_verify_wire_dev(e):
    for c, d in e.presets.items():
        for compact, keys in d.keys.items():
            o = filled((N,), (N,))[:1 if compact else 2]
            e.ctx.ecdsa_verify_wire_dev(c, T(d.h), T(d.der), T(d.lens), T(keys), T(o[0]),
                                        out_err=None if compact else T(o[1]))
            h = e.ctx.ecdsa_verify_wire(c, d.h, (d.der, d.lens), keys)
            mixed(h[0]), mixed(h[1])
            yield (c, compact), list(h)[:len(o)], o


def case_x25519_dev(e):
    o = filled((N, 32), (N,))
    e.ctx.x25519_dev(T(e.ed.k), T(e.ed.x), T(o[0]), T(o[1]))
    h = e.ctx.x25519(e.ed.k, e.ed.x)
    mixed(h[1])
    yield "curve25519", h, o


def case_eddsa_sign_dev(e):
    d = e.ed
    o = filled((N, 64), (N, 32))
    e.ctx.eddsa_sign_dev(T(d.secrets), T(d.msgs2d), 17, T(o[0]), T(o[1]))
    yield "fixed length", e.ctx.eddsa_sign(d.msgs2d, d.secrets), o
    o = filled((N, 64))
    e.ctx.eddsa_sign_dev(T(d.secrets), T(d.flat), 0, T(o[0]), msg_off=T(d.off))
    yield "offsets, no out_pub", e.ctx.eddsa_sign(d.ragged, d.secrets)[:1], o


def case_eddsa_verify_dev(e):
    d = e.ed
    o = filled((N,), (N,))
    e.ctx.eddsa_verify_dev(T(d.msgs2d), 17, T(d.sig2d), T(d.pub), T(o[0]), T(o[1]))
    h = e.ctx.eddsa_verify(d.msgs2d, d.sig2d, d.pub)
    mixed(h[0])
    yield "fixed length", h, o
    o = filled((N,))
    e.ctx.eddsa_verify_dev(T(d.flat), 0, T(d.sig_r), T(d.pub), T(o[0]), msg_off=T(d.off))
    h = e.ctx.eddsa_verify(d.ragged, d.sig_r, d.pub)
    mixed(h[0])
    yield "offsets, no out_err", h[:1], o


# user-defined short curves

def case_custom_decompress_dev(e):
    d, cid = e.short, e.short.cid
    idx = pick(e.ctx.custom_decompress(cid, d.xs, d.odd)[1])
    x, odd = take({"x": d.xs, "odd": d.odd}, idx, "x", "odd")
    o = filled((N, 64), (N,))
    e.ctx.custom_decompress_dev(cid, T(x), T(odd), T(o[0]), T(o[1]))
    h = e.ctx.custom_decompress(cid, x, odd, out=filled((N, 64), (N,)))
    mixed(h[1])
    yield SHORT, h, o


def case_custom_decode_points_dev(e):
    for form in ("compressed", "full"):
        w = e.short.wire[form]
        enc, = take(w, pick(w["err"]), "keys")
        o = filled((N, 64), (N,))
        e.ctx.custom_decode_points_dev(e.short.cid, T(enc), T(o[0]), T(o[1]))
        h = e.ctx.custom_decode_points(e.short.cid, enc, out=filled((N, 64), (N,)))
        mixed(h[1])
        yield form, h, o


def case_custom_verify_wire_dev(e):
    d, cid = e.short.wire, e.short.cid
    for form, want_err in (("compressed", False), ("full", True)):
        w = d[form]
        idx = pick(w["err"], must=[CW.KEY_PREFIX, CW.SIG_DER, CW.KEY_OFF])
        h_, = take(d, idx, "h")
        der, lens, keys = take(w, idx, "der", "lens", "keys")
        o = filled((N,), (N,))[:2 if want_err else 1]
        e.ctx.custom_verify_wire_dev(cid, T(h_), T(der), T(lens), T(keys), T(o[0]), out_err=T(o[1]) if want_err else None)
        h = e.ctx.custom_verify_wire(cid, h_, (der, lens), keys, out=filled((N,), (N,)), want_err=want_err)
        mixed(h[0])
        yield form, list(h)[:len(o)], o


def case_custom_recover_dev(e):
    bt, cid = e.short.rec, e.short.cid
    args = take(bt, pick(bt["st"]), "h", "r", "s", "j")
    o = filled((N, 64), (N,))
    e.ctx.custom_recover_dev(cid, *map(T, args), T(o[0]), T(o[1]))
    h = e.ctx.custom_recover(cid, *args, out=filled((N, 64), (N,)))
    mixed(h[1])
    yield SHORT, h, o


def _sign_cases(e, d, cid, host, dev, host_det, dev_det):
    args = take(d.sup, pick(d.sup["ok"]), "h", "d", "k")
    for canonical in (False, True):
        o = filled((N, 32), (N, 32), (N,), (N,))
        dev(cid, *map(T, args), *map(T, o), canonical=canonical)
        h = host(cid, *args, canonical=canonical, out=filled((N, 32), (N, 32), (N,), (N,)))
        mixed(h[3])
        yield ("supplied", canonical), h, o
    args = take(d.det, np.arange(N), "h", "d")
    for drbg_hash in (elliptic_amd.engine.HASH_SHA256, elliptic_amd.engine.HASH_SHA512):
        o = filled((N, 32), (N, 32), (N,), (N,))
        dev_det(cid, *map(T, args), *map(T, o), drbg_hash=drbg_hash, canonical=True)
        h = host_det(cid, *args, drbg_hash=drbg_hash, canonical=True, out=filled((N, 32), (N, 32), (N,), (N,)))
        assert h[3].all()
        if drbg_hash == elliptic_amd.engine.HASH_SHA256:
            assert (h[0] == d.det["r"]).all() and (h[1] == d.det["s"]).all()      # drbg_hash reaches the library
        else:
            assert (h[0] != d.det["r"]).any()
        yield ("det", drbg_hash), h, o


def case_custom_sign_dev(e):
    c = e.ctx
    return (t for t in _sign_cases(e, e.short, e.short.cid, c.custom_sign, c.custom_sign_dev, c.custom_sign_det,
                                   c.custom_sign_det_dev) if t[0][0] == "supplied")


def case_custom_sign_det_dev(e):
    c = e.ctx
    return (t for t in _sign_cases(e, e.short, e.short.cid, c.custom_sign, c.custom_sign_dev, c.custom_sign_det,
                                   c.custom_sign_det_dev) if t[0][0] == "det")


def case_custom_derive_dev(e):
    bt, cid = e.short.ecdh, e.short.cid
    args = take(bt, pick(bt["st"]), "priv", "pub")
    o = filled((N, 32), (N,))
    e.ctx.custom_derive_dev(cid, T(args[0]), T(args[1]), T(o[0]), T(o[1]))
    h = e.ctx.custom_derive(cid, *args, out=filled((N, 32), (N,)))
    mixed(h[1])
    yield SHORT, h, o


def case_custom_derive_wire_dev(e):
    bt, cid = e.short.ecdh, e.short.cid
    for compact, want_err in ((True, True), (False, False)):
        enc, st = e.short.ecdh_wire[compact][:2]
        idx = pick(st)
        priv, enc = np.ascontiguousarray(bt["priv"][idx]), np.ascontiguousarray(enc[idx])
        o = filled((N, 32), (N,), (N,))[:3 if want_err else 2]
        e.ctx.custom_derive_wire_dev(cid, T(priv), T(enc), *map(T, o))
        h = e.ctx.custom_derive_wire(cid, priv, enc, out=filled((N, 32), (N,), (N,))[:len(o)], want_err=want_err)
        mixed(h[1])
        yield compact, list(h)[:len(o)], o


def case_custom_validate_dev(e):
    bt, cid = e.short.ecdh, e.short.cid
    idx = pick(bt["vst"], must=np.nonzero((bt["st"] == 1) & (bt["inf"] == 0))[0][:1])      # a key off the curve, not flagged
    xy, inf = take(bt, idx, "pub", "inf")
    for flags, check_order in ((inf, True), (None, False)):
        o = filled((N,))
        e.ctx.custom_validate_dev(cid, T(xy), T(flags), check_order, T(o[0]))
        yield flags is None, [mixed(e.ctx.custom_validate(cid, xy, flags, check_order, out=filled((N,))))], o


def case_custom_encode_points_dev(e):
    xy = np.ascontiguousarray(e.short.ecdh["pub"][:N])
    for compact in (False, True):
        shape = (N, 1 + e.short.pl if compact else 1 + 2 * e.short.pl)
        o = filled(shape)
        e.ctx.custom_encode_points_dev(e.short.cid, T(xy), compact, T(o[0]))
        yield compact, [e.ctx.custom_encode_points(e.short.cid, xy, compact, out=filled(shape))], o


# user-defined Montgomery curves

def case_custom_mont_ladder_dev(e):
    o = filled((N, 32), (N,))
    e.ctx.custom_mont_ladder_dev(e.mont_cid, T(e.mont["k"]), T(e.mont["x"]), T(o[0]), T(o[1]))
    h = e.ctx.custom_mont_ladder(e.mont_cid, e.mont["k"], e.mont["x"], out=filled((N, 32), (N,)))
    mixed(h[1])
    yield MONT, h, o


def case_custom_mont_validate_dev(e):
    o = filled((N,))
    e.ctx.custom_mont_validate_dev(e.mont_cid, T(e.mont["x"]), T(o[0]))
    yield MONT, [mixed(e.ctx.custom_mont_validate(e.mont_cid, e.mont["x"], out=filled((N,))))], o


def case_custom_mont_derive_dev(e):
    o = filled((N, 32), (N,))
    e.ctx.custom_mont_derive_dev(e.mont_cid, T(e.mont["k"]), T(e.mont["x"]), T(o[0]), T(o[1]))
    h = e.ctx.custom_mont_derive(e.mont_cid, e.mont["k"], e.mont["x"], out=filled((N, 32), (N,)))
    mixed(h[1])
    yield MONT, h, o


# user-defined Edwards curves

def case_custom_ed_decompress_dev(e):
    bt, cid = e.edw.key, e.edw.cid
    v, odd = take(bt, np.arange(N), "v", "odd")
    for from_y in (False, True):
        o = filled((N, 64), (N,))
        e.ctx.custom_ed_decompress_dev(cid, T(v), T(odd), from_y, T(o[0]), T(o[1]))
        h = e.ctx.custom_ed_decompress(cid, v, odd, from_y, out=filled((N, 64), (N,)))
        mixed(h[1])
        yield from_y, h, o


def case_custom_ed_decode_points_dev(e):
    for form, w in e.edw.key["wire"].items():
        enc = np.ascontiguousarray(w["enc"][:N])
        o = filled((N, 64), (N,))
        e.ctx.custom_ed_decode_points_dev(e.edw.cid, T(enc), T(o[0]), T(o[1]))
        h = e.ctx.custom_ed_decode_points(e.edw.cid, enc, out=filled((N, 64), (N,)))
        mixed(h[1])
        yield form, h, o


def case_custom_ed_validate_dev(e):
    bt = e.edw.key
    xy = np.ascontiguousarray(bt["xy"][:N])
    for order in (None, bt["order"]):
        o = filled((N,))
        e.ctx.custom_ed_validate_dev(e.edw.cid, T(xy), order, T(o[0]))
        yield order is None, [mixed(e.ctx.custom_ed_validate(e.edw.cid, xy, order, out=filled((N,))))], o


def case_custom_ed_derive_dev(e):
    k, xy = take(e.edw.key, np.arange(N), "k", "xy")
    o = filled((N, 32), (N,))
    e.ctx.custom_ed_derive_dev(e.edw.cid, T(k), T(xy), T(o[0]), T(o[1]))
    h = e.ctx.custom_ed_derive(e.edw.cid, k, xy, out=filled((N, 32), (N,)))
    mixed(h[1])
    yield EDWARDS, h, o


def case_custom_ed_derive_wire_dev(e):
    for (form, w), want_err in zip(e.edw.key["wire"].items(), (True, False)):
        k, enc = take(w, np.arange(N), "k", "enc")
        o = filled((N, 32), (N,), (N,))[:3 if want_err else 2]
        e.ctx.custom_ed_derive_wire_dev(e.edw.cid, T(k), T(enc), *map(T, o))
        h = e.ctx.custom_ed_derive_wire(e.edw.cid, k, enc, out=filled((N, 32), (N,), (N,))[:len(o)], want_err=want_err)
        mixed(h[1])
        yield form, list(h)[:len(o)], o


def case_custom_ed_encode_points_dev(e):
    bt = e.edw.key
    xy = np.ascontiguousarray(bt["xy"][:N])
    for compact in (False, True):
        shape = (N, 1 + bt["pl"] if compact else 1 + 2 * bt["pl"])
        o = filled(shape)
        e.ctx.custom_ed_encode_points_dev(e.edw.cid, T(xy), compact, T(o[0]))
        yield compact, [e.ctx.custom_ed_encode_points(e.edw.cid, xy, compact, out=filled(shape))], o


def case_custom_ed_verify_dev(e):
    bt, cid = e.edw.ver, e.edw.cid
    args = take(bt, pick(1 - bt["ok"], must=np.nonzero(bt["st"] == 2)[0][:1]), "h", "r", "s", "q")
    for status in (True, False):
        o = filled((N,), (N,))[:2 if status else 1]
        e.ctx.custom_ed_verify_dev(cid, *map(T, args), T(o[0]), out_status=T(o[1]) if status else None)
        h = e.ctx.custom_ed_verify(cid, *args, status=status, out=filled((N,), (N,))[:len(o)])
        h = list(h) if status else [h]
        mixed(h[0])
        if status:
            mixed(h[1])
        yield status, h, o


def case_custom_ed_sign_dev(e):
    c = e.ctx
    return (t for t in _sign_cases(e, e.edw, e.edw.cid, c.custom_ed_sign, c.custom_ed_sign_dev, c.custom_ed_sign_det,
                                   c.custom_ed_sign_det_dev) if t[0][0] == "supplied")


def case_custom_ed_sign_det_dev(e):
    c = e.ctx
    return (t for t in _sign_cases(e, e.edw, e.edw.cid, c.custom_ed_sign, c.custom_ed_sign_dev, c.custom_ed_sign_det,
                                   c.custom_ed_sign_det_dev) if t[0][0] == "det")


CASES = {name[len("case_"):]: fn for name, fn in list(globals().items()) if name.startswith("case_")}


def test_every_dev_method_has_a_case():
    """the methods under test are Context's own list: a new _dev twin without a case fails here"""
    assert len(DEV_METHODS) >= 38
    assert set(CASES) == set(DEV_METHODS)


@pytest.mark.parametrize("method", DEV_METHODS)
def test_dev_form_equals_host_form(env, method):
    assert method in CASES, "no case for Context.%s" % method
    ran = 0
    for label, host, dev in CASES[method](env):
        assert len(host) == len(dev) and len(dev) > 0, (method, label)
        for i, (a, b) in enumerate(zip(host, dev)):
            assert a.dtype == b.dtype == np.uint8 and a.shape == b.shape, (method, label, i)
            assert a.tobytes() == b.tobytes(), (method, label, i, a, b)
        ran += 1
    assert ran > 0
