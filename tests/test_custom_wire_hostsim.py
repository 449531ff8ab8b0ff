"""Wire formats on user-defined short curves (ellgpu_custom_decompress / _custom_decode_points /
_custom_verify_wire) on the CPU: the hostsim build of the device code (tests/hostsim) against the
reference's recorded answers (tests/golden/custom_wire.json), against pointFromX / decodePoint
restated over Python integers, and against ellgpu_ecdsa_verify and the C oracle on random batches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import custom_domain_checks as CD  # noqa: E402
import custom_wire_checks as CW  # noqa: E402

NAMES = [c["name"] for c in CW.curves()]
DOMAINS = [c["name"] for c in CW.curves() if CW.is_domain(c)]
# one curve of each kind of root: a^((p+1)/4), and Tonelli-Shanks with p - 1 = q 2^s, s = 2, 3, 32, 96
ROOTS = {"brainpoolP256r1": 1, "secp224k1": 2, "plain_s3": 3, "plain_s32": 32, "p224_user": 96}
SIZES = [1, 8, 9, 41, 203]             # the hostsim small-call and chunk edges (test_hostsim_forms.py)
FORMS = ["host", "dev_np"]


@pytest.fixture(scope="module")
def hs():
    return _lib.load(build_hostsim(), optional=("ellgpu_probe_valu", "ellgpu_ctx_set_timing",
                                                "ellgpu_ctx_get_timing", "ellgpu_debug_field_op"))


@pytest.fixture(scope="module")
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


def test_curve_set():
    assert len(NAMES) == 8 and len(DOMAINS) == 6
    for name, s in ROOTS.items():
        p = CW.pab(CW.spec_of(name))[0]
        assert CW.two_adicity(p) == s and (p % 4 == 3) == (s == 1)


@pytest.mark.parametrize("name", NAMES)
def test_decode_golden(ctx, name):
    """every decodePoint case the reference recorded -- all prefixes, wrong lengths, hybrid parity,
    x with and without a y, x >= p, x = 0, x = p - 1 -- and the compressed ones through pointFromX"""
    assert CW.check_decode_golden(ctx, CW.spec_of(name)) >= 50


@pytest.mark.parametrize("name", DOMAINS)
def test_wire_golden(ctx, name):
    """every EC#verify(msg, der, key) case the reference recorded: valid signatures under
    compressed, uncompressed and hybrid keys, disturbed r / s / digest / key, every malformed-DER
    family, r and s out of range and wider than 32 bytes, refused and off-curve keys"""
    assert CW.check_wire_golden(ctx, CW.spec_of(name)) >= 57


@pytest.mark.parametrize("name", ["secp112r1", "p224_user"])
def test_golden_dev_form(ctx, name):
    spec = CW.spec_of(name)
    CW.check_decode_golden(ctx, spec, form="dev_np")
    CW.check_wire_golden(ctx, spec, form="dev_np")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(ROOTS))
def test_random_decompress_matches_model(ctx, name, n):
    spec = CW.spec_of(name)
    good = CW.check_random_decompress(ctx, spec, n, seed=1000 + n)
    if n >= 203:
        # about half of all x are abscissae of the curve: a test that decodes nothing checks nothing
        assert 0.3 * n <= good <= 0.7 * n, good
    CW.check_random_decode(ctx, spec, n, seed=2000 + n)


@pytest.mark.parametrize("n", SIZES)
def test_host_form_equals_dev_form(ctx, n):
    """byte for byte, outputs pre-filled with 0xA5, on a Tonelli-Shanks curve"""
    spec = CW.spec_of("secp224k1")
    cid = CW.define(ctx, spec)
    xs, odd = CW.random_xs(spec, n, seed=77 + n)
    x = np.stack([CW.b32(v) for v in xs])
    odd = np.array(odd, np.uint8)
    a, b = (CW.run_decompress(ctx, cid, x, odd, f) for f in FORMS)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    enc = np.concatenate([(2 + odd)[:, None], x[:, 32 - spec["pl"]:]], axis=1).astype(np.uint8)
    a, b = (CW.run_decode(ctx, cid, enc, f) for f in FORMS)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    batch = CW.wire_batch(spec, n, seed=5)
    for e in ("compressed", "full"):
        w = batch[e]
        a, b = (CW.run_wire(ctx, cid, batch["h"], w["der"], w["lens"], w["keys"], 0, f) for f in FORMS)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
        assert set(np.unique(a[0])) <= {0, 1} and CW.FILL not in a[1]


@pytest.fixture(scope="module", params=["brainpoolP256r1", "secp224k1"])
def wire(request, ctx):
    """one 257-item batch per curve and its reference verdicts (raw-form verify == C oracle),
    shared by the sizes below"""
    spec = CW.spec_of(request.param)
    batch = CW.wire_batch(spec, 257, seed=sum(map(ord, request.param)))
    return spec, batch, CW.wire_reference(ctx, spec, batch)


@pytest.mark.parametrize("n", SIZES + [257])
def test_random_wire_matches_verify_and_oracle(ctx, wire, n):
    spec, batch, want = wire
    CW.check_wire_batch(ctx, spec, batch, want, n)


def test_random_wire_dev_form_and_null_err(ctx, wire):
    spec, batch, want = wire
    CW.check_wire_batch(ctx, spec, batch, want, 257, form="dev_np")
    CW.check_wire_batch(ctx, spec, batch, want, 203, want_err=False)
    CW.check_wire_batch(ctx, spec, batch, want, 9, form="dev_np", want_err=False)


def _code(call):
    with pytest.raises(_lib.EllgpuError) as e:
        call()
    return e.value.code, str(e.value).split(": ", 1)[1]


def test_error_paths(hs, ctx):
    spec = CW.spec_of("brainpoolP256r1")
    p, a, b = CW.pab(spec)
    dom = CW.define(ctx, spec)
    plain = ctx.define_short(p, a, b)
    ed = ctx.define_edwards((1 << 255) - 19, -1 % ((1 << 255) - 19), 121665)
    assert dom != plain
    x = np.zeros((1, 32), np.uint8)
    one = np.zeros(1, np.uint8)
    enc = np.zeros((1, 33), np.uint8)
    h = np.zeros((1, 32), np.uint8)
    sig = [bytes.fromhex("3006020101020101")]
    # a plain id decodes, and refuses the verify; a preset id and an unknown id are argument errors;
    # an Edwards curve has no short-curve encodings
    assert ctx.custom_decompress(plain, x, one)[1][0] in (0, 2)
    assert ctx.custom_decode_points(plain, enc)[1][0] == 1
    assert _code(lambda: ctx.custom_verify_wire(plain, h, sig, enc))[0] == -5
    for cid in (0, 3, 6, 7):
        assert _code(lambda: ctx.custom_decompress(cid, x, one))[0] == -2
        assert _code(lambda: ctx.custom_decode_points(cid, enc))[0] == -2
        assert _code(lambda: ctx.custom_verify_wire(cid, h, sig, enc))[0] == -2
    for cid in (31, 99, -1):
        assert _code(lambda: ctx.custom_decompress(cid, x, one)) == (-2, "unknown curve id")
        assert _code(lambda: ctx.custom_verify_wire(cid, h, sig, enc)) == (-2, "unknown curve id")
    assert _code(lambda: ctx.custom_decompress(ed, x, one))[0] == -5
    assert _code(lambda: ctx.custom_decode_points(ed, enc))[0] == -5
    assert _code(lambda: ctx.custom_verify_wire(ed, h, sig, enc))[0] == -5
    # enc_len / pub_len / stride / hash_len 0
    assert _code(lambda: ctx.custom_decode_points(dom, np.zeros((1, 0), np.uint8)))[0] == -2
    assert _code(lambda: ctx.custom_verify_wire(dom, h, sig, np.zeros((1, 0), np.uint8)))[0] == -2
    assert _code(lambda: ctx.custom_verify_wire(dom, np.zeros((1, 0), np.uint8), sig, enc))[0] == -2
    # NULL pointers, in the host and the _dev form
    P = lambda arr: arr.ctypes.data
    out, st = np.zeros((1, 64), np.uint8), np.zeros(1, np.uint8)
    lens = np.array([8], np.uint32)
    der = np.frombuffer(sig[0], np.uint8).copy()
    for suffix, extra in (("", ()), ("_dev", (None,))):
        dec = getattr(hs, "ellgpu_custom_decompress" + suffix)
        dcd = getattr(hs, "ellgpu_custom_decode_points" + suffix)
        ver = getattr(hs, "ellgpu_custom_verify_wire" + suffix)
        good = [P(x), P(one), P(out), P(st)]
        for k in range(4):
            args = list(good)
            args[k] = None
            assert dec(ctx._ctx, dom, 1, *args, *extra) == -2
            assert hs.ellgpu_last_error() == b"null pointer"
        good = [P(enc), 33, P(out), P(st)]
        for k in (0, 2, 3):
            args = list(good)
            args[k] = None
            assert dcd(ctx._ctx, dom, 1, *args, *extra) == -2
        assert dcd(ctx._ctx, dom, 1, P(enc), 0, P(out), P(st), *extra) == -2
        assert hs.ellgpu_last_error() == b"enc_len must be positive"
        good = [P(h), 32, 0, P(der), 8, P(lens), P(enc), 33, P(st), None]       # out_err may be NULL
        assert ver(ctx._ctx, dom, 1, *good, *extra) == 0
        for k in (0, 3, 5, 6, 8):
            args = list(good)
            args[k] = None
            assert ver(ctx._ctx, dom, 1, *args, *extra) == -2
        # n = 0: nothing is read or written, NULL buffers included
        assert dec(ctx._ctx, dom, 0, None, None, None, None, *extra) == 0
        assert dcd(ctx._ctx, dom, 0, None, 33, None, None, *extra) == 0
        assert ver(ctx._ctx, dom, 0, None, 32, 0, None, 8, None, None, 33, None, None, *extra) == 0
        assert dec(None, dom, 0, None, None, None, None, *extra) == -2
    # a digest that msgBitLength leaves wider than 256 bits: refused like ellgpu_ecdsa_verify
    assert _code(lambda: ctx.custom_verify_wire(dom, np.zeros((1, 64), np.uint8), sig, enc, msg_bits=256))[0] == -2
    # the preset-named entry points keep refusing user-defined ids
    assert _code(lambda: ctx.decompress(dom, x, one))[0] == -5
    assert _code(lambda: ctx.decode_points(plain, enc))[0] == -5
    assert _code(lambda: ctx.ecdsa_verify_wire(dom, h, sig, enc))[0] == -5
    assert hs.ellgpu_version() == 0x000200


def test_same_parameters_same_id(hs):
    """the block a definition builds is deterministic (the square-root constants included): the
    same parameters give the same id again, on one context and on both members of a group; a
    domain and the plain curve under it stay apart"""
    c = elliptic_amd.Context(0, lib_path=hs)
    g = elliptic_amd.Context(lib_path=hs, devices=[0, 0])
    try:
        ids = {}
        for rnd in range(2):
            for spec in CW.curves():
                cid = CW.define(c, spec)
                assert ids.setdefault(spec["name"], cid) == cid
                if CW.is_domain(spec):
                    pid = c.define_short(*CW.pab(spec))
                    assert pid != cid and ids.setdefault(spec["name"] + "/plain", pid) == pid
        assert len(set(ids.values())) == len(ids) == 14
        spec = CW.spec_of("p224_user")
        gid = CW.define(g, spec)
        assert gid == CW.define(g, spec)
        # a group runs the new calls on its first member
        assert CW.check_wire_golden(g, spec, cid=gid) >= 57
        assert CW.check_decode_golden(g, spec, cid=gid) >= 50
    finally:
        g.close()
        c.close()
