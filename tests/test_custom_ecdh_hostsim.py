"""ECDH, key validation and SEC1 encoding on user-defined short-curve domains (ellgpu_custom_derive,
_custom_derive_wire, _custom_validate, _custom_encode_points) on the CPU: the hostsim build of the
device code (tests/hostsim) against the reference's recorded answers (tests/golden/custom_ecdh.json)
and against KeyPair#derive / #validate / BasePoint#encode restated over Python integers on random
batches (tests/custom_ecdh_checks.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import custom_ecdh_checks as CE  # noqa: E402

DOMAINS = [c["name"] for c in CE.curves()]


@pytest.fixture(scope="module")
def hs():
    return _lib.load(build_hostsim(), optional=("ellgpu_probe_valu", "ellgpu_ctx_set_timing",
                                                "ellgpu_ctx_get_timing", "ellgpu_debug_field_op"))


@pytest.fixture(scope="module")
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


def test_domain_set():
    assert DOMAINS == ["brainpoolP256r1", "secp192k1", "secp112r1", "secp224k1", "w25519_like", "p224_user"]
    assert [c["name"] for c in CE.CR.curves()] == DOMAINS
    w = CE.spec_of("w25519_like")
    p, a, b, n = CE.CD.params(w)[:4]
    assert p // n == 7 and p % 4 == 1
    # the point of order 2: x = 486662 / 3, y = 0
    o2 = next(c for c in w["validate"] if c["tag"] == "order_2")
    assert CE.I(o2["y"]) == 0 and CE.I(o2["x"]) * 3 % p == 486662


@pytest.mark.parametrize("name", ["brainpoolP256r1", "secp224k1", "w25519_like", "p224_user"])
def test_model_meets_the_conditions(name):
    """the batch construction alone gives every status and at least 60 % shared secrets"""
    bt = CE.random_batch(CE.spec_of(name), 300, seed=sum(map(ord, name)))
    assert CE.model_meets_conditions(bt, 257) and CE.model_meets_conditions(bt, 300)
    assert (bt["st"] == 0).sum() >= 0.65 * 300


@pytest.mark.parametrize("form", ["host", "dev_np"])
@pytest.mark.parametrize("name", DOMAINS)
def test_golden(ctx, name, form):
    """every case the reference recorded: its own key pairs in both directions, priv = 0, 1, n - 1,
    n, n + 1, 2^256 - 1, off-curve peers, coordinates + p, every SEC1 prefix and the wrong ones,
    KeyPair#validate on subgroup, infinite, off-curve and low-order points, encodings"""
    seen = CE.check_golden(ctx, CE.spec_of(name), form)
    assert seen["derive"] == {0, 1, 2} and seen["wire"] == {0, 1, 2, 3}


@pytest.mark.parametrize("name", DOMAINS)
def test_random_batch_matches_model(ctx, name):
    spec = CE.spec_of(name)
    x, st = CE.check_random(ctx, spec, 300, seed=sum(map(ord, name)))
    x2, st2 = CE.check_random(ctx, spec, 300, seed=sum(map(ord, name)), form="dev_np")
    assert (x == x2).all() and (st == st2).all()
    CE.check_symmetry(ctx, spec, CE.random_batch(spec, 300, seed=sum(map(ord, name))), 300)


@pytest.mark.parametrize("n", [1, 8, 9, 41, 203])
def test_sizes(ctx, n):
    """the hostsim small-call and chunk edges, on the cofactor curve and on the domain with n > p"""
    for name in ("w25519_like", "secp224k1"):
        spec = CE.spec_of(name)
        CE.check_batch(ctx, spec, CE.random_batch(spec, 300, seed=sum(map(ord, name))), n)
        CE.check_wire_batch(ctx, spec, CE.random_batch(spec, 300, seed=sum(map(ord, name))), n)


def test_plain_id_derives_and_encodes(ctx):
    """derive, validate without the order test and encode need neither n nor G"""
    spec = CE.spec_of("brainpoolP256r1")
    p, a, b = CE.CD.params(spec)[:3]
    plain = ctx.define_short(p, a, b)
    assert plain != CE.define(ctx, spec)
    bt = CE.random_batch(spec, 300, seed=sum(map(ord, spec["name"])))
    x, st = CE.run_derive(ctx, plain, bt["priv"][:41], bt["pub"][:41])
    assert (x == bt["x"][:41]).all() and (st == bt["st"][:41]).all()
    assert (CE.run_validate(ctx, plain, bt["pub"][:41], bt["inf"][:41], False) == bt["vst0"][:41]).all()
    CE.check_encode_batch(ctx, spec, bt, 41, cid=plain)
    CE.check_wire_batch(ctx, spec, bt, 41, cid=plain)


def _code(call):
    with pytest.raises(_lib.EllgpuError) as e:
        call()
    return e.value.code


def test_refusals(hs, ctx):
    spec = CE.spec_of("brainpoolP256r1")
    p, a, b = CE.CD.params(spec)[:3]
    dom = CE.define(ctx, spec)
    plain = ctx.define_short(p, a, b)
    ed = ctx.define_edwards((1 << 255) - 19, -1 % ((1 << 255) - 19), 121665)
    k = np.ones((1, 32), np.uint8)
    g = CE.xy64(CE.I(spec["g"]["x"]), CE.I(spec["g"]["y"])).reshape(1, 64).copy()
    enc = ctx.custom_encode_points(dom, g, True)
    assert ctx.custom_derive(dom, k, g)[1][0] == 0 and ctx.custom_derive_wire(dom, k, enc)[1][0] == 0
    # a plain id: everything but the order test
    assert _code(lambda: ctx.custom_validate(plain, g, check_order=True)) == -5
    assert ctx.custom_validate(plain, g, check_order=False)[0] == 0
    calls = [lambda c: ctx.custom_derive(c, k, g), lambda c: ctx.custom_derive_wire(c, k, enc),
             lambda c: ctx.custom_validate(c, g, check_order=False), lambda c: ctx.custom_validate(c, g),
             lambda c: ctx.custom_encode_points(c, g), lambda c: ctx.custom_encode_points(c, g, True)]
    for call in calls:
        assert _code(lambda: call(ed)) == -5                       # a user-defined Edwards id
        for cid in (0, 3, 6, 7, 31, 99, -1):                       # preset ids and unknown ids
            assert _code(lambda: call(cid)) == -2
    # pub_len: 0 is an argument error; a length that is no encoding's leaves every item undecoded
    P = lambda arr: arr.ctypes.data
    x, st, err = np.zeros((1, 32), np.uint8), np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    for suffix, extra in (("", ()), ("_dev", (None,))):
        fn = getattr(hs, "ellgpu_custom_derive_wire" + suffix)
        assert fn(ctx._ctx, dom, 1, P(k), P(enc), 0, P(x), P(st), P(err), *extra) == -2
        assert hs.ellgpu_last_error() == b"pub_len must be positive"
        assert fn(ctx._ctx, dom, 1, P(k), P(enc), enc.shape[1] - 1, P(x), P(st), P(err), *extra) == 0
        assert (st[0], err[0]) == (3, 1) and not x.any()
    # NULL pointers, in the host and the _dev form; n = 0 reads and writes nothing
    xy_out = np.zeros((1, 65), np.uint8)
    table = {"ellgpu_custom_derive": ([P(k), P(g), P(x), P(st)], (0, 1, 2, 3)),
             "ellgpu_custom_derive_wire": ([P(k), P(enc), enc.shape[1], P(x), P(st), P(err)], (0, 1, 3, 4)),
             "ellgpu_custom_validate": ([P(g), None, 1, P(st)], (0, 3)),
             "ellgpu_custom_encode_points": ([P(g), 0, P(xy_out)], (0, 2))}
    for name, (good, ptrs) in table.items():
        for suffix, extra in (("", ()), ("_dev", (None,))):
            fn = getattr(hs, name + suffix)
            assert fn(ctx._ctx, dom, 1, *good, *extra) == 0, name
            for j in ptrs:
                args = list(good)
                args[j] = None
                assert fn(ctx._ctx, dom, 1, *args, *extra) == -2, (name, j)
                assert hs.ellgpu_last_error() == b"null pointer"
            nulls = [None if (j in ptrs or v is None) else v for j, v in enumerate(good)]
            assert fn(ctx._ctx, dom, 0, *nulls, *extra) == 0
            assert fn(None, dom, 0, *nulls, *extra) == -2
    # out_err may be NULL
    assert hs.ellgpu_custom_derive_wire(ctx._ctx, dom, 1, P(k), P(enc), enc.shape[1], P(x), P(st), None) == 0
    # the preset-named entry points keep refusing user-defined ids
    for cid in (dom, plain):
        assert _code(lambda: ctx.validate(cid, g)) == -5
        assert _code(lambda: ctx.encode_points(cid, g)) == -5
        assert _code(lambda: ctx.ecdh_derive(cid, k, g)) == -5
    assert hs.ellgpu_version() == 0x000200


def test_group_runs_on_its_first_member(hs, ctx):
    g = elliptic_amd.Context(lib_path=hs, devices=[0, 0])
    try:
        for name in ("secp224k1", "w25519_like"):
            spec = CE.spec_of(name)
            gid = CE.define(g, spec)
            CE.check_golden(g, spec, cid=gid)
            a = CE.check_random(g, spec, 41, seed=9, cid=gid)
            b = CE.check_random(ctx, spec, 41, seed=9)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    finally:
        g.close()
