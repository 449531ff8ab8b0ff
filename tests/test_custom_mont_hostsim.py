"""User-defined Montgomery curves (ellgpu_curve_define_mont, ellgpu_custom_mont_ladder, _validate,
_derive) on the CPU: the hostsim build of the device code (tests/hostsim) against the reference's
recorded answers (tests/golden/custom_mont.json), against mont.js restated over Python integers on
random batches (tests/custom_mont_checks.py) and, on curve25519 written out by hand, against the
preset's own ladder."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import custom_ecdh_checks as CE  # noqa: E402
import custom_mont_checks as CM  # noqa: E402

CURVES = [c["name"] for c in CM.curves()]
SEED = {name: sum(map(ord, name)) for name in CM.BIG}


@pytest.fixture(scope="module")
def hs():
    return _lib.load(build_hostsim(), optional=("ellgpu_probe_valu", "ellgpu_ctx_set_timing",
                                                "ellgpu_ctx_get_timing", "ellgpu_debug_field_op"))


@pytest.fixture(scope="module")
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batches():
    """one 203-item batch per curve and the model's answers, shared by every size"""
    return {name: CM.random_batch(CM.spec_of(name), 203, SEED[name]) for name in CM.BIG}


def test_curve_set():
    assert CURVES == CM.BIG + ["toy_p23"]
    want = {"c25519_user": ((1 << 255) - 19, 486662, 1, 32), "m221": ((1 << 221) - 3, 117050, 1, 28),
            "toy_p23": (23, 5, 3, 1)}
    for name, (p, a, m4, pl) in want.items():
        s = CM.spec_of(name)
        assert CM.params(s) == (p, a) and s["pmod4"] == m4 == p % 4 and s["pl"] == pl
    bp, top = CM.spec_of("bp256_mont"), CM.spec_of("top256_mont")
    assert CM.I(bp["p"]) == 0xA9FB57DBA1EEA9BC3E660A909D838D726E3BF623D52620282013481D1F6E5377
    assert CM.I(top["p"]) == (1 << 256) - 189 and bp["pmod4"] == top["pmod4"] == 3
    # a full-width a24: a one-limb product would not do
    assert CM.I(bp["a"]).bit_length() > 224 and CM.I(bp["a24"]).bit_length() > 224
    toy = CM.spec_of("toy_p23")["cases"]
    assert sorted((CM.I(c["x"]), CM.I(c["k"])) for c in toy) == [(x, k) for x in range(23) for k in range(31)]
    # the facts the engine's contract rests on, as the reference recorded them
    for name in CM.BIG:
        cs = CM.spec_of(name)["cases"]
        assert sum(c["tag"] == "k_random" for c in cs) >= 40
        assert all(c["z0"] == 1 and CM.I(c["getx"]) == 0 for c in cs if CM.I(c["x"]) in (0, CM.I(CM.spec_of(name)["p"])))
        assert all(c.get("valid") == 1 for c in cs if CM.I(c["x"]) == 0)
    low = next(c for c in CM.spec_of("c25519_user")["cases"] if c["tag"] == "low_order_x_1_k_4")
    assert low["z0"] == 1 and low["valid"] == 1


@pytest.mark.parametrize("name", CM.BIG)
def test_model_meets_the_conditions(batches, name):
    """the batch construction alone gives every status and at least 60 % shared secrets"""
    bt = batches[name]
    assert CM.model_meets_conditions(bt, 203)
    assert set(bt["dst"][:4].tolist()) == CM.statuses_of(CM.spec_of(name))
    assert 0.6 * 203 <= (bt["kind"] == 0).sum() <= 0.8 * 203 and 0.1 * 203 <= (bt["kind"] == 1).sum() <= 0.3 * 203


@pytest.mark.parametrize("form", ["host", "dev_np"])
@pytest.mark.parametrize("name", CURVES)
def test_golden(ctx, name, form):
    """every case the reference recorded: k = 0, 1, 2, 3, 2^255, 2^256 - 1, scalars with leading zero
    bytes, random ones; x = 0, 1, p - 1, p, p + 1, 2^256 - 1, abscissae of the curve, non-residues,
    both as x + p; every (x, k) of the toy curve"""
    spec = CM.spec_of(name)
    assert CM.check_golden(ctx, spec, form) == CM.statuses_of(spec)


@pytest.mark.parametrize("n", [1, 8, 9, 41, 203])
def test_random_batch_matches_model(ctx, batches, n):
    """the hostsim small-call and chunk edges"""
    for name in CM.BIG:
        spec = CM.spec_of(name)
        a = CM.check_batch(ctx, spec, batches[name], n)
        b = CM.check_batch(ctx, spec, batches[name], n, "dev_np")
        assert all((u == v).all() for u, v in zip(a, b))


def test_c25519_user_equals_the_preset(ctx, batches):
    """curve25519 written out by hand against ellgpu_x25519_ladder / _derive on the same rows"""
    spec = CM.spec_of("c25519_user")
    cid = CM.define(ctx, spec)
    cs = spec["cases"]
    sets = [(batches["c25519_user"]["k"], batches["c25519_user"]["x"]),
            (CM.rows([CM.I(c["k"]) for c in cs]), CM.rows([CM.I(c["x"]) for c in cs]))]
    for k, x in sets:
        ox, inf = CM.run_ladder(ctx, cid, k, x)
        px, pinf = ctx.x25519(k, x)
        assert (ox == px).all() and (inf == pinf).all()
        dx, dst = CM.run_derive(ctx, cid, k, x)
        qx, qst = ctx.x25519_derive(k, x)
        # the preset numbers 'Assertion failed' 1 and leaves the ladder's x beside it
        assert (np.where(dst == 3, 1, dst) == qst).all() and (dx[dst == 0] == qx[dst == 0]).all()
        assert set(dst.tolist()) == {0, 2, 3}


@pytest.mark.parametrize("name", CM.BIG)
def test_ecdh_symmetry(ctx, name):
    CM.check_symmetry(ctx, CM.spec_of(name), 9, seed=1)
    CM.check_symmetry(ctx, CM.spec_of(name), 9, seed=2, form="dev_np")


def _code(call):
    with pytest.raises(_lib.EllgpuError) as e:
        call()
    return e.value.code


def test_ids(hs):
    """same (p, a): same id; never the id of a short or Edwards curve over the same numbers"""
    ctx = elliptic_amd.Context(0, lib_path=hs)
    p, a = CM.params(CM.spec_of("bp256_mont"))
    m = ctx.define_mont(p, a)
    assert ctx.define_mont(p, a) == m and ctx.define_mont(p, a + p if a + p < CM.TOP else a) == m
    for other_b in (1, a, (a + 2) * pow(4, -1, p) % p):
        assert ctx.define_short(p, a, other_b) != m
        assert ctx.define_edwards(p, a, other_b if other_b != a else 2) != m
    assert ctx.define_mont(p, a + 1) != m
    for bad_p in (0, 1, 2, 3, 4, 22, 1 << 255):
        assert _code(lambda: ctx.define_mont(bad_p, 1 if bad_p < 2 else 5 % bad_p)) == -2
    assert ctx.define_mont(5, 1) >= 16
    ctx.close()


def test_id_space_is_shared_and_limited(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        ids = [c.define_mont(23, 5), c.define_short(23, 5, 1), c.define_edwards(23, 5, 7)]
        ids += [c.define_mont(10007, a) for a in range(3, 16)]
        assert ids == list(range(16, 32))
        assert _code(lambda: c.define_mont(10007, 99)) == -5
        assert c.define_mont(23, 5) == 16
    finally:
        c.close()


def test_refusals(hs, ctx):
    spec = CM.spec_of("bp256_mont")
    p, a = CM.params(spec)
    mont = CM.define(ctx, spec)
    short = ctx.define_short(p, a, 7)
    dom = CE.define(ctx, CE.spec_of("brainpoolP256r1"))
    ed = ctx.define_edwards((1 << 255) - 19, -1 % ((1 << 255) - 19), 121665)
    k = np.ones((1, 32), np.uint8)
    x = CM.rows([CM.base_point(spec)])
    xy = np.concatenate([x, x], axis=1)
    inf = np.zeros(1, np.uint8)
    h = np.ones((1, 32), np.uint8)
    new_calls = [lambda c: ctx.custom_mont_ladder(c, k, x), lambda c: ctx.custom_mont_validate(c, x),
                 lambda c: ctx.custom_mont_derive(c, k, x)]
    for call in new_calls:
        call(mont)
        for cid in (short, dom, ed):                               # short, domain and Edwards user-defined ids
            assert _code(lambda: call(cid)) == -5
        for cid in (0, 3, 6, 7, 15, 31, 32, 99, -1):               # preset ids and unknown ids
            assert _code(lambda: call(cid)) == -2
    # every other entry point refuses a Montgomery id
    old_calls = [lambda: ctx.mul_var(mont, k, xy), lambda: ctx.mul_add2(mont, k, xy, k, xy),
                 lambda: ctx.point_add(mont, xy, xy), lambda: ctx.mul_fixed(mont, k),
                 lambda: ctx.custom_decompress(mont, x, inf), lambda: ctx.custom_decode_points(mont, np.ones((1, 33), np.uint8)),
                 lambda: ctx.custom_derive(mont, k, xy), lambda: ctx.custom_validate(mont, xy, check_order=False),
                 lambda: ctx.custom_encode_points(mont, xy), lambda: ctx.ecdsa_verify(mont, h, k, k, xy),
                 lambda: ctx.validate(mont, xy), lambda: ctx.encode_points(mont, xy),
                 lambda: ctx.ecdh_derive(mont, k, xy), lambda: ctx.decompress(mont, x, inf)]
    for i, call in enumerate(old_calls):
        assert _code(call) == -5, i
    P = lambda arr: arr.ctypes.data
    ox, oxy, st = np.zeros((1, 32), np.uint8), np.zeros((1, 64), np.uint8), np.zeros(1, np.uint8)
    raw = [("ellgpu_custom_recover", [P(h), 32, P(k), P(k), P(inf), P(oxy), P(st)]),
           ("ellgpu_custom_sign", [P(h), 32, 0, P(k), P(k), 0, P(ox), P(ox), P(st), P(st)]),
           ("ellgpu_custom_sign_det", [P(h), 32, 0, P(k), 0, 0, P(ox), P(ox), P(st), P(st)]),
           ("ellgpu_custom_verify_wire", [P(h), 32, 0, P(xy), 64, None, P(xy), 33, P(st), P(st)]),
           ("ellgpu_custom_derive_wire", [P(k), P(xy), 33, P(ox), P(st), None]),
           ("ellgpu_mul_var_dev", [P(k), P(xy), P(oxy), P(st), None]),
           ("ellgpu_point_add_dev", [P(xy), None, P(xy), None, P(oxy), P(st), None])]
    for name, args in raw:
        assert getattr(hs, name)(ctx._ctx, mont, 1, *args) == -5, name
        assert b"Montgomery" in hs.ellgpu_last_error(), name
    # NULL pointers, in the host and the _dev form; n = 0 reads and writes nothing
    table = {"ellgpu_custom_mont_ladder": ([P(k), P(x), P(ox), P(st)], (0, 1, 2, 3)),
             "ellgpu_custom_mont_validate": ([P(x), P(st)], (0, 1)),
             "ellgpu_custom_mont_derive": ([P(k), P(x), P(ox), P(st)], (0, 1, 2, 3))}
    for name, (good, ptrs) in table.items():
        for suffix, extra in (("", ()), ("_dev", (None,))):
            fn = getattr(hs, name + suffix)
            assert fn(ctx._ctx, mont, 1, *good, *extra) == 0, name
            for j in ptrs:
                args = list(good)
                args[j] = None
                assert fn(ctx._ctx, mont, 1, *args, *extra) == -2, (name, j)
                assert hs.ellgpu_last_error() == b"null pointer"
            assert fn(ctx._ctx, mont, 0, *[None] * len(good), *extra) == 0
            assert fn(None, mont, 0, *[None] * len(good), *extra) == -2
            assert fn(ctx._ctx, 7, 1, *good, *extra) == -2 and b"ellgpu_x25519_ladder" in hs.ellgpu_last_error()
            assert fn(ctx._ctx, short, 1, *good, *extra) == -5 and b"ellgpu_curve_define_mont" in hs.ellgpu_last_error()
    cid = np.zeros(1, np.int32)
    for args in ([None, b"\x05" * 32], [b"\x17".rjust(32, b"\0"), None]):
        assert hs.ellgpu_curve_define_mont(ctx._ctx, *args, cid.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == -2
    assert hs.ellgpu_curve_define_mont(ctx._ctx, b"\x17".rjust(32, b"\0"), b"\x05".rjust(32, b"\0"), None) == -2
    # the preset's calls are the preset's
    assert ctx.x25519(k, x)[1][0] == 0
    assert hs.ellgpu_version() == 0x000200


def test_group_runs_on_its_first_member(hs, ctx):
    g = elliptic_amd.Context(lib_path=hs, devices=[0, 0])
    try:
        for name in ("m221", "top256_mont"):
            spec = CM.spec_of(name)
            gid = CM.define(g, spec)
            assert CM.define(g, spec) == gid
            CM.check_golden(g, spec, cid=gid)
            bt = CM.random_batch(spec, 41, seed=9)
            a = CM.check_batch(g, spec, bt, 41, cid=gid)
            b = CM.check_batch(ctx, spec, bt, 41)
            assert all((u == v).all() for u, v in zip(a, b))
            assert _code(lambda: g.mul_var(gid, np.ones((1, 32), np.uint8), np.ones((1, 64), np.uint8))) == -5
    finally:
        g.close()
