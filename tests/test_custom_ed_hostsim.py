"""The key side of user-defined Edwards curves (ellgpu_custom_ed_decompress, _decode_points, _validate,
_derive, _derive_wire, _encode_points) on the CPU: the hostsim build of the device code (tests/hostsim)
against the reference's recorded answers (tests/golden/custom_ed.json), against edwards.js, base.js
and key.js restated over Python integers on random batches (tests/custom_ed_checks.py), the refusal
matrix, and the parameter block, which the new calls must leave as it was."""
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
import custom_ed_checks as CK  # noqa: E402

SEED = {name: sum(map(ord, name)) for name in CK.BIG}


@pytest.fixture(scope="module")
def hs():
    lib = _lib.load(build_hostsim(), optional=("ellgpu_probe_valu", "ellgpu_ctx_set_timing",
                                               "ellgpu_ctx_get_timing", "ellgpu_debug_field_op"))
    lib.hs_rt_block.restype = ctypes.c_int
    lib.hs_rt_block.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batches():
    """one 65-item batch per curve and the model's answers, shared by every size"""
    return {name: CK.random_batch(CK.spec_of(name), 65, SEED[name]) for name in CK.BIG}


def _block(hs, ctx, cid):
    buf = np.zeros(4096, np.uint8)
    size = hs.hs_rt_block(ctx._ctx, cid, buf.ctypes.data, buf.size)
    assert 0 < size <= buf.size
    return buf[:size].tobytes()


def test_curve_set():
    assert [c["name"] for c in CK.curves()] == CK.BIG + CK.TOY
    p224 = CK.spec_of("p224_d11")
    assert CK.params(p224) == ((1 << 224) - (1 << 96) + 1, 1, 11) and p224["pl"] == 28
    for name in CK.BIG:
        p, a, d = CK.params(CK.spec_of(name))
        assert pow(a, (p - 1) // 2, p) == 1 and pow(d, (p - 1) // 2, p) == p - 1        # complete addition laws
        assert CK.spec_of(name)["pmod4"] == p % 4 == (3 if name in ("curve1174", "e222") else 1)
    # the order test has the published prime subgroup order on Curve1174 and E-222; the facts the
    # contract pins, as recorded
    assert CK.I(CK.spec_of("curve1174")["n"]) == (1 << 249) - 11332719920821432534773113288178349711
    assert CK.I(CK.spec_of("e222")["n"]) == 1684996666696914987166688442938726735569737456760058294185521417407
    PRIME_ORDER = ("curve1174", "e222")
    for name in CK.BIG:
        cs = CK.spec_of(name)["cases"]
        tags = {c["tag"]: c for c in cs if c["op"] == "validate"}
        assert tags["identity"]["reason"] == tags["identity_plus_p"]["reason"] == "Invalid public key"
        assert tags["off_curve"]["reason"] == "Public key is not a point"
        # n is the prime subgroup order on Curve1174 and E-222 and 4 elsewhere (those group orders are not known)
        assert tags["subgroup"]["result"] == (1 if name in PRIME_ORDER else 0)
        assert tags["order_4"]["result"] == tags["minus_one"]["result"] == (0 if name in PRIME_ORDER else 1)
        assert tags["shifted_by_(0,-1)"]["reason"] == "Public key * N != O"
        der = {c["tag"]: c for c in cs if c["op"] == "derive"}
        assert CK.I(der["priv_0"]["x"]) == 0 and CK.I(der["identity:priv_1"]["x"]) == 0      # legal peer, legal result
        assert der["off_curve:priv_0"]["xmsg"] == "public point not validated"
    # the toy curves hold the zero-denominator cases: pointFromX returns (x, 0) for either parity
    # (p = 13, d = 4, x = 6 and x = 7), pointFromY answers x^2 = 0 by parity before any root
    toy = {r["v"]: r for r in CK.spec_of("p13_d4")["rows"]}
    assert toy[6]["fx"] == [[6, 0], [6, 0]] and toy[7]["fx"] == [[7, 0], [7, 0]]
    assert toy[1]["fy"] == [[0, 1], "invalid point"] and toy[12]["fy"] == [[0, 12], "invalid point"]
    both = {r if isinstance(r, str) else "ok" for name in CK.TOY for row in CK.spec_of(name)["rows"] for r in row["fx"] + row["fy"]}
    assert both == {"ok", "invalid point", "Assertion failed"}


@pytest.mark.parametrize("name", CK.BIG)
def test_model_meets_the_conditions(batches, name):
    """the batch construction alone gives every status and at least 60 % shared secrets"""
    assert CK.model_meets_conditions(batches[name], 65)
    big = CK.random_batch(CK.spec_of(name), 300, SEED[name], distinct=31)
    assert CK.model_meets_conditions(big, 300)


@pytest.mark.parametrize("form", ["host", "dev_np"])
@pytest.mark.parametrize("name", CK.BIG)
def test_golden(ctx, name, form):
    spec = CK.spec_of(name)
    seen = CK.check_golden(ctx, spec, form)
    nr = 3 if spec["pmod4"] == 1 else 2
    assert {("fromx", 0), ("fromx", nr), ("fromy", 0), ("fromy", 2), ("fromy", nr), ("decode", 1), ("decode", 3),
            ("validate", 0), ("validate", 1), ("validate", 2), ("validate", 3), ("derive", 0), ("derive", 1),
            ("derive_wire", 0), ("derive_wire", 1), ("derive_wire", 3)} <= seen


@pytest.mark.parametrize("form", ["host", "dev_np"])
@pytest.mark.parametrize("name", CK.TOY)
def test_toy_exhaustive(ctx, name, form):
    spec = CK.spec_of(name)
    seen, dseen = CK.check_toy(ctx, spec, form)
    assert seen == ({0, 2, 3} if spec["pmod4"] == 1 else {0, 2})
    assert dseen == ({0, 2} if name == "p13_d4" else {0})       # Z = 0: the incomplete law alone


@pytest.mark.parametrize("n", [1, 5, 64, 65])
def test_random_batch_matches_model(ctx, batches, n):
    for name in CK.BIG:
        spec = CK.spec_of(name)
        a = CK.check_batch(ctx, spec, batches[name], n)
        b = CK.check_batch(ctx, spec, batches[name], n, "dev_np")
        assert all((u == v).all() for u, v in zip(a, b))


def test_derive_wire_while_the_scratch_regrows(hs):
    """one context, one curve, n = 3, 257, 3 through both forms, each against a context of its own"""
    spec = CK.spec_of("curve1174")
    bt = CK.random_batch(spec, 257, SEED["curve1174"], distinct=31)
    got = CK.check_derive_wire_regrow(lambda: elliptic_amd.Context(0, lib_path=hs), spec, bt["wire"]["comp"], ["host", "dev_np"])
    assert len(got) == 6 and set(bt["wire"]["comp"]["st"].tolist()) == {0, 3}      # shared secrets, and keys that do not decode


@pytest.mark.parametrize("name", ["curve1174", "p224_d11"])
def test_ecdh_symmetry(ctx, name):
    CK.check_symmetry(ctx, CK.spec_of(name), 5, seed=1)
    CK.check_symmetry(ctx, CK.spec_of(name), 5, seed=2, form="dev_np")


def _code(call):
    with pytest.raises(_lib.EllgpuError) as e:
        call()
    return e.value.code


def test_refusals_and_the_block(hs, ctx):
    spec = CK.spec_of("twisted_a4")
    p, a, d = CK.params(spec)
    ed = CK.define(ctx, spec)
    before = _block(hs, ctx, ed)
    short = ctx.define_short(p, a, 7)
    dom = CE.define(ctx, CE.spec_of("brainpoolP256r1"))
    mont = ctx.define_mont(p, 486662)
    k = np.ones((1, 32), np.uint8)
    x = CK.rows([5])
    pt = CK.model_of(spec).from_y(5, 0)[0] or CK.model_of(spec).from_y(6, 0)[0]
    xy = CK.xy_rows([pt])
    odd = np.zeros(1, np.uint8)
    enc = np.frombuffer(CK.model_of(spec).encode(*pt, False), np.uint8).reshape(1, -1)
    new_calls = [lambda c: ctx.custom_ed_decompress(c, x, odd), lambda c: ctx.custom_ed_decompress(c, x, odd, True),
                 lambda c: ctx.custom_ed_decode_points(c, enc), lambda c: ctx.custom_ed_validate(c, xy),
                 lambda c: ctx.custom_ed_validate(c, xy, 4), lambda c: ctx.custom_ed_derive(c, k, xy),
                 lambda c: ctx.custom_ed_derive_wire(c, k, enc),
                 lambda c: CK._raw_encode(ctx, c, xy)]
    for call in new_calls:
        call(ed)
        for cid in (short, dom, mont):                             # short, domain and Montgomery user-defined ids
            assert _code(lambda: call(cid)) == -5
        for cid in (0, 3, 6, 7, 15, 31, 32, 99, -1):               # preset ids and unknown ids
            assert _code(lambda: call(cid)) == -2
    assert ctx.custom_ed_encode_points(ed, xy).tobytes() == enc.tobytes()
    # every old custom_* call still refuses an Edwards id
    h = np.ones((1, 32), np.uint8)
    old_calls = [lambda: ctx.custom_decompress(ed, x, odd), lambda: ctx.custom_decode_points(ed, enc),
                 lambda: ctx.custom_derive(ed, k, xy), lambda: ctx.custom_derive_wire(ed, k, enc),
                 lambda: ctx.custom_validate(ed, xy, check_order=False),
                 lambda: ctx.custom_mont_ladder(ed, k, x), lambda: ctx.custom_mont_validate(ed, x),
                 lambda: ctx.custom_mont_derive(ed, k, x), lambda: ctx.ecdsa_verify(ed, h, k, k, xy),
                 lambda: ctx.validate(ed, xy), lambda: ctx.encode_points(ed, xy), lambda: ctx.ecdh_derive(ed, k, xy),
                 lambda: ctx.decompress(ed, x, odd), lambda: ctx.mul_fixed(ed, k)]
    for i, call in enumerate(old_calls):
        assert _code(call) == -5, i
    P = lambda arr: arr.ctypes.data
    ox, oxy, st = np.zeros((1, 32), np.uint8), np.zeros((1, 64), np.uint8), np.zeros(1, np.uint8)
    oenc = np.zeros((1, 65), np.uint8)
    raw = [("ellgpu_custom_encode_points", [P(xy), 0, P(oenc)]),
           ("ellgpu_custom_recover", [P(h), 32, P(k), P(k), P(odd), P(oxy), P(st)]),
           ("ellgpu_custom_sign", [P(h), 32, 0, P(k), P(k), 0, P(ox), P(ox), P(st), P(st)]),
           ("ellgpu_custom_verify_wire", [P(h), 32, 0, P(xy), 64, None, P(xy), 33, P(st), P(st)])]
    for name, args in raw:
        assert getattr(hs, name)(ctx._ctx, ed, 1, *args) == -5, name
    # NULL pointers, in the host and the _dev form; n = 0 reads and writes nothing
    table = {"ellgpu_custom_ed_decompress": ([P(x), P(odd), 0, P(oxy), P(st)], (0, 1, 3, 4)),
             "ellgpu_custom_ed_decode_points": ([P(enc), enc.shape[1], P(oxy), P(st)], (0, 2, 3)),
             "ellgpu_custom_ed_validate": ([P(xy), None, P(st)], (0, 2)),
             "ellgpu_custom_ed_derive": ([P(k), P(xy), P(ox), P(st)], (0, 1, 2, 3)),
             "ellgpu_custom_ed_derive_wire": ([P(k), P(enc), enc.shape[1], P(ox), P(st), None], (0, 1, 3, 4)),
             "ellgpu_custom_ed_encode_points": ([P(xy), 1, P(oenc)], (0, 2))}
    for name, (good, ptrs) in table.items():
        for suffix, extra in (("", ()), ("_dev", (None,))):
            fn = getattr(hs, name + suffix)
            assert fn(ctx._ctx, ed, 1, *good, *extra) == 0, name
            for j in ptrs:
                args = list(good)
                args[j] = None
                assert fn(ctx._ctx, ed, 1, *args, *extra) == -2, (name, j)
                assert hs.ellgpu_last_error() == b"null pointer"
            empty = [None if isinstance(g, int) and j in ptrs else g for j, g in enumerate(good)]
            assert fn(ctx._ctx, ed, 0, *empty, *extra) == 0
            assert fn(None, ed, 0, *empty, *extra) == -2
            assert fn(ctx._ctx, 6, 1, *good, *extra) == -2 and b"ed25519" in hs.ellgpu_last_error()
            assert fn(ctx._ctx, short, 1, *good, *extra) == -5 and b"ellgpu_curve_define_edwards" in hs.ellgpu_last_error()
    for name in ("ellgpu_custom_ed_decode_points", "ellgpu_custom_ed_derive_wire"):
        good = list(table[name][0])
        good[1 if name.endswith("points") else 2] = 0
        assert getattr(hs, name)(ctx._ctx, ed, 1, *good) == -2
    # the old calls on the same id still work, and the registered block is what it was
    oxy2, inf = ctx.mul_var(ed, CK.rows([1]), xy)
    assert inf[0] == 0 and oxy2.tobytes() == xy.tobytes()
    assert _block(hs, ctx, ed) == before
    assert ctx.define_edwards(p, a, d) == ed
    assert hs.ellgpu_version() == 0x000200


def test_block_is_unchanged_on_every_curve(hs, batches):
    """a fresh context: define, read the block, run every new call, read it again"""
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        for name in CK.BIG + CK.TOY:
            spec = CK.spec_of(name)
            cid = CK.define(c, spec)
            before = _block(hs, c, cid)
            if name in CK.BIG:
                CK.check_batch(c, spec, batches[name], 9, cid=cid)
            else:
                CK.check_toy(c, spec)
            assert _block(hs, c, cid) == before and CK.define(c, spec) == cid
    finally:
        c.close()


def test_group_runs_on_its_first_member(hs, ctx, batches):
    g = elliptic_amd.Context(lib_path=hs, devices=[0, 0])
    try:
        for name in ("e222", "twisted_am1"):
            spec = CK.spec_of(name)
            gid = CK.define(g, spec)
            assert CK.define(g, spec) == gid
            CK.check_golden(g, spec, cid=gid)
            a = CK.check_batch(g, spec, batches[name], 41, cid=gid)
            b = CK.check_batch(ctx, spec, batches[name], 41)
            assert all((u == v).all() for u, v in zip(a, b))
    finally:
        g.close()
