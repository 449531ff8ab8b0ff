"""Fixed-base tables of caller-chosen points (ellgpu_base_define, _release, _info, ellgpu_mul_base,
ellgpu_mul_base2) on the CPU: the hostsim build of the device code (tests/hostsim) against the
reference's recorded answers (tests/golden/fixed_base.json) and against the Python-integer model of
tests/fixed_base_checks.py on random batches; handles, widths, memory accounting and every refusal."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import fixed_base_checks as FB  # noqa: E402

OPTIONAL = ("ellgpu_probe_valu", "ellgpu_ctx_set_timing", "ellgpu_ctx_get_timing", "ellgpu_debug_field_op")
E_ARG, E_NOMEM, E_UNSUPPORTED = -2, -4, -5


@pytest.fixture(scope="module")
def hs():
    return _lib.load(build_hostsim(), optional=OPTIONAL)


@pytest.fixture(scope="module")
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batches():
    """one 203-item batch per curve and the model's answers, shared by every size"""
    return {name: FB.random_batch(FB.spec_of(name), 203, 1) for name in FB.NAMES}


def _code(call):
    with pytest.raises(_lib.EllgpuError) as e:
        call()
    return e.value.code


def test_curve_set():
    assert [c["name"] for c in FB.curves()] == FB.NAMES
    for name in FB.NAMES:
        s = FB.spec_of(name)
        m, pts = FB.model_of(s), FB.bases_of(s)
        assert len(pts) == 4 and all(m.on_curve(P) for P in pts)
        assert pts[1] == m.add(pts[0], pts[0]) and pts[2] == m.neg(pts[0])
        assert m.mul(FB.I(s["n"]), pts[0]) is None and len(s["k"]) == 54 and len(s["pairs"]) == 13
        ks = [FB.I(k) for k in s["k"]]
        n, B = FB.I(s["n"]), s["B"]
        assert ks[:7] == [0, 1, 2, n - 1, n, n + 1, (1 << (8 * B)) - 1]
        for lo, hi in ((15, 16), (3, 4), (7, 8), (11, 12), (21, 22)):
            assert {1 << lo, (1 << lo) + 1, (1 << hi) - 1, 1 << hi} <= set(ks)
    cof = FB.spec_of("cof_p10007")
    m = FB.model_of(cof)
    T = tuple(FB.I(v) for v in cof["refused"][0])
    assert m.on_curve(T) and T[1] == 0 and FB.I(cof["order"]) == 2 * FB.I(cof["n"]) and FB.I(cof["n"]) > 255


@pytest.mark.parametrize("name", FB.NAMES)
def test_model_is_pinned_to_the_fixture(name):
    FB.check_model_pinned(FB.spec_of(name))


@pytest.mark.parametrize("name", FB.NAMES)
def test_golden(ctx, name):
    """every recorded case at every width the CPU build walks, through both memory kinds: the
    bytes are the same"""
    spec = FB.spec_of(name)
    for width in FB.widths_of(name):
        a = FB.check_golden(ctx, spec, width, "host")
        b = FB.check_golden(ctx, spec, width, "dev_np")
        assert all((u[0] == v[0]).all() and (u[1] == v[1]).all() for u, v in zip(a, b))


@pytest.mark.parametrize("name", FB.NAMES)
def test_model_meets_the_conditions(batches, name):
    assert FB.model_meets_conditions(FB.spec_of(name), batches[name])


@pytest.mark.parametrize("name", FB.NAMES)
def test_random_batch_matches_model(ctx, batches, name):
    """n = 1, 8, 9, 41, 203: the hostsim small-call and chunk edges (one set of tables per curve)"""
    spec = FB.spec_of(name)
    _, hs_ = FB.define_bases(ctx, spec, 8 if name in FB.SIGNED else 0)
    try:
        for n in (1, 8, 9, 41, 203):
            a = FB.check_batch(ctx, spec, batches[name], n, hs_, "host")
            b = FB.check_batch(ctx, spec, batches[name], n, hs_, "dev_np")
            assert all((u == v).all() for u, v in zip(a, b))
    finally:
        for h in hs_:
            ctx.release_base(h)


def test_two_widths_in_one_call(ctx, batches):
    """mul_base2 over a 4-bit and an 8-bit table: each walk reads its own table's header"""
    for name in FB.SIGNED:
        spec, bt = FB.spec_of(name), batches[name]
        pts, B = FB.bases_of(spec), spec["B"]
        h1 = ctx.define_base(name, FB.xy_bytes(pts[0], B), 4)
        h2 = ctx.define_base(name, FB.xy_bytes(pts[2], B), 8)
        try:
            assert ctx.base_info(h1)[1] == 4 and ctx.base_info(h2)[1] == 8
            xy, inf = FB.run_mul2(ctx, h1, h2, bt["k1"][:41], bt["k2"][:41], B)
            assert (inf == bt["inf2"][:41]).all() and (xy == bt["xy2"][:41]).all()
        finally:
            ctx.release_base(h1)
            ctx.release_base(h2)


def test_handles(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        spec = FB.spec_of("p192")
        pts = FB.bases_of(spec)
        m = FB.model_of(spec)
        xy = [FB.xy_bytes(P, 24) for P in pts]
        h0 = c.define_base("p192", xy[0])
        assert c.define_base("p192", xy[0]) == h0 == c.define_base("p192", xy[0], 8)
        h1 = c.define_base("p192", xy[1])
        assert h1 != h0
        c.release_base(h0)
        h2 = c.define_base("p192", xy[0])
        assert h2 not in (h0, h1)                                   # never reused
        # a released handle is an argument error in every call
        k = np.ones((1, 24), np.uint8)
        for call in (lambda: c.release_base(h0), lambda: c.base_info(h0), lambda: c.mul_base(h0, k),
                     lambda: c.mul_base2(h0, h1, k, k), lambda: c.mul_base2(h1, h0, k, k)):
            assert _code(call) == E_ARG
        # the 17th live base
        P, live = pts[3], [h1, h2]
        while len(live) < 16:
            P = m.add(P, pts[0])
            live.append(c.define_base("p192", FB.xy_bytes(P, 24)))
        assert len(set(live)) == 16
        P = m.add(P, pts[0])
        assert _code(lambda: c.define_base("p192", FB.xy_bytes(P, 24))) == E_UNSUPPORTED
        assert c.define_base("p192", xy[1]) == h1                   # an existing one is still found
        c.release_base(live[-1])
        assert c.define_base("p192", FB.xy_bytes(P, 24)) > max(live)
    finally:
        c.close()


def test_base_info(ctx):
    for name, B, aff in (("p192", 24, 48), ("p384", 48, 96), ("secp256k1", 32, 64)):
        spec = FB.spec_of(name)
        h = ctx.define_base(name, FB.xy_bytes(FB.bases_of(spec)[3], B), 8)
        cid, bits, size = ctx.base_info(h)
        assert cid == elliptic_amd.engine.CURVE_ID[name] and bits == 8
        entries = 33 * 128 if name in FB.SIGNED else B * 255         # signed: 257 bits in 8-bit windows, half a window each
        assert size % (entries + 1) == 0 and size // (entries + 1) >= aff
        ctx.release_base(h)
    h = ctx.define_base("secp256k1", FB.xy_bytes(FB.bases_of(FB.spec_of("secp256k1"))[3], 32), 4)
    assert ctx.base_info(h)[1] == 4 and ctx.base_info(h)[2] % (65 * 8 + 1) == 0
    ctx.release_base(h)


@pytest.mark.parametrize("name", FB.PRESETS + ["brainpoolP256r1"])
def test_generator_alias_and_by_coordinates(ctx, name):
    """xy == NULL aliases the curve's own table: the same bytes as ellgpu_mul_fixed, also after
    release; G by coordinates at width 8 gives them too"""
    spec = FB.spec_of(name)
    B = spec["B"]
    cid = FB.curve_id(ctx, spec)
    k = FB.rows([FB.I(v) for v in spec["k"]], B)
    want = ctx.mul_fixed(cid, k)
    alias = ctx.define_base(cid)
    assert ctx.define_base(cid) == alias
    for mem in ("host", "dev_np"):
        xy, inf = FB.run_mul(ctx, alias, k, B, mem)
        assert (xy == want[0]).all() and (inf == want[1]).all()
    info = ctx.base_info(alias)
    assert info[1] == ctx.comb_bits(cid) if isinstance(cid, str) else info[1] == 8
    assert info[2] > 0
    assert _code(lambda: ctx.define_base(cid, None, 8)) == E_ARG
    ctx.release_base(alias)
    again = ctx.mul_fixed(cid, k)
    assert (again[0] == want[0]).all() and (again[1] == want[1]).all()
    g = ctx.define_base(cid, FB.xy_bytes(FB.bases_of(spec)[0], B), 8)
    xy, inf = FB.run_mul(ctx, g, k, B)
    assert (xy == want[0]).all() and (inf == want[1]).all()
    # v * G + r * H with G the alias
    alias = ctx.define_base(cid)
    hb = ctx.define_base(cid, FB.xy_bytes(FB.bases_of(spec)[3], B), 8)
    pa = FB.run_mul2(ctx, alias, hb, k, k[::-1], B)
    pb = FB.run_mul2(ctx, g, hb, k, k[::-1], B)
    assert (pa[0] == pb[0]).all() and (pa[1] == pb[1]).all()
    for h in (g, hb, alias):
        ctx.release_base(h)


def test_refusals(hs, ctx):
    spec = FB.spec_of("p256")
    pts = FB.bases_of(spec)
    p256 = FB.model_of(spec).p
    good = FB.xy_bytes(pts[3], 32)
    x, y = pts[3]
    # off the curve, and coordinates >= p (x + p fits in 32 bytes on no preset but p256's p < 2^256)
    bad_points = [FB.xy_bytes((x, y ^ 1), 32), FB.xy_bytes((x ^ 1, y), 32), bytes(64),
                  FB.xy_bytes((x + p256, y), 32) if x + p256 < 1 << 256 else FB.xy_bytes((p256, 0), 32),
                  FB.xy_bytes((p256, y), 32), FB.xy_bytes((x, p256), 32), b"\xff" * 64]
    for xy in bad_points:
        assert _code(lambda: ctx.define_base("p256", xy, 8)) == E_ARG
    # a point given as x + p where that fits: secp192k1's p is 192 bits in a 32-byte coordinate
    s192 = FB.spec_of("secp192k1")
    cid192 = FB.curve_id(ctx, s192)
    gx, gy = FB.bases_of(s192)[0]
    assert _code(lambda: ctx.define_base(cid192, FB.xy_bytes((gx + FB.I(s192["p"]), gy), 32))) == E_ARG
    assert _code(lambda: ctx.define_base(cid192, FB.xy_bytes((gx, gy ^ 1), 32))) == E_ARG
    assert _code(lambda: ctx.define_base(cid192)) == E_ARG            # a plain id has no generator
    # widths per comb kind
    for w in (1, 2, 3, 5, 6, 10, 20, 21, 23, 24, 32, -1):
        assert _code(lambda: ctx.define_base("p256", good, w)) == E_ARG
        assert _code(lambda: ctx.define_base("secp256k1", FB.xy_bytes(FB.bases_of(FB.spec_of("secp256k1"))[0], 32), w)) == E_ARG
    p384 = FB.xy_bytes(FB.bases_of(FB.spec_of("p384"))[0], 48)
    for w in (4, 12, 16, 22, 7, -8):
        assert _code(lambda: ctx.define_base("p384", p384, w)) == E_ARG
        assert _code(lambda: ctx.define_base(cid192, FB.xy_bytes((gx, gy), 32), w)) == E_ARG
    # curves
    ed = ctx.define_edwards((1 << 255) - 19, -1 % ((1 << 255) - 19), 121665)
    mont = ctx.define_mont((1 << 255) - 19, 486662)
    for cid in ("ed25519", "curve25519", ed, mont):
        assert _code(lambda: ctx.define_base(cid, good, 0)) == E_UNSUPPORTED
        assert _code(lambda: ctx.define_base(cid)) == E_UNSUPPORTED
    for cid in (8, 15, 31, 32, 99, -1):
        assert _code(lambda: ctx.define_base(cid, good, 0)) == E_ARG
    # mixed curves, memory kinds, streams, null pointers
    h256 = ctx.define_base("p256", good, 8)
    h384 = ctx.define_base("p384", p384)
    P = lambda a: a.ctypes.data
    k, k48 = np.ones((1, 32), np.uint8), np.ones((1, 48), np.uint8)
    oxy, oinf = np.zeros((1, 96), np.uint8), np.zeros(1, np.uint8)
    assert _code(lambda: ctx.mul_base2(h256, h384, k, k)) == E_ARG
    assert hs.ellgpu_mul_base2(ctx._ctx, h384, h256, 1, P(k48), P(k48), P(oxy), P(oinf), 0, None) == E_ARG
    assert b"different curves" in hs.ellgpu_last_error()
    one = [P(k), P(oxy), P(oinf)]
    two = [P(k), P(k), P(oxy), P(oinf)]
    for mem in (2, -1, 7):
        assert hs.ellgpu_mul_base(ctx._ctx, h256, 1, *one, mem, None) == E_ARG
        assert hs.ellgpu_mul_base2(ctx._ctx, h256, h256, 1, *two, mem, None) == E_ARG
    stream = ctypes.c_void_p(0x1000)
    assert hs.ellgpu_mul_base(ctx._ctx, h256, 1, *one, 0, stream) == E_ARG
    assert hs.ellgpu_mul_base2(ctx._ctx, h256, h256, 1, *two, 0, stream) == E_ARG
    for mem in (0, 1):
        assert hs.ellgpu_mul_base(ctx._ctx, h256, 1, *one, mem, None) == 0
        assert hs.ellgpu_mul_base2(ctx._ctx, h256, h256, 1, *two, mem, None) == 0
        for j in range(3):
            args = list(one)
            args[j] = None
            assert hs.ellgpu_mul_base(ctx._ctx, h256, 1, *args, mem, None) == E_ARG
            assert hs.ellgpu_last_error() == b"null pointer"
        for j in range(4):
            args = list(two)
            args[j] = None
            assert hs.ellgpu_mul_base2(ctx._ctx, h256, h256, 1, *args, mem, None) == E_ARG
        assert hs.ellgpu_mul_base(ctx._ctx, h256, 0, None, None, None, mem, None) == 0
        assert hs.ellgpu_mul_base2(ctx._ctx, h256, h256, 0, None, None, None, None, mem, None) == 0
        assert hs.ellgpu_mul_base(None, h256, 0, None, None, None, mem, None) == E_ARG
    # device memory: operands and results must not overlap
    buf = np.ones((1, 64), np.uint8)
    assert hs.ellgpu_mul_base(ctx._ctx, h256, 1, P(buf), P(buf), P(oinf), 1, None) == E_ARG
    assert hs.ellgpu_mul_base2(ctx._ctx, h256, h256, 1, P(k), P(buf), P(buf), P(oinf), 1, None) == E_ARG
    out = ctypes.c_int(-1)
    assert hs.ellgpu_base_define(ctx._ctx, 3, good, 8, None) == E_ARG
    assert hs.ellgpu_base_define(None, 3, good, 8, ctypes.byref(out)) == E_ARG
    assert hs.ellgpu_base_info(ctx._ctx, h256, None, None, None) == 0
    ctx.release_base(h256)
    ctx.release_base(h384)
    assert hs.ellgpu_version() == 0x000200


def test_comb_max_bytes(hs, monkeypatch):
    """ELLGPU_COMB_MAX_BYTES applies per table: an explicit width that does not fit is NOMEM, the
    default width narrows and base_info shows it"""
    spec = FB.spec_of("secp256k1")
    pts = FB.bases_of(spec)
    # an 8-bit signed table: (33 * 128 + 1) entries of 64 bytes = 270 400 bytes; a 4-bit one: 33 344
    monkeypatch.setenv("ELLGPU_COMB_MAX_BYTES", "100000")
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        assert _code(lambda: c.define_base("secp256k1", FB.xy_bytes(pts[0], 32), 8)) == E_NOMEM
        h = c.define_base("secp256k1", FB.xy_bytes(pts[0], 32))
        cid, bits, size = c.base_info(h)
        assert bits == 4 and size <= 100000
        assert c.define_base("secp256k1", FB.xy_bytes(pts[0], 32), 4) == h       # the width in use
        k = FB.rows([FB.I(v) for v in spec["k"]], 32)
        xy, inf = FB.run_mul(c, h, k, 32)
        want = FB.golden_answers(spec)[0][0]
        assert (xy == want[0]).all() and (inf == want[1]).all()
        # the unsigned comb has one width: nothing to narrow to
        p192 = FB.xy_bytes(FB.bases_of(FB.spec_of("p192"))[0], 24)
        assert _code(lambda: c.define_base("p192", p192)) == E_NOMEM
    finally:
        c.close()


def test_small_order_base_is_refused(hs):
    """a base whose table would hold the point at infinity: refused, and nothing is left behind --
    the context still takes 16 bases"""
    spec = FB.spec_of("cof_p10007")
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        cid = FB.curve_id(c, spec)
        T = tuple(FB.I(v) for v in spec["refused"][0])
        for _ in range(3):
            with pytest.raises(_lib.EllgpuError) as e:
                c.define_base(cid, FB.xy_bytes(T, 32))
            assert e.value.code == E_ARG and "point at infinity" in str(e.value)
        m, pts = FB.model_of(spec), FB.bases_of(spec)
        P, live = pts[0], []
        for _ in range(16):
            live.append(c.define_base(cid, FB.xy_bytes(P, 32)))
            P = m.add(P, pts[0])
        assert len(set(live)) == 16
        c.release_base(live[0])
        # order 2 q: no entry d 2^(8w) (T + G) with d < 256 < q is O
        TG = tuple(FB.I(v) for v in spec["accepted_2q"])
        h = c.define_base(cid, FB.xy_bytes(TG, 32))
        k = [0, 1, 2, FB.I(spec["order"]), FB.I(spec["order"]) + 1, (1 << 256) - 1]
        xy, inf = FB.run_mul(c, h, FB.rows(k, 32), 32)
        want = [FB.answer(m.mul(v, TG), 32) for v in k]
        assert inf.tolist() == [w[1] for w in want] == [1, 0, 0, 1, 0, 0]
        assert all((xy[i] == w[0]).all() for i, w in enumerate(want))
    finally:
        c.close()


def _live(hs):
    hs.hs_live_allocs.restype = ctypes.c_long
    return hs.hs_live_allocs()


def test_live_allocations_return_to_their_level(hs, monkeypatch):
    """the CPU backend's count of live allocations after every refused define, after define and
    release, and after a define that arrives at a live table: a preset and a user-defined domain"""
    spec = FB.spec_of("secp256k1")
    pts = [FB.xy_bytes(P, 32) for P in FB.bases_of(spec)]
    x, y = FB.bases_of(spec)[3]
    cof = FB.spec_of("cof_p10007")
    T = FB.xy_bytes(tuple(FB.I(v) for v in cof["refused"][0]), 32)
    cg = FB.xy_bytes(FB.bases_of(cof)[0], 32)
    monkeypatch.setenv("ELLGPU_COMB_MAX_BYTES", "100000")          # 8 bits signed: 270 400 bytes, 4 bits: 33 344
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        cid = FB.curve_id(c, cof)
        c.release_base(c.define_base("secp256k1", pts[3]))          # (the scratch arena has its size from here on)
        level = _live(hs)
        assert _code(lambda: c.define_base("secp256k1", pts[3], 8)) == E_NOMEM and _live(hs) == level
        assert _code(lambda: c.define_base("secp256k1", FB.xy_bytes((x, y ^ 1), 32))) == E_ARG and _live(hs) == level
        h = c.define_base("secp256k1", pts[3], 4)
        assert _live(hs) == level + 1
        assert c.define_base("secp256k1", pts[3]) == h and _live(hs) == level + 1     # narrowed 16 -> 4: the live table
        h2 = c.define_base("secp256k1", pts[1])                     # a default width that narrows, then succeeds
        assert c.base_info(h2)[1] == 4 and _live(hs) == level + 2
        c.release_base(h)
        c.release_base(h2)
        assert _live(hs) == level
        # the unsigned comb of a user-defined id has one width: refused, explicit or default
        assert _code(lambda: c.define_base(cid, cg)) == E_NOMEM and _code(lambda: c.define_base(cid, cg, 8)) == E_NOMEM
        assert _live(hs) == level
    finally:
        c.close()
    monkeypatch.delenv("ELLGPU_COMB_MAX_BYTES")
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        cid = FB.curve_id(c, cof)
        c.release_base(c.define_base(cid, cg))
        level = _live(hs)
        assert _code(lambda: c.define_base(cid, T)) == E_ARG        # small order: refused after the whole build
        assert _live(hs) == level
        gx, gy = FB.bases_of(cof)[0]
        assert _code(lambda: c.define_base(cid, FB.xy_bytes((gx, gy ^ 1), 32))) == E_ARG and _live(hs) == level
        h = c.define_base(cid, cg)
        assert _live(hs) == level + 1
        c.release_base(h)
        assert _live(hs) == level
    finally:
        c.close()


def test_last_entry_of_a_sliced_build(ctx):
    """p256 at 8 bits: 32 x 255 = 8160 entries, built in slices of 1000 with a remainder of 160 --
    the scalar whose only digit is the last entry of the last window, against the model"""
    spec = FB.spec_of("p256")
    P = FB.bases_of(spec)[3]
    h = ctx.define_base("p256", FB.xy_bytes(P, 32), 8)
    try:
        k = [255 << (8 * 31), 255 << (8 * 30), 1 << (8 * 31), 254 << (8 * 31)]
        xy, inf = FB.run_mul(ctx, h, FB.rows(k, 32), 32)
        m = FB.model_of(spec)
        for i, v in enumerate(k):
            want = FB.answer(m.mul(v, P), 32)
            assert inf[i] == want[1] == 0 and (xy[i] == want[0]).all()
    finally:
        ctx.release_base(h)


def test_group_gives_a_single_contexts_bytes(hs, ctx, batches):
    g = elliptic_amd.Context(lib_path=hs, devices=[0, 0])
    try:
        for name in ("secp256k1", "p192", "brainpoolP256r1"):
            spec, bt = FB.spec_of(name), batches[name]
            gid, gh = FB.define_bases(g, spec, 8)
            _, gh2 = FB.define_bases(g, spec, 8, gid)
            assert gh2 == gh
            _, ch = FB.define_bases(ctx, spec, 8)
            a = FB.check_batch(g, spec, bt, 41, gh, "host")
            b = FB.check_batch(ctx, spec, bt, 41, ch, "host")
            assert all((u == v).all() for u, v in zip(a, b))
            for h in gh:
                g.release_base(h)
            for h in ch:
                ctx.release_base(h)
            assert _code(lambda: g.mul_base(gh[0], bt["k"][:1])) == E_ARG
        # all or nothing: a point no member takes leaves no handle behind on any of them
        assert _code(lambda: g.define_base("p192", bytes(48))) == E_ARG
    finally:
        g.close()


def test_mul_fixed_launches_unchanged(hs, ctx):
    """the kernels ellgpu_mul_fixed launches on a preset are the same before and after a base was
    defined and used"""
    spec = FB.spec_of("p256")
    k = FB.rows([FB.I(v) for v in spec["k"]], 32)
    names = [b"mul_fixed", b"normalize", b"comb_gen", b"base_comb_gen", b"mul_base2", b"mul_var", b"base_check"]

    def counts(n):
        hs.hs_launches_reset()
        out = ctx.mul_fixed("p256", k[:n])
        return [hs.hs_launches(nm) for nm in names], out

    ctx.mul_fixed("p256", k[:1])                                   # the curve's own table exists from here on
    before = [counts(n) for n in (1, 9, 54)]
    h = ctx.define_base("p256", FB.xy_bytes(FB.bases_of(spec)[3], 32), 8)
    FB.run_mul(ctx, h, k, 32)
    FB.run_mul2(ctx, h, h, k, k, 32)
    after = [counts(n) for n in (1, 9, 54)]
    ctx.release_base(h)
    for (ca, oa), (cb, ob) in zip(before, after):
        assert ca == cb and ca[3] == ca[4] == ca[6] == 0 and (oa[0] == ob[0]).all() and (oa[1] == ob[1]).all()
    assert all(c[2] == 0 for c, _ in before + after)               # and the curve's own table is not built again
