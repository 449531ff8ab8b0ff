"""Fixed-base tables of caller-chosen points on Edwards curves (ellgpu_ed_base_define, then
ellgpu_mul_base, ellgpu_mul_base2, ellgpu_base_info, ellgpu_base_release on its handles) on the CPU:
the hostsim build of the device code (tests/hostsim) against the reference's recorded answers
(tests/golden/fixed_base_ed.json) and against the engine's own variable-base calls on random batches;
handles, the limit shared with the short curves' bases, and every refusal.

A table costs the CPU build some seconds and a context holds 16, so the tables of G, -G and the PRNG
point are built once per curve (`tables`) and shared by the tests that only walk them; the golden
test adds the other four bases of its curve for as long as it runs."""
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
import fixed_base_ed_checks as FE  # noqa: E402

OPTIONAL = ("ellgpu_probe_valu", "ellgpu_ctx_set_timing", "ellgpu_ctx_get_timing", "ellgpu_debug_field_op")
E_ARG, E_NOMEM, E_UNSUPPORTED = -2, -4, -5
ED_BITS = 8                                    # EdWork::COMB_BITS of the CPU unit-test build
P25519 = (1 << 255) - 19


@pytest.fixture(scope="module")
def hs():
    return _lib.load(build_hostsim(), optional=OPTIONAL)


@pytest.fixture(scope="module")
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tables(ctx):
    """name -> (curve id, {base index: handle}): bases 0, 2 and 3 of the fixture at the default width"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = FE.define_bases(ctx, FE.spec_of(name), which=(0, 2, 3))
        return made[name]
    yield get
    for _, hs_ in made.values():
        FE.release(ctx, hs_)


def _code(call):
    with pytest.raises(_lib.EllgpuError) as e:
        call()
    return e.value.code


def test_curve_set():
    assert [c["name"] for c in FE.curves()] == FE.NAMES
    assert [c["kind"] for c in FE.curves()] == ["preset", "domain", "plain", "domain"]
    for name in FE.NAMES:
        s = FE.spec_of(name)
        m, pts, p, n = FE.model_of(s), FE.bases_of(s), FB.I(s["p"]), FB.I(s["n"])
        assert len(pts) == 7 and all(m.on_curve(P) for P in pts)
        assert pts[1] == m.add(pts[0], pts[0]) and pts[2] == m.neg(pts[0]) and pts[4] == m.ID and pts[5] == (0, p - 1)
        assert m.mul(2, pts[6]) == pts[5] and m.mul(2, pts[5]) == m.ID            # orders 4 and 2
        assert m.mul(n, pts[0]) == m.ID and len(s["k"]) == 42 and len(s["pairs"]) == 15
        ks = [FB.I(k) for k in s["k"]]
        assert ks[:7] == [0, 1, 2, n - 1, n, n + 1, (1 << 256) - 1]
        for lo, hi in ((15, 16), (7, 8)):
            assert {1 << lo, (1 << lo) + 1, (1 << hi) - 1, 1 << hi} <= set(ks)
    a, b = FE.spec_of("ed25519"), FE.spec_of("ed25519_by_hand")
    assert all(a[f] == b[f] for f in ("p", "a", "d", "n", "g"))


@pytest.mark.parametrize("name", FE.NAMES)
def test_model_is_pinned_to_the_fixture(name):
    FE.check_model_pinned(FE.spec_of(name))


@pytest.mark.parametrize("name", FE.NAMES)
def test_golden(ctx, tables, name):
    """every recorded case through both memory kinds: the bytes are the same"""
    spec = FE.spec_of(name)
    cid, shared = tables(name)
    _, rest = FE.define_bases(ctx, spec, 0, cid, which=(1, 4, 5, 6))
    hs_ = {**shared, **rest}
    try:
        assert all(ctx.base_info(h)[1] == 8 for h in hs_.values())
        a = FE.check_golden(ctx, spec, hs_, "host")
        b = FE.check_golden(ctx, spec, hs_, "dev_np")
        assert all((u[0] == v[0]).all() and (u[1] == v[1]).all() for u, v in zip(a, b))
    finally:
        FE.release(ctx, rest)


@pytest.mark.parametrize("name", FE.NAMES)
def test_random_batch_matches_variable_base(ctx, tables, name):
    """mul_base = mul_var and mul_base2 = mul_add2, byte for byte, at n = 1, 8, 9, 41, 203"""
    spec = FE.spec_of(name)
    bt = FE.random_batch(spec, 203, 1)
    assert FE.model_meets_conditions(spec, bt)
    cid, hs_ = tables(name)
    want = FE.variable_base_answers(ctx, cid, spec, bt)
    m, pts = FE.model_of(spec), FE.bases_of(spec)
    for j in range(4):                             # and the rows by construction, against the model
        assert (want["xy"][j] == FE.answer(spec, m.mul(bt["ints"][0][j], pts[3]))[0]).all()
        assert (want["xy2"][j] == FE.answer(spec, m.mul2(bt["ints"][1][j], pts[0], bt["ints"][2][j], pts[2]))[0]).all()
    assert want["inf"][0] == want["inf2"][0] == (1 if spec["kind"] == "preset" else 0)
    for n in (1, 8, 9, 41, 203):
        a = FE.check_batch(ctx, spec, bt, want, n, hs_, "host")
        b = FE.check_batch(ctx, spec, bt, want, n, hs_, "dev_np")
        assert all((u == v).all() for u, v in zip(a, b))


def test_handles_are_shared_with_the_short_bases(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        spec = FE.spec_of("e222")
        cid = FE.curve_id(c, spec)
        m, pts = FE.model_of(spec), FE.bases_of(spec)
        xy = [FB.xy_bytes(P, 32) for P in pts]
        h0 = c.define_ed_base(cid, xy[0])
        assert c.define_ed_base(cid, xy[0]) == h0 == c.define_ed_base(cid, xy[0], 8)      # the width in use
        assert c.base_info(h0) == (cid, 8, (32 * 255 + 1) * 64)
        h1 = c.define_ed_base(cid, xy[1])
        assert h1 != h0
        c.release_base(h0)
        h2 = c.define_ed_base(cid, xy[0])
        assert h2 not in (h0, h1)                                   # never reused
        k = np.ones((1, 32), np.uint8)
        for call in (lambda: c.release_base(h0), lambda: c.base_info(h0), lambda: c.mul_base(h0, k),
                     lambda: c.mul_base2(h0, h1, k, k), lambda: c.mul_base2(h1, h0, k, k)):
            assert _code(call) == E_ARG
        # one list: short bases count towards the 16
        sp = FB.spec_of("p192")
        live = [h1, h2, c.define_base("p192", FB.xy_bytes(FB.bases_of(sp)[0], 24)), c.define_ed_base("ed25519"),
                c.define_base("p192")]
        assert len(set(live)) == 5
        P = FB.bases_of(sp)[0]
        ms = FB.model_of(sp)
        while len(live) < 16:
            P = ms.add(P, FB.bases_of(sp)[0])
            live.append(c.define_base("p192", FB.xy_bytes(P, 24)))
        assert len(set(live)) == 16
        assert _code(lambda: c.define_ed_base(cid, xy[3])) == E_UNSUPPORTED
        assert _code(lambda: c.define_ed_base("ed25519", FB.xy_bytes(FE.bases_of(FE.spec_of("ed25519"))[3], 32))) == E_UNSUPPORTED
        assert c.define_ed_base(cid, xy[1]) == h1                   # an existing one is still found
        c.release_base(live[-1])
        assert c.define_ed_base(cid, xy[3]) > max(live)
        # a short handle beside an Edwards handle: different curves
        assert _code(lambda: c.mul_base2(h1, live[2], k, k)) == E_ARG
        assert b"different curves" in hs.ellgpu_last_error()
        assert _code(lambda: c.mul_base2(live[2], h1, np.ones((1, 24), np.uint8), np.ones((1, 24), np.uint8))) == E_ARG
        assert _code(lambda: c.mul_base2(h1, live[3], k, k)) == E_ARG            # e222 beside ed25519
    finally:
        c.close()


def test_generator_alias_on_ed25519(ctx, tables):
    """xy == NULL aliases the curve's own table: the bytes of ellgpu_mul_fixed, also after release; G
    by coordinates gives them too, and 0 and the comb's own width name one table"""
    spec = FE.spec_of("ed25519")
    k = FB.rows([FB.I(v) for v in spec["k"]], 32)
    want = ctx.mul_fixed("ed25519", k)
    alias = ctx.define_ed_base("ed25519")
    assert ctx.define_ed_base("ed25519") == alias
    for mem in ("host", "dev_np"):
        xy, inf = FB.run_mul(ctx, alias, k, 32, mem)
        assert (xy == want[0]).all() and (inf == want[1]).all()
    assert ctx.base_info(alias) == (6, ED_BITS, (256 // ED_BITS) * ((1 << ED_BITS) - 1) * 128)
    assert _code(lambda: ctx.define_ed_base("ed25519", None, ED_BITS)) == E_ARG
    ctx.release_base(alias)
    again = ctx.mul_fixed("ed25519", k)
    assert (again[0] == want[0]).all() and (again[1] == want[1]).all()
    gxy = FB.xy_bytes(FE.bases_of(spec)[0], 32)
    g = tables("ed25519")[1][0]                    # (shared: not released here)
    assert ctx.define_ed_base("ed25519", gxy) == g == ctx.define_ed_base("ed25519", gxy, ED_BITS) and ctx.base_info(g)[1:] == ctx.base_info(ctx.define_ed_base("ed25519"))[1:]
    xy, inf = FB.run_mul(ctx, g, k, 32)
    assert (xy == want[0]).all() and (inf == want[1]).all()
    alias = ctx.define_ed_base("ed25519")
    pa = FB.run_mul2(ctx, alias, g, k, k[::-1], 32)
    pb = FB.run_mul2(ctx, g, g, k, k[::-1], 32)
    assert (pa[0] == pb[0]).all() and (pa[1] == pb[1]).all()
    # the curve's own table is a table of G by coordinates: the first and the last entry of every
    # window, 0 and the all-ones scalar through the alias, the handle of G and mul_fixed
    top = (1 << ED_BITS) - 1
    ends = [d << (ED_BITS * w) for w in range(256 // ED_BITS) for d in (1, top)] + [0, (1 << 256) - 1]
    ke = FB.rows(ends, 32)
    fixed = ctx.mul_fixed("ed25519", ke)
    for h in (alias, g):
        xy, inf = FB.run_mul(ctx, h, ke, 32)
        assert (xy == fixed[0]).all() and (inf == fixed[1]).all()
    m, G = FE.model_of(spec), FE.bases_of(spec)[0]
    for i in (0, 1, len(ends) - 4, len(ends) - 3, len(ends) - 1):
        assert (fixed[0][i] == FE.answer(spec, m.mul(ends[i], G))[0]).all()
    ctx.release_base(alias)


def test_last_entry_of_a_sliced_build(ctx, tables):
    """Curve1174 at 8 bits: 32 x 255 = 8160 entries, built in slices of 1000 with a remainder of
    160 -- the scalar whose only digit is the last entry of the last window, against the model"""
    spec = FE.spec_of("curve1174")
    _, hs_ = tables("curve1174")
    m, P = FE.model_of(spec), FE.bases_of(spec)[3]
    k = [255 << 248, 255 << 240, 1 << 248, 254 << 248]
    xy, inf = FB.run_mul(ctx, hs_[3], FB.rows(k, 32), 32)
    for i, v in enumerate(k):
        assert inf[i] == 0 and (xy[i] == FE.answer(spec, m.mul(v, P))[0]).all()


def _live(hs):
    hs.hs_live_allocs.restype = ctypes.c_long
    return hs.hs_live_allocs()


def test_live_allocations_return_to_their_level(hs, monkeypatch):
    """the CPU backend's count of live allocations after every refused define and after define and
    release, on ed25519 and on a user-defined Edwards curve"""
    e222, ed = FE.spec_of("e222"), FE.spec_of("ed25519")
    xy = FB.xy_bytes(FE.bases_of(e222)[3], 32)
    x, y = FE.bases_of(e222)[3]
    exy = FB.xy_bytes(FE.bases_of(ed)[3], 32)
    ex, ey = FE.bases_of(ed)[3]
    one = np.ones((1, 32), np.uint8)
    monkeypatch.setenv("ELLGPU_COMB_MAX_BYTES", "600000")          # 8 bits: 522 304 bytes; ed25519's: 1 044 480
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        cid = FE.curve_id(c, e222)
        c.release_base(c.define_ed_base(cid, xy))                   # (the scratch arena has its size from here on)
        level = _live(hs)
        assert _code(lambda: c.define_ed_base(cid, xy, 16)) == E_NOMEM and _live(hs) == level
        assert _code(lambda: c.define_ed_base(cid, FB.xy_bytes((x, y ^ 1), 32))) == E_ARG and _live(hs) == level
        assert _code(lambda: c.define_ed_base("ed25519", exy)) == E_NOMEM and _live(hs) == level
        h = c.define_ed_base(cid, xy)
        assert _live(hs) == level + 1 and c.define_ed_base(cid, xy, 8) == h and _live(hs) == level + 1
        c.release_base(h)
        assert _live(hs) == level
        # the curve's own comb is not subject to the limit (it never was): one more allocation, the table
        c.mul_fixed("ed25519", one)
        grown = _live(hs)
        c.mul_fixed("ed25519", one)
        assert grown > level and _live(hs) == grown
    finally:
        c.close()
    monkeypatch.delenv("ELLGPU_COMB_MAX_BYTES")
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        c.release_base(c.define_ed_base("ed25519", exy))
        level = _live(hs)
        assert _code(lambda: c.define_ed_base("ed25519", FB.xy_bytes((ex, ey ^ 1), 32))) == E_ARG and _live(hs) == level
        h = c.define_ed_base("ed25519", exy)
        assert _live(hs) == level + 1
        c.release_base(h)
        assert _live(hs) == level
    finally:
        c.close()


def test_generator_of_an_edwards_domain(ctx, tables):
    """xy == NULL on a domain: a table of the domain's G that the handle owns -- the handle of G by
    coordinates at the default width; on a plain id there is no generator"""
    cid, hs_ = tables("curve1174")
    assert ctx.define_ed_base(cid) == hs_[0]
    assert ctx.base_info(hs_[0]) == (cid, 8, (32 * 255 + 1) * 64)
    assert _code(lambda: ctx.define_ed_base(cid, None, 8)) == E_ARG
    plain, _ = tables("e222")
    assert _code(lambda: ctx.define_ed_base(plain)) == E_ARG


def test_refusals(hs, ctx, tables):
    spec = FE.spec_of("curve1174")
    cid, hs_ = tables("curve1174")
    p = FB.I(spec["p"])
    x, y = FE.bases_of(spec)[3]
    good = FB.xy_bytes((x, y), 32)
    # off the curve, and coordinates >= p (p has 251 bits: x + p fits in 32 bytes)
    bad_points = [FB.xy_bytes((x, y ^ 1), 32), FB.xy_bytes((x ^ 1, y), 32), bytes(64), FB.xy_bytes((x + p, y), 32),
                  FB.xy_bytes((x, y + p), 32), FB.xy_bytes((0, p + 1), 32), FB.xy_bytes((p, 1), 32), b"\xff" * 64]
    for xy in bad_points:
        assert _code(lambda: ctx.define_ed_base(cid, xy, 8)) == E_ARG
    ex, ey = FE.bases_of(FE.spec_of("ed25519"))[3]
    for xy in (FB.xy_bytes((ex, ey ^ 1), 32), FB.xy_bytes((0, P25519 + 1), 32), FB.xy_bytes((P25519, 1), 32), bytes(64)):
        assert _code(lambda: ctx.define_ed_base("ed25519", xy)) == E_ARG
    # widths
    for w in (1, 4, 7, 9, 12, 15, 17, 22, 32, -8):
        assert _code(lambda: ctx.define_ed_base(cid, good, w)) == E_ARG
    for w in (1, 4, 12, 22, 32, -8) + ((16,) if ED_BITS != 16 else (8,)):
        assert _code(lambda: ctx.define_ed_base("ed25519", FB.xy_bytes((ex, ey), 32), w)) == E_ARG
    # curves: short ids belong to ellgpu_base_define, and the message says so
    s192 = FB.spec_of("secp192k1")
    short = ctx.define_short(FB.I(s192["p"]), FB.I(s192["a"]), FB.I(s192["b"]))
    mont = ctx.define_mont(P25519, 486662)
    for c in ("secp256k1", "p521", short):
        with pytest.raises(_lib.EllgpuError) as e:
            ctx.define_ed_base(c, good)
        assert e.value.code == E_UNSUPPORTED and "ellgpu_base_define" in str(e.value)
        assert _code(lambda: ctx.define_ed_base(c)) == E_UNSUPPORTED
    for c in ("curve25519", mont):
        assert _code(lambda: ctx.define_ed_base(c, good)) == E_UNSUPPORTED
        assert _code(lambda: ctx.define_ed_base(c)) == E_UNSUPPORTED
    for c in (31, 32, 99, -1):
        assert _code(lambda: ctx.define_ed_base(c, good)) == E_ARG
    # ellgpu_base_define refuses these ids as it did
    for c in ("ed25519", "curve25519", cid, tables("e222")[0], mont):
        assert _code(lambda: ctx.define_base(c, good, 0)) == E_UNSUPPORTED
        assert _code(lambda: ctx.define_base(c)) == E_UNSUPPORTED
    # memory kinds, streams, null pointers, overlap: the checks of the existing calls hold for these handles
    h = hs_[3]
    P = lambda a: a.ctypes.data
    k = np.ones((1, 32), np.uint8)
    oxy, oinf = np.zeros((1, 64), np.uint8), np.zeros(1, np.uint8)
    one, two = [P(k), P(oxy), P(oinf)], [P(k), P(k), P(oxy), P(oinf)]
    for mem in (2, -1):
        assert hs.ellgpu_mul_base(ctx._ctx, h, 1, *one, mem, None) == E_ARG
        assert hs.ellgpu_mul_base2(ctx._ctx, h, h, 1, *two, mem, None) == E_ARG
    assert hs.ellgpu_mul_base(ctx._ctx, h, 1, *one, 0, ctypes.c_void_p(0x1000)) == E_ARG
    for mem in (0, 1):
        assert hs.ellgpu_mul_base(ctx._ctx, h, 1, *one, mem, None) == 0
        assert hs.ellgpu_mul_base2(ctx._ctx, h, h, 1, *two, mem, None) == 0
        for j in range(3):
            args = list(one)
            args[j] = None
            assert hs.ellgpu_mul_base(ctx._ctx, h, 1, *args, mem, None) == E_ARG
        for j in range(4):
            args = list(two)
            args[j] = None
            assert hs.ellgpu_mul_base2(ctx._ctx, h, h, 1, *args, mem, None) == E_ARG
        assert hs.ellgpu_mul_base(ctx._ctx, h, 0, None, None, None, mem, None) == 0
        assert hs.ellgpu_mul_base2(ctx._ctx, h, h, 0, None, None, None, None, mem, None) == 0
    buf = np.ones((1, 64), np.uint8)
    assert hs.ellgpu_mul_base(ctx._ctx, h, 1, P(buf), P(buf), P(oinf), 1, None) == E_ARG
    out = ctypes.c_int(-1)
    assert hs.ellgpu_ed_base_define(ctx._ctx, 6, good, 0, None) == E_ARG
    assert hs.ellgpu_ed_base_define(None, 6, good, 0, ctypes.byref(out)) == E_ARG
    assert hs.ellgpu_version() == 0x000200


def test_comb_max_bytes(hs, monkeypatch):
    """ELLGPU_COMB_MAX_BYTES applies per table: a width that does not fit is NOMEM, explicit or default
    (the default is the narrowest width there is)"""
    monkeypatch.setenv("ELLGPU_COMB_MAX_BYTES", "600000")          # 8 bits: 522 304 bytes; 16 bits: 67 MB
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        spec = FE.spec_of("e222")
        cid = FE.curve_id(c, spec)
        xy = FB.xy_bytes(FE.bases_of(spec)[0], 32)
        assert _code(lambda: c.define_ed_base(cid, xy, 16)) == E_NOMEM
        h = c.define_ed_base(cid, xy)
        assert c.base_info(h)[1:] == (8, 522304)
        assert _code(lambda: c.define_ed_base("ed25519", FB.xy_bytes(FE.bases_of(FE.spec_of("ed25519"))[0], 32))) == E_NOMEM
        c.release_base(h)
    finally:
        c.close()
    monkeypatch.setenv("ELLGPU_COMB_MAX_BYTES", "500000")
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        cid = FE.curve_id(c, FE.spec_of("e222"))
        assert _code(lambda: c.define_ed_base(cid, xy)) == E_NOMEM
        assert _code(lambda: c.define_ed_base(cid, xy, 8)) == E_NOMEM
    finally:
        c.close()


def test_group_gives_a_single_contexts_bytes(hs, ctx, tables):
    g = elliptic_amd.Context(lib_path=hs, devices=[0, 0])
    try:
        spec = FE.spec_of("e222")
        bt = FE.random_batch(spec, 41, 1)
        gid, gh = FE.define_bases(g, spec, 8, which=(0, 2, 3))
        assert FE.define_bases(g, spec, 8, gid, which=(0, 2, 3))[1] == gh
        cid, ch = tables("e222")
        want = FE.variable_base_answers(ctx, cid, spec, bt)
        FE.check_batch(g, spec, bt, want, 41, gh, "host")
        FE.release(g, gh)
        assert _code(lambda: g.mul_base(gh[0], bt["k"][:1])) == E_ARG
        # all or nothing: a point no member takes leaves no handle behind on any of them
        assert _code(lambda: g.define_ed_base(gid, bytes(64))) == E_ARG
        assert g.define_ed_base("ed25519") == g.define_ed_base("ed25519")
    finally:
        g.close()


def test_launches(hs, ctx, tables):
    """the kernels behind the calls carry their own names (ellgpu_ctx_get_timing shows them): every
    chunk of a call is one launch of the walk and one normalisation, at every n, and nothing of the
    variable-base ladder or of the table build runs again"""
    spec = FE.spec_of("curve1174")
    _, hs_ = tables("curve1174")
    k = FB.rows([FB.I(v) for v in spec["k"]], 32)
    names = [b"edc_mul_base", b"edc_mul_base2", b"edc_normalize", b"edc_mul_var", b"ed_base_comb_gen", b"edc_base_check"]
    for n in (1, 9, 42):
        hs.hs_launches_reset()
        FB.run_mul(ctx, hs_[3], k[:n], 32)
        got = [hs.hs_launches(nm) for nm in names]
        assert got[0] == got[2] >= 1 and got[1:2] + got[3:] == [0, 0, 0, 0]
        hs.hs_launches_reset()
        FB.run_mul2(ctx, hs_[0], hs_[3], k[:n], k[:n], 32, "dev_np")
        assert [hs.hs_launches(nm) for nm in names] == [0, 1, 1, 0, 0, 0]
    e = FE.spec_of("ed25519")
    a = ctx.define_ed_base("ed25519", FB.xy_bytes(FE.bases_of(e)[1], 32))
    for n in (1, 9, 42):
        hs.hs_launches_reset()
        FB.run_mul(ctx, a, k[:n], 32, "dev_np")
        FB.run_mul2(ctx, a, a, k[:n], k[:n], 32, "dev_np")
        assert [hs.hs_launches(nm) for nm in (b"ed_mul_fixed", b"ed_mul_base2", b"ed_normalize", b"ed_mul_var")] == [1, 1, 2, 0]
    ctx.release_base(a)
