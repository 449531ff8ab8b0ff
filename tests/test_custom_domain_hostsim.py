"""ECDSA on user-defined domains (ellgpu_curve_define_short_domain) on the CPU: the hostsim build
of the device code (tests/hostsim) against the reference's recorded verdicts and points
(tests/golden/custom_ecdsa.json) and against the C oracle on random batches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import custom_domain_checks as CD  # noqa: E402

NAMES = [c["name"] for c in CD.curves()]


@pytest.fixture(scope="module")
def hs():
    return _lib.load(build_hostsim(), optional=("ellgpu_probe_valu", "ellgpu_ctx_set_timing",
                                                "ellgpu_ctx_get_timing", "ellgpu_debug_field_op"))


@pytest.fixture(scope="module")
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


def _spec(name):
    return next(c for c in CD.curves() if c["name"] == name)


@pytest.mark.parametrize("name", NAMES)
def test_domain_verify_golden(ctx, name):
    """every EC#verify verdict the reference recorded: valid signatures, wrong digests and keys,
    r / s at 0, n, n + 1, 2^256 - 1, digests of 20..64 bytes, msgBitLength, u1 G + u2 Q = O,
    x(R) >= n (eqXToP's later candidates), r = x + p where n > p (accepted), off-curve keys"""
    assert CD.check_verify_golden(ctx, _spec(name)) >= 38


@pytest.mark.parametrize("name", NAMES)
def test_domain_points_golden(ctx, name):
    """k*G through the domain's comb for any 32-byte k (n, n + 1, 2^256 - 1: not reduced mod n)
    and k1*G + k2*Q with p1 = None"""
    assert CD.check_points_golden(ctx, _spec(name)) == 32


@pytest.mark.parametrize("name", NAMES)
def test_domain_random_batch_matches_oracle(ctx, name):
    """4 096 items per curve: the verdicts known by construction, the rest equal the C oracle"""
    spec = _spec(name)
    cid = CD.define(ctx, spec)
    h, r, s, q, expect = CD.random_batch(spec, 4096, seed=sum(map(ord, name)))
    ok, st = ctx.ecdsa_verify(cid, h, r, s, q, status=True)
    want = CD.oracle_verify(spec, h, r, s, q)
    assert not st.any()
    assert (ok == want).all(), np.nonzero(ok != want)[0][:10]
    known = [i for i, e in enumerate(expect) if e is not None]
    assert len(known) > 1500 and all(ok[i] == 1 for i in known)
    assert 0 < int(ok.sum()) < len(ok)


def test_plain_curve_ids_still_refuse(ctx):
    """a define_short id keeps answering ELLGPU_E_UNSUPPORTED for k*G, mulAdd without p1 and verify;
    the domain over the same (p, a, b) is a different id"""
    spec = _spec("brainpoolP256r1")
    p, a, b = CD.params(spec)[:3]
    plain = ctx.define_short(p, a, b)
    dom = CD.define(ctx, spec)
    assert dom != plain and CD.define(ctx, spec) == dom
    k = np.zeros((1, 32), np.uint8)
    q = np.zeros((1, 64), np.uint8)
    for call in (lambda: ctx.mul_fixed(plain, k), lambda: ctx.mul_add2(plain, k, None, k, q),
                 lambda: ctx.ecdsa_verify(plain, np.zeros((1, 32), np.uint8), k, k, q)):
        with pytest.raises(_lib.EllgpuError) as e:
            call()
        assert e.value.code == -5
    # and the rest of the C ABI stays refused on a domain id
    with pytest.raises(_lib.EllgpuError) as e:
        ctx.ecdsa_sign(dom, np.zeros((1, 32), np.uint8), np.ones((1, 32), np.uint8), np.ones((1, 32), np.uint8))
    assert e.value.code == -5
    with pytest.raises(_lib.EllgpuError) as e:
        ctx.decompress(dom, np.zeros((1, 32), np.uint8), np.zeros(1, np.uint8))
    assert e.value.code == -5


def test_bad_domains_are_refused(ctx):
    spec = _spec("secp192k1")
    p, a, b, n, gx, gy = CD.params(spec)
    bad = [
        (p + 1, a, b, n, gx, gy),              # even p
        (3, 0, 1, 5, 0, 1),                    # p <= 3
        (p, a, b, n + 1, gx, gy),              # even n
        (p, a, b, 1, gx, gy),                  # n < 3
        (p, a, b, n, gx, gy + 1),              # G off the curve
        (p, a, b, n, gx + p, gy),              # a coordinate >= p
        (p, 0, 0, n, 0, 0),                    # 4a^3 + 27b^2 = 0 (G = (0, 0) is on y^2 = x^3)
    ]
    for args in bad:
        with pytest.raises(_lib.EllgpuError) as e:
            ctx.define_short_domain(*args)
        assert e.value.code == -2, args


def test_group_context_matches_single(hs):
    """a group of two contexts registers the domain on both members and splits a batch over them:
    the same verdicts as a single context"""
    spec = _spec("w25519_like")
    h, r, s, q, _ = CD.random_batch(spec, 600, seed=7)
    single = elliptic_amd.Context(0, lib_path=hs)
    group = elliptic_amd.Context(lib_path=hs, devices=[0, 0])
    try:
        assert group.group_size() == 2
        a = single.ecdsa_verify(CD.define(single, spec), h, r, s, q)
        gid = CD.define(group, spec)
        assert gid == CD.define(group, spec)
        b = group.ecdsa_verify(gid, h, r, s, q)
        assert (a == b).all() and 0 < int(a.sum()) < len(a)
        xy1, inf1 = single.mul_fixed(CD.define(single, spec), r)
        xy2, inf2 = group.mul_fixed(gid, r)
        assert (xy1 == xy2).all() and (inf1 == inf2).all()
    finally:
        group.close()
        single.close()


def test_small_order_compares_x_mod_n(ctx):
    """floor(p / n) > 100: no Maxwell trick in the reference (base.js:33-40), the verdict is
    getX().umod(n) == r on the affine x.  n = 2^61 - 1 over secp192k1's curve and G (n need not be
    G's order): items built so that u1 + u2 = c (mod n) with Q = G and r = x(c G) mod n -- the
    verdict is 1 where the integer sum u1 + u2 is c itself -- against the C oracle"""
    import random
    from oracle import c_oracle
    spec = dict(_spec("secp192k1"))
    spec["n"] = "%x" % ((1 << 61) - 1)
    spec["name"] = "secp192k1_n61"
    n = (1 << 61) - 1
    cid = CD.define(ctx, spec)
    name = CD.oracle_name(spec)
    rnd = random.Random(61)
    m = 512
    cs = [rnd.randrange(1, n) for _ in range(m)]
    xy, _ = c_oracle.mul_mt(name, np.stack([CD.b32(c) for c in cs]), threads=8)
    g = np.concatenate([CD.b32(CD.I(spec["g"]["x"])), CD.b32(CD.I(spec["g"]["y"]))])
    h, r, s = [], [], []
    for i, c in enumerate(cs):
        ri = int.from_bytes(xy[i, :32].tobytes(), "big") % n or 1
        e = rnd.randrange(0, n)
        si = (e + ri) * pow(c, n - 2, n) % n or 1
        h.append(CD.b32(e << (256 - 61)))               # _truncateToN keeps the top 61 bits
        r.append(CD.b32(ri))
        s.append(CD.b32(si))
    h, r, s = np.stack(h), np.stack(r), np.stack(s)
    q = np.tile(g, (m, 1))
    ok = ctx.ecdsa_verify(cid, h, r, s, q)
    want = CD.oracle_verify(spec, h, r, s, q)
    assert (ok == want).all()
    assert 0 < int(ok.sum()) < m


def test_domain_comb_respects_comb_max_bytes(hs, monkeypatch):
    """ELLGPU_COMB_MAX_BYTES below the domain's 0.5 MB comb: k*G, mulAdd(G) and verify are refused
    with ELLGPU_E_NOMEM (the unsigned comb has no narrower form); the ladders still run"""
    monkeypatch.setenv("ELLGPU_COMB_MAX_BYTES", str(256 * 1024))
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        spec = _spec("secp192k1")
        cid = CD.define(c, spec)
        k = np.stack([CD.b32(5)])
        g = np.concatenate([CD.b32(CD.I(spec["g"]["x"])), CD.b32(CD.I(spec["g"]["y"]))])[None]
        for call in (lambda: c.mul_fixed(cid, k), lambda: c.mul_add2(cid, k, None, k, g),
                     lambda: c.ecdsa_verify(cid, np.zeros((1, 32), np.uint8), k, k, g)):
            with pytest.raises(_lib.EllgpuError) as e:
                call()
            assert e.value.code == -4
        xy, inf = c.mul_var(cid, k, g)
        assert not inf[0] and xy.any()
    finally:
        c.close()


@pytest.mark.parametrize("name", ["brainpoolP256r1"])
def test_domain_later_candidate_floor_one(ctx, name):
    """floor(p/n) = 1: an R whose x lies in [n, p), r = x - n, Q = r^-1 (s R - e G) -- eqXToP's
    second candidate r + n accepts it (the reference's verdict; the C oracle agrees), and the same
    item with r = x (out of range) is refused"""
    from oracle import c_oracle
    spec = _spec(name)
    p, a, b, n, gx, gy = CD.params(spec)
    assert p // n == 1 and p % 4 == 3
    oname = CD.oracle_name(spec)
    pts = []
    x = n
    while len(pts) < 4:
        v = (x * x * x + a * x + b) % p
        y = pow(v, (p + 1) // 4, p)
        if y * y % p == v:
            pts.append((x, y))
        x += 1
    h, r, s, q = [], [], [], []
    for j, (x, y) in enumerate(pts):
        ri = x - n
        si = 12345 + j
        e = (0xABCDEF << 200) + j
        z = e >> max(0, 256 - n.bit_length())
        z = z - n if z >= n else z
        rinv = pow(ri, n - 2, n)
        k1 = np.stack([CD.b32(si * rinv % n)])
        k2 = np.stack([CD.b32((-z) * rinv % n)])
        R = np.concatenate([CD.b32(x), CD.b32(y)])[None]
        G = np.concatenate([CD.b32(gx), CD.b32(gy)])[None]
        qq, inf = c_oracle.mul_add(oname, k1, R, k2, G)
        assert not inf[0]
        h.append(CD.b32(e))
        r.append(CD.b32(ri))
        s.append(CD.b32(si))
        q.append(qq[0])
    h, r, s, q = np.stack(h), np.stack(r), np.stack(s), np.stack(q)
    cid = CD.define(ctx, spec)
    ok = ctx.ecdsa_verify(cid, h, r, s, q)
    assert (ok == 1).all() and (CD.oracle_verify(spec, h, r, s, q) == 1).all()
