"""ECDSA on user-defined Edwards domains (ellgpu_curve_define_edwards_domain, ellgpu_custom_ed_verify,
_custom_ed_sign, _custom_ed_sign_det) on the CPU: the hostsim build of the device code (tests/hostsim)
against the reference's recorded answers (tests/golden/custom_ed_ecdsa.json), against ec/index.js
restated over Python integers on the affine addition law (tests/custom_ed_ecdsa_checks.py) on random
batches, the definition's refusals, the refusal matrix in both directions, the plain Edwards block,
which the new calls must leave as it was, and the launches: no edc_mul_add2, one table of G."""
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
import custom_ed_ecdsa_checks as EC  # noqa: E402

SEED = {name: sum(map(ord, name)) for name in EC.DOMAINS}


@pytest.fixture(scope="module")
def hs():
    lib = _lib.load(build_hostsim(), optional=("ellgpu_probe_valu", "ellgpu_ctx_set_timing",
                                               "ellgpu_ctx_get_timing", "ellgpu_debug_field_op"))
    lib.hs_rt_block.restype = ctypes.c_int
    lib.hs_rt_block.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    lib.hs_launches.restype = ctypes.c_int
    lib.hs_launches.argtypes = [ctypes.c_char_p]
    return lib


@pytest.fixture(scope="module")
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


def _block(hs, ctx, cid):
    buf = np.zeros(4096, np.uint8)
    size = hs.hs_rt_block(ctx._ctx, cid, buf.ctypes.data, buf.size)
    assert 0 < size <= buf.size
    return buf[:size].tobytes()


def _code(call):
    with pytest.raises(_lib.EllgpuError) as e:
        call()
    return e.value.code


def I_ge_n(name):
    """the supplied-nonce cases hold a private key >= n"""
    spec = EC.spec_of(name)
    return any(EC.I(c["d"]) >= EC.params(spec)[3] for c in spec["sup"])


def test_domain_set():
    assert [c["name"] for c in EC.domains()] == EC.DOMAINS
    facts = {"curve1174": (4, 1), "e222": (4, 1), "ed25519_by_hand": (7, 1)}
    for name, (q, mx) in facts.items():
        spec = EC.spec_of(name)
        assert (int(spec["p_div_n"]), spec["maxwell"]) == (q, mx)
    toy = EC.spec_of("toy_p65521")
    p, a, d, n, gx, gy = EC.params(toy)
    assert p == 65521 and a == 1 and 257 <= n < p // 100 and n % 2 == 1 and toy["maxwell"] == 0 and toy["curve_order"] % n == 0
    assert all(n % f for f in range(3, int(n ** 0.5) + 1, 2))
    p, a = EC.params(EC.spec_of("ed25519_by_hand"))[:2]
    assert a == p - 1
    assert EC.params(EC.spec_of("e222"))[0].bit_length() == 222 and EC.spec_of("e222")["nbytes"] == 28
    for name in EC.DOMAINS:
        tags = {c["tag"]: c for c in EC.spec_of(name)["verify"]}
        assert tags["valid"]["ok"] == tags["j_0"]["ok"] == tags["j_1"]["ok"] == 1
        assert tags["msg_bits_short"]["ok"] == tags["msg_bits_long"]["ok"] == tags["digest_64"]["ok"] == 1
        for t in ("r_flipped", "s_flipped", "digest_flipped", "other_key", "r_0", "s_0", "r_n", "s_n", "p_is_identity",
                  "key_identity", "key_order_2"):
            assert tags[t]["ok"] == 0, (name, t)
        assert "ok" not in tags["off_curve"] and "r_n_minus_1" in tags
        sup = {c["tag"]: c for c in EC.spec_of(name)["sup"]}
        # (k = n - 1 and k = n are refused only where n fills its bytes: elsewhere _truncateToN shifts them into range)
        assert sup["k_0"]["ok"] == sup["k_1"]["ok"] == 0 and sup["k_2"]["ok"] == 1 and {"k_n_minus_1", "k_n"} <= set(sup)
        assert any(c["ok"] for c in sup.values()) and I_ge_n(name)
        if EC.spec_of(name)["nbytes"] < 32:                  # (a 32-byte n leaves no room for a wider nonce)
            assert "k_wider_than_n" in sup
        hashes = {c["hash"] for c in EC.spec_of(name)["det"]}
        assert hashes == {"sha256", "sha384", "sha512"}
        if name != "toy_p65521":
            assert {c["c"] for c in EC.spec_of(name)["det"]} == {0, 1}
        else:
            assert all("msg" in c for c in toy["det"])


@pytest.mark.parametrize("name", EC.DOMAINS)
def test_model_against_golden(name):
    tags = EC.check_model_against_golden(EC.spec_of(name))
    assert {"valid", "p_is_identity", "key_identity", "j_1", "k_n", "k_0"} <= tags


@pytest.mark.parametrize("form", ["host", "dev_np"])
@pytest.mark.parametrize("name", EC.DOMAINS)
def test_golden(ctx, name, form):
    spec = EC.spec_of(name)
    assert EC.check_golden(ctx, spec, form) == len(spec["verify"]) + len(spec["det"]) + len(spec["sup"])


@pytest.mark.parametrize("n", [65, 300])
@pytest.mark.parametrize("name", EC.DOMAINS)
def test_verify_batch_matches_model(ctx, name, n):
    spec = EC.spec_of(name)
    bt = EC.verify_batch(spec, n, SEED[name], distinct=min(n, 96))
    assert EC.verify_batch_meets_conditions(spec, bt)
    a = EC.check_verify_batch(ctx, spec, bt, n)
    b = EC.check_verify_batch(ctx, spec, bt, n, "dev_np")
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


@pytest.mark.parametrize("n", [65, 300])
@pytest.mark.parametrize("name", EC.DOMAINS)
def test_sign_batches_match_model(ctx, name, n):
    spec = EC.spec_of(name)
    cid = EC.define(ctx, spec)
    sup = EC.sup_batch(spec, n, SEED[name], 32, n & 1, distinct=48)
    a = EC.check_sup_batch(ctx, spec, sup, n, n & 1, cid=cid)
    b = EC.check_sup_batch(ctx, spec, sup, n, n & 1, form="dev_np", cid=cid)
    assert all((u == v).all() for u, v in zip(a, b)) and 0 < a[3].sum() < n
    if name == "toy_p65521":
        return
    hname = ("sha256", "sha384", "sha512")[SEED[name] % 3]
    det = EC.det_batch(spec, n, SEED[name], hname, 48 if n == 65 else 32, 1 - (n & 1), distinct=48)
    got = EC.check_det_batch(ctx, spec, det, n, hname, 1 - (n & 1), form="dev_np" if n == 65 else "host", cid=cid)
    if name == "ed25519_by_hand":
        assert (det["draws"] >= 2).mean() >= 0.2          # a 253-bit n in 32 bytes: about half the candidates are refused
    # the round trip through verify: Q = (priv mod n) G from the model.  Only what EC#sign made without
    # `canonical` verifies: on an Edwards curve -(x, y) = (-x, y), so (r, n - s) belongs to another x
    ok = EC.run_verify(ctx, cid, det["h"][:n], got[0], got[1], det["pub"][:n])[0]
    if 1 - (n & 1) == 0:
        assert (ok == 1).all()
    else:
        plain = EC.det_batch(spec, n, SEED[name], hname, 48 if n == 65 else 32, 0, distinct=48)
        low = (plain["s"][:n] == got[1]).all(axis=1)                   # s was low already
        assert (ok == low).all() and 0 < low.sum() < n


def test_definition(hs, ctx):
    spec = EC.spec_of("curve1174")
    p, a, d, n, gx, gy = EC.params(spec)
    dom = EC.define(ctx, spec)
    assert EC.define(ctx, spec) == dom                                    # the same seven values: the same id
    plain = ctx.define_edwards(p, a, d)
    assert plain != dom and ctx.define_edwards(p, a, d) == plain
    assert ctx.define_edwards_domain(p, a, d, n, p - gx, gy) not in (dom, plain)   # -G: another domain
    bad = [(n + 1, gx, gy), (1, gx, gy), (2, gx, gy), (0, gx, gy),          # n even, n < 3
           (n, gx, (gy + 1) % p), (n, gx + p, gy), (n, gx, gy + p), (n, p, 1), (n, 0, 1)]
    for nn, x, y in bad:
        assert _code(lambda: ctx.define_edwards_domain(p, a, d, nn, x, y)) == -2, (nn == n, x == gx, y == gy)
    assert _code(lambda: ctx.define_edwards_domain(p, a, a, n, gx, gy)) == -2                 # a = d: no curve
    assert ctx.define_edwards_domain(p, a, d, 3, 0, p - 1) > dom           # n * G = O is not tested, nor n's size
    # the domain's block: the plain curve's fields, then the domain's
    b_plain, b_dom = _block(hs, ctx, plain), _block(hs, ctx, dom)
    assert len(b_plain) == len(b_dom) and b_plain != b_dom


def test_plain_edwards_block_is_pinned(hs, ctx):
    """tests/golden/rt_blocks.json pins the plain definition's bytes; here: they do not move when the
    domain over the same (p, a, d) is defined and used"""
    spec = EC.spec_of("e222")
    p, a, d = EC.params(spec)[:3]
    plain = ctx.define_edwards(p, a, d)
    before = _block(hs, ctx, plain)
    dom = EC.define(ctx, spec)
    dom_before = _block(hs, ctx, dom)
    EC.check_golden(ctx, spec, cid=dom)
    assert _block(hs, ctx, plain) == before and _block(hs, ctx, dom) == dom_before
    assert ctx.define_edwards(p, a, d) == plain and EC.define(ctx, spec) == dom


def test_domain_id_is_a_plain_edwards_id_too(ctx):
    """every call that takes a plain Edwards id takes the domain id, with identical results"""
    name = "curve1174"
    spec, ks = EC.spec_of(name), CK.spec_of(name)
    dom, plain = EC.define(ctx, spec), CK.define(ctx, ks)
    bt = CK.random_batch(ks, 33, 5, distinct=33)
    a = CK.check_batch(ctx, ks, bt, 33, cid=dom)
    b = CK.check_batch(ctx, ks, bt, 33, cid=plain)
    assert all((u == v).all() for u, v in zip(a, b))
    CK.check_golden(ctx, ks, cid=dom)
    good = CK.xy_rows(bt["good"][:8])
    k1, k2 = bt["k"][:8], bt["k"][8:16]
    for cid in (dom, plain):
        r1 = ctx.mul_var(cid, k1, good)
        r2 = ctx.mul_add2(cid, k1, good, k2, good[::-1].copy())
        r3 = ctx.point_add(cid, good, good[::-1].copy())
        if cid == dom:
            first = (r1, r2, r3)
    for u, v in zip(first, (r1, r2, r3)):
        assert all((x == y).all() for x, y in zip(u, v))


def test_refusal_matrix(hs, ctx):
    spec = EC.spec_of("curve1174")
    p, a, d, n, gx, gy = EC.params(spec)
    dom = EC.define(ctx, spec)
    plain = ctx.define_edwards(p, a, d)
    short = ctx.define_short(p, a, 7)
    sdom = CE.define(ctx, CE.spec_of("brainpoolP256r1"))
    mont = ctx.define_mont(p, 486662)
    h = np.full((1, 32), 7, np.uint8)
    k = np.full((1, 32), 1, np.uint8)
    k[0, 31] = 9
    xy = CK.xy_rows([(gx, gy)])
    x = CK.rows([gx])
    odd = np.zeros(1, np.uint8)
    enc = np.concatenate([[4], xy[0]]).astype(np.uint8).reshape(1, -1)
    # the new calls on every other kind of id
    new_calls = [lambda c: ctx.custom_ed_verify(c, h, k, k, xy), lambda c: ctx.custom_ed_sign(c, h, k, k),
                 lambda c: ctx.custom_ed_sign_det(c, h, k)]
    for call in new_calls:
        call(dom)
        for cid in (plain, short, sdom, mont):
            assert _code(lambda: call(cid)) == -5
        for cid in (0, 3, 6, 7, 15, 32, 99, -1):
            assert _code(lambda: call(cid)) == -2
    # every older call that refuses a plain Edwards id refuses the domain id with the same code
    old_calls = [lambda c: ctx.custom_decompress(c, x, odd), lambda c: ctx.custom_decode_points(c, enc),
                 lambda c: ctx.custom_derive(c, k, xy), lambda c: ctx.custom_derive_wire(c, k, enc),
                 lambda c: ctx.custom_validate(c, xy, check_order=False), lambda c: ctx.custom_validate(c, xy, check_order=True),
                 lambda c: ctx.custom_mont_ladder(c, k, x), lambda c: ctx.custom_mont_validate(c, x),
                 lambda c: ctx.custom_mont_derive(c, k, x), lambda c: ctx.ecdsa_verify(c, h, k, k, xy),
                 lambda c: ctx.validate(c, xy), lambda c: ctx.encode_points(c, xy), lambda c: ctx.ecdh_derive(c, k, xy),
                 lambda c: ctx.decompress(c, x, odd), lambda c: ctx.mul_fixed(c, k), lambda c: ctx.mul_add2(c, k, None, k, xy),
                 lambda c: ctx.custom_sign(c, h, k, k), lambda c: ctx.custom_sign_det(c, h, k),
                 lambda c: ctx.custom_recover(c, h, k, k, odd), lambda c: ctx.custom_encode_points(c, xy),
                 lambda c: ctx.ecdsa_sign(c, h, k, k), lambda c: ctx.ecdsa_sign_det(c, h, k), lambda c: ctx.ecdsa_recover(c, h, k, k, odd)]
    for i, call in enumerate(old_calls):
        want = _code(lambda: call(plain))
        assert want in (-5, -2) and _code(lambda: call(dom)) == want, i
    P = lambda arr: arr.ctypes.data
    st = np.zeros(1, np.uint8)
    args = [P(h), 32, 0, P(xy), 64, None, P(xy), 33, P(st), P(st)]
    assert hs.ellgpu_custom_verify_wire(ctx._ctx, dom, 1, *args) == hs.ellgpu_custom_verify_wire(ctx._ctx, plain, 1, *args) == -5
    # arguments of the new calls
    for bad in (np.zeros((1, 0), np.uint8), np.zeros((1, 65), np.uint8)):
        assert _code(lambda: ctx.custom_ed_verify(dom, bad, k, k, xy)) == -2
        assert _code(lambda: ctx.custom_ed_sign(dom, bad, k, k)) == -2
        assert _code(lambda: ctx.custom_ed_sign_det(dom, bad, k)) == -2
    assert _code(lambda: ctx.custom_ed_sign_det(dom, h, k, drbg_hash=3)) == -2
    toy = EC.define(ctx, EC.spec_of("toy_p65521"))
    assert _code(lambda: ctx.custom_ed_sign_det(toy, h, k)) == -5          # n.byteLength() < 24
    assert ctx.custom_ed_sign(toy, h, k, k)[3][0] == 1
    ok = np.zeros(1, np.uint8)
    good = [P(h), 32, 0, P(k), P(k), P(xy), P(ok), None]
    for suffix, extra in (("", ()), ("_dev", (None,))):
        fn = getattr(hs, "ellgpu_custom_ed_verify" + suffix)
        assert fn(ctx._ctx, dom, 1, *good, *extra) == 0
        for j in (0, 3, 4, 5, 6):
            bad = list(good)
            bad[j] = None
            assert fn(ctx._ctx, dom, 1, *bad, *extra) == -2 and hs.ellgpu_last_error() == b"null pointer"
        assert fn(None, dom, 0, *good, *extra) == -2
    assert hs.ellgpu_version() == 0x000200


def test_empty_batch(ctx):
    dom = EC.define(ctx, EC.spec_of("e222"))
    e32, e64, eh = np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8), np.zeros((0, 32), np.uint8)
    ok, st = ctx.custom_ed_verify(dom, eh, e32, e32, e64, status=True)
    assert ok.shape == st.shape == (0,)
    assert ctx.custom_ed_sign(dom, eh, e32, e32)[3].shape == (0,)
    assert ctx.custom_ed_sign_det(dom, eh, e32)[3].shape == (0,)


def test_launches(hs):
    """a verify batch launches the shared-table ladder and no edc_mul_add2; G's table is built once
    per domain, whatever the number of calls; the scalar halves are the short domain's kernels"""
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        spec = EC.spec_of("curve1174")
        dom = EC.define(c, spec)
        bt = EC.verify_batch(spec, 65, SEED["curve1174"], distinct=65)
        hs.hs_launches_reset()
        EC.check_verify_batch(c, spec, bt, 65, cid=dom)
        EC.check_verify_batch(c, spec, bt, 9, cid=dom, form="dev_np")
        L = lambda name: hs.hs_launches(name.encode())
        assert L("edc_ecdsa_gtable") == 1 and L("edc_ecdsa_ladder") >= 2 and L("edc_ecdsa_eq") == L("edc_ecdsa_ladder")
        assert L("ecdsa_prep") == L("edc_ecdsa_ladder")
        assert L("edc_mul_add2") == L("edc_mul_var") == L("edc_ecdsa_eq_affine") == L("edc_key_front_xy") == 0
        sup = EC.sup_batch(spec, 9, 1, 32, 0, distinct=9)
        EC.check_sup_batch(c, spec, sup, 9, 0, cid=dom)
        assert L("edc_ecdsa_gtable") == 1 and L("edc_sign_mul") >= 1 and L("rt_sign_finish") == L("edc_sign_mul")
        assert L("rt_sign_mul") == L("comb_gen") == 0
        toy = EC.spec_of("toy_p65521")
        tid = EC.define(c, toy)
        EC.check_verify_batch(c, toy, EC.verify_batch(toy, 9, 2, distinct=9), 9, cid=tid)
        assert L("edc_ecdsa_gtable") == 2 and L("edc_ecdsa_eq_affine") >= 1
    finally:
        c.close()


def test_group_runs_on_its_first_member(hs, ctx):
    g = elliptic_amd.Context(lib_path=hs, devices=[0, 0])
    try:
        spec = EC.spec_of("ed25519_by_hand")
        gid = EC.define(g, spec)
        assert EC.define(g, spec) == gid
        EC.check_golden(g, spec, cid=gid)
    finally:
        g.close()
