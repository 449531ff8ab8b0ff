"""EC#sign on user-defined ECDSA domains (ellgpu_custom_sign, ellgpu_custom_sign_det) on the CPU:
the Python-integer model against the reference's recorded answers (tests/golden/custom_sign.json),
then the hostsim build of the device code (tests/hostsim) against the same records and against the
model on random batches (tests/custom_sign_checks.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import custom_sign_checks as CS  # noqa: E402

DOMAINS = [c["name"] for c in CS.curves()]
# domain -> (hash, digest bytes, canonical): one hash per domain so that all three are used
RANDOM = {"brainpoolP256r1": ("sha256", 32, 1), "secp224k1": ("sha384", 48, 0), "w25519_like": ("sha512", 64, 1),
          "p224_user": ("sha256", 28, 0)}


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
    assert [CS.spec_of(n)["nbytes"] for n in DOMAINS] == [32, 24, 14, 29, 32, 28]
    assert CS.spec_of("secp224k1")["nbits"] == 225 and CS.spec_of("w25519_like")["nbits"] == 253


@pytest.mark.parametrize("name", DOMAINS)
def test_model_matches_the_reference(name):
    """the model alone, first: every recorded EC#sign answer, acceptance and thrown message"""
    spec = CS.spec_of(name)
    most = CS.check_model_against_golden(spec)
    kinds = {c["tag"] for c in spec["sup"]}
    assert {"k_0", "k_1", "k_2", "k_n_minus_2", "k_n_minus_1", "k_n", "k_zero_top_byte", "k_ordinary"} <= kinds
    assert ("k_wider_than_n" in kinds) == (spec["nbytes"] < 32)
    if spec["nbytes"] >= 24:
        assert {c["hash"] for c in spec["det"]} == set(CS.HASH_ID) and {c["c"] for c in spec["det"]} == {0, 1}
        assert {"short_digest", "digest_as_n", "digest_64", "msg_bits", "truncation_ge_n", "priv_one",
                "priv_n_minus_1", "priv_ge_n", "priv_32_bytes"} <= {c["tag"] for c in spec["det"]}
    else:
        assert all(c.get("msg") == CS.ENTROPY for c in spec["det"])
    if name in ("secp224k1", "w25519_like"):
        assert most >= 2                    # the reseed in front of a further draw is in the fixture


@pytest.mark.parametrize("form", ["host", "dev_np"])
@pytest.mark.parametrize("name", DOMAINS)
def test_golden(ctx, name, form):
    spec = CS.spec_of(name)
    assert CS.check_golden(ctx, spec, form) == len(spec["det"]) + len(spec["sup"])


@pytest.mark.parametrize("name", sorted(RANDOM))
def test_random_batches_match_model(ctx, name):
    spec = CS.spec_of(name)
    hname, hl, can = RANDOM[name]
    seed = sum(map(ord, name))
    cid = CS.define(ctx, spec)
    bt = CS.det_batch(spec, 300, seed, hname, hl, can)
    if name in ("secp224k1", "w25519_like"):
        assert (bt["draws"] >= 2).sum() >= 60
    assert bt["draws"].max() <= CS.MAX_DRAWS
    got = CS.check_det_batch(ctx, spec, bt, 300, hname, can, cid=cid)
    got2 = CS.check_det_batch(ctx, spec, bt, 300, hname, can, form="dev_np", cid=cid)
    assert all((a == b).all() for a, b in zip(got, got2))
    assert CS.check_round_trip(ctx, spec, bt, 300, got, cid=cid) == 300
    sb = CS.sup_batch(spec, 300, seed + 1, hl, 1 - can)
    got = CS.check_sup_batch(ctx, spec, sb, 300, 1 - can, cid=cid)
    assert 0.3 * 300 <= got[3].sum() <= 300 - 3 * (300 // 8)
    assert CS.check_round_trip(ctx, spec, sb, 300, got, cid=cid) == got[3].sum()


@pytest.mark.parametrize("n", [1, 8, 9, 41, 203])
def test_sizes(ctx, n):
    """the hostsim small-call and chunk edges, on the domain with n > p and 29-byte draws"""
    spec = CS.spec_of("secp224k1")
    cid = CS.define(ctx, spec)
    CS.check_det_batch(ctx, spec, CS.det_batch(spec, 203, 77, "sha512", 33, 1, bits=260), n, "sha512", 1, bits=260, cid=cid)
    CS.check_sup_batch(ctx, spec, CS.sup_batch(spec, 203, 78, 20, 0), n, 0, cid=cid)


def _code(call):
    with pytest.raises(_lib.EllgpuError) as e:
        call()
    return e.value.code


def test_refusals(hs, ctx):
    spec = CS.spec_of("brainpoolP256r1")
    p, a, b = CS.CD.params(spec)[:3]
    dom = CS.define(ctx, spec)
    small = CS.define(ctx, CS.spec_of("secp112r1"))
    plain = ctx.define_short(p, a, b)
    ed = ctx.define_edwards((1 << 255) - 19, -1 % ((1 << 255) - 19), 121665)
    h = np.full((1, 32), 7, np.uint8)
    d = np.full((1, 32), 1, np.uint8)
    assert ctx.custom_sign(dom, h, d, d)[3][0] == 1 and ctx.custom_sign_det(dom, h, d)[3][0] == 1
    # a plain id and an Edwards id: unsupported; a preset id and an unknown id: argument errors
    for cid, code in [(plain, -5), (ed, -5)] + [(c, -2) for c in (0, 3, 6, 7, 31, 99, -1)]:
        assert _code(lambda: ctx.custom_sign(cid, h, d, d)) == code
        assert _code(lambda: ctx.custom_sign_det(cid, h, d)) == code
    # hash_len 0 and 65, a drbg_hash that is none of the three
    for bad in (np.zeros((1, 0), np.uint8), np.zeros((1, 65), np.uint8)):
        assert _code(lambda: ctx.custom_sign(dom, bad, d, d)) == -2
        assert _code(lambda: ctx.custom_sign_det(dom, bad, d)) == -2
    assert ctx.custom_sign(dom, np.zeros((1, 64), np.uint8), d, d)[3][0] in (0, 1)
    for bad in (-1, 3, 256):
        assert _code(lambda: ctx.custom_sign_det(dom, h, d, drbg_hash=bad)) == -2
    # n.byteLength() < 24: EC#sign itself throws; one pass of its loop stays computable
    for hid in (0, 1, 2):
        assert _code(lambda: ctx.custom_sign_det(small, h, d, drbg_hash=hid)) == -5
    assert b"Not enough entropy" in hs.ellgpu_last_error()
    assert ctx.custom_sign(small, h, d, np.full((1, 32), 0, np.uint8) + np.eye(1, 32, 31, dtype=np.uint8) * 9)[3][0] == 1
    # NULL pointers, in the host and the _dev form; n = 0 reads and writes nothing
    P = lambda arr: arr.ctypes.data
    o = [np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8), np.zeros(1, np.uint8), np.zeros(1, np.uint8)]
    for suffix, extra in (("", ()), ("_dev", (None,))):
        for fn, mid in ((getattr(hs, "ellgpu_custom_sign" + suffix), [P(d), P(d), 0]),
                        (getattr(hs, "ellgpu_custom_sign_det" + suffix), [P(d), 0, 0])):
            good = [P(h), 32, 0] + mid + [P(x) for x in o]
            assert fn(ctx._ctx, dom, 1, *good, *extra) == 0
            for k in range(len(good)):
                if good[k] in (0, 32):
                    continue
                args = list(good)
                args[k] = None
                assert fn(ctx._ctx, dom, 1, *args, *extra) == -2
                assert hs.ellgpu_last_error() == b"null pointer"
            none = [None, 32, 0] + [None if isinstance(v, int) and v > 64 else v for v in mid] + [None] * 4
            assert fn(ctx._ctx, dom, 0, *none, *extra) == 0
            assert fn(None, dom, 0, *none, *extra) == -2
    # the preset-named entry points keep refusing user-defined ids
    for cid in (dom, plain):
        assert _code(lambda: ctx.ecdsa_sign(cid, h, d, d)) == -5
        assert _code(lambda: ctx.ecdsa_sign_det(cid, h, d)) == -5
    assert hs.ellgpu_version() == 0x000200


def test_group_runs_on_its_first_member(hs, ctx):
    g = elliptic_amd.Context(lib_path=hs, devices=[0, 0])
    try:
        spec = CS.spec_of("secp224k1")
        gid = CS.define(g, spec)
        assert CS.check_golden(g, spec, cid=gid) == len(spec["det"]) + len(spec["sup"])
        bt = CS.det_batch(spec, 203, 77, "sha512", 33, 1, bits=260)
        CS.check_det_batch(g, spec, bt, 41, "sha512", 1, bits=260, cid=gid)
    finally:
        g.close()
