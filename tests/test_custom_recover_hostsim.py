"""EC#recoverPubKey on user-defined ECDSA domains (ellgpu_custom_recover) on the CPU: the hostsim
build of the device code (tests/hostsim) against the reference's recorded answers
(tests/golden/custom_recover.json) and against recoverPubKey restated over Python integers on
random batches (tests/custom_recover_checks.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import custom_recover_checks as CR  # noqa: E402

DOMAINS = [c["name"] for c in CR.curves()]
HASH_LEN = {"brainpoolP256r1": 32, "secp192k1": 24, "secp112r1": 20, "secp224k1": 28, "w25519_like": 64,
            "p224_user": 33}


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
    shape = {}
    for name in DOMAINS:
        p, a, b, n = CR.CD.params(CR.spec_of(name))[:4]
        shape[name] = (n > p, p // n, p % 4)
    assert shape["secp224k1"][0] and shape["secp112r1"][0] and shape["w25519_like"][1] == 7
    assert shape["secp224k1"][2] == 1 and shape["p224_user"][2] == 1 and shape["brainpoolP256r1"][2] == 3


@pytest.mark.parametrize("form", ["host", "dev_np"])
@pytest.mark.parametrize("name", DOMAINS)
def test_golden(ctx, name, form):
    """every case the reference recorded: its own signatures under every j, the second candidate
    below and around p mod n, r around p where n > p, r / s out of range, e = 0, n, 64 bytes of
    ones and one byte, and the point at infinity"""
    assert CR.check_golden(ctx, CR.spec_of(name), form) == {0, 1, 2, 3}


@pytest.mark.parametrize("name", DOMAINS)
def test_random_batch_matches_model(ctx, name):
    spec = CR.spec_of(name)
    xy, st = CR.check_random(ctx, spec, 300, seed=sum(map(ord, name)), hash_len=HASH_LEN[name])
    xy2, st2 = CR.check_random(ctx, spec, 300, seed=sum(map(ord, name)), hash_len=HASH_LEN[name], form="dev_np")
    assert (xy == xy2).all() and (st == st2).all()


@pytest.mark.parametrize("n", [1, 8, 9, 41, 203])
def test_sizes(ctx, n):
    """the hostsim small-call and chunk edges, on the domain with n > p"""
    CR.check_random(ctx, CR.spec_of("secp224k1"), n, seed=40 + n, hash_len=1 + (n * 5) % 64)


def _code(call):
    with pytest.raises(_lib.EllgpuError) as e:
        call()
    return e.value.code


def test_refusals(hs, ctx):
    spec = CR.spec_of("brainpoolP256r1")
    p, a, b = CR.CD.params(spec)[:3]
    dom = CR.define(ctx, spec)
    plain = ctx.define_short(p, a, b)
    ed = ctx.define_edwards((1 << 255) - 19, -1 % ((1 << 255) - 19), 121665)
    h = np.zeros((1, 32), np.uint8)
    r = np.ones((1, 32), np.uint8)
    j = np.zeros(1, np.uint8)
    assert ctx.custom_recover(dom, h, r, r, j)[1][0] in (0, 2)
    # a plain id and an Edwards id: unsupported; a preset id and an unknown id: argument errors
    assert _code(lambda: ctx.custom_recover(plain, h, r, r, j)) == -5
    assert _code(lambda: ctx.custom_recover(ed, h, r, r, j)) == -5
    for cid in (0, 3, 6, 7, 31, 99, -1):
        assert _code(lambda: ctx.custom_recover(cid, h, r, r, j)) == -2
    # hash_len 0 and 65
    assert _code(lambda: ctx.custom_recover(dom, np.zeros((1, 0), np.uint8), r, r, j)) == -2
    assert _code(lambda: ctx.custom_recover(dom, np.zeros((1, 65), np.uint8), r, r, j)) == -2
    assert ctx.custom_recover(dom, np.zeros((1, 64), np.uint8), r, r, j)[1][0] in (0, 2)
    # NULL pointers, in the host and the _dev form; n = 0 reads and writes nothing
    P = lambda arr: arr.ctypes.data
    xy, st = np.zeros((1, 64), np.uint8), np.zeros(1, np.uint8)
    for suffix, extra in (("", ()), ("_dev", (None,))):
        fn = getattr(hs, "ellgpu_custom_recover" + suffix)
        good = [P(h), 32, P(r), P(r), P(j), P(xy), P(st)]
        assert fn(ctx._ctx, dom, 1, *good, *extra) == 0
        for k in (0, 2, 3, 4, 5, 6):
            args = list(good)
            args[k] = None
            assert fn(ctx._ctx, dom, 1, *args, *extra) == -2
            assert hs.ellgpu_last_error() == b"null pointer"
        assert fn(ctx._ctx, dom, 0, None, 32, None, None, None, None, None, *extra) == 0
        assert fn(ctx._ctx, dom, 1, *([P(h), 0] + good[2:]), *extra) == -2
        assert fn(None, dom, 0, None, 32, None, None, None, None, None, *extra) == -2
    # the preset-named entry point keeps refusing user-defined ids
    assert _code(lambda: ctx.ecdsa_recover(dom, h, r, r, j)) == -5
    assert _code(lambda: ctx.ecdsa_recover(plain, h, r, r, j)) == -5
    assert hs.ellgpu_version() == 0x000200


def test_group_runs_on_its_first_member(hs, ctx):
    g = elliptic_amd.Context(lib_path=hs, devices=[0, 0])
    try:
        for name in ("secp224k1", "w25519_like"):
            spec = CR.spec_of(name)
            gid = CR.define(g, spec)
            assert CR.check_golden(g, spec, cid=gid) == {0, 1, 2, 3}
            a = CR.check_random(g, spec, 41, seed=9, cid=gid)
            b = CR.check_random(ctx, spec, 41, seed=9)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    finally:
        g.close()
