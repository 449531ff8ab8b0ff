"""ECDSA on user-defined Edwards domains on the MI355X: the reference's recorded answers
(tests/golden/custom_ed_ecdsa.json) through the host and the device-buffer forms, and per domain one
4 099-item batch -- a seeded permutation of at most 300 modelled tuples -- checked at n = 1, 63, 64,
65, 257 and 4 099: a lone lane, the wave edge, a partial workgroup, and a ragged tail across
inversion groups and workgroups that each stage G's table in LDS.  The model is ec/index.js over
Python integers on the affine addition law (tests/custom_ed_ecdsa_checks.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import custom_ed_ecdsa_checks as EC  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 4099]
SEED = {name: sum(map(ord, name)) for name in EC.DOMAINS}


@pytest.fixture(scope="module")
def ctx():
    c = elliptic_amd.Context(0)          # raises if libellgpu.so or the GPU is missing
    yield c
    c.close()


@pytest.mark.parametrize("form", ["host", "dev_torch"])
@pytest.mark.parametrize("name", EC.DOMAINS)
def test_golden_on_device(ctx, name, form):
    spec = EC.spec_of(name)
    EC.check_model_against_golden(spec)
    assert EC.check_golden(ctx, spec, form) == len(spec["verify"]) + len(spec["det"]) + len(spec["sup"])


@pytest.fixture(scope="module", params=EC.DOMAINS)
def batch(request):
    """one 4 099-item verify batch per domain and the model's answers, shared by every size; the
    conditions on it are asserted on the model alone, before the engine sees it"""
    spec = EC.spec_of(request.param)
    bt = EC.verify_batch(spec, 4099, SEED[request.param], distinct=288)
    assert EC.verify_batch_meets_conditions(spec, bt)
    return spec, bt


@pytest.mark.parametrize("n", SIZES)
def test_verify_batch_matches_model(ctx, batch, n):
    spec, bt = batch
    form, other = ("dev_torch", "host") if n in (64, 4099) else ("host", "dev_torch")
    cid = EC.define(ctx, spec)
    EC.check_verify_batch(ctx, spec, bt, n, form, cid)
    if n in (65, 4099):
        EC.check_verify_batch(ctx, spec, bt, n, other, cid)


@pytest.fixture(scope="module", params=EC.DOMAINS)
def sign_batches(request):
    """supplied-nonce and (where n.byteLength() >= 24) deterministic batches of 4 099 items"""
    name = request.param
    spec = EC.spec_of(name)
    sup = EC.sup_batch(spec, 4099, SEED[name], 32, 1, distinct=96)
    det = None
    if name != "toy_p65521":
        det = EC.det_batch(spec, 4099, SEED[name], "sha256", 32, 0, distinct=96)
        if name == "ed25519_by_hand":                   # a 253-bit n in 32 bytes
            assert (det["draws"] >= 2).mean() >= 0.2
        if name in ("curve1174", "ed25519_by_hand"):
            assert det["wrapped"].mean() >= 0.25
    return spec, sup, det


@pytest.mark.parametrize("n", SIZES)
def test_sign_batches_match_model(ctx, sign_batches, n):
    spec, sup, det = sign_batches
    form = "dev_torch" if n in (64, 4099) else "host"
    cid = EC.define(ctx, spec)
    EC.check_sup_batch(ctx, spec, sup, n, 1, form=form, cid=cid)
    if det is not None:
        EC.check_det_batch(ctx, spec, det, n, "sha256", 0, form=form, cid=cid)


@pytest.mark.parametrize("name", EC.BIG)
def test_round_trip(ctx, name):
    """257 signatures from custom_ed_sign_det through custom_ed_verify, with the keys the model made;
    sha384 and sha512 take their turn here"""
    spec = EC.spec_of(name)
    cid = EC.define(ctx, spec)
    hname = "sha384" if name == "e222" else "sha512"
    det = EC.det_batch(spec, 257, SEED[name] + 1, hname, 48, 0, distinct=64)
    got = EC.check_det_batch(ctx, spec, det, 257, hname, 0, form="dev_torch", cid=cid)
    ok, st = EC.run_verify(ctx, cid, det["h"], got[0], got[1], det["pub"], form="dev_torch")
    assert (ok == 1).all() and not st.any()
    bad = got[1].copy()
    bad[:, 31] ^= 1
    assert not EC.run_verify(ctx, cid, det["h"], got[0], bad, det["pub"])[0].any()


def _code(call):
    with pytest.raises(_lib.EllgpuError) as e:
        call()
    return e.value.code


def test_refusals(ctx):
    spec = EC.spec_of("curve1174")
    p, a, d, n, gx, gy = EC.params(spec)
    dom = EC.define(ctx, spec)
    assert EC.define(ctx, spec) == dom
    plain = ctx.define_edwards(p, a, d)
    short = ctx.define_short(p, a, 7)
    mont = ctx.define_mont(p, 486662)
    assert plain != dom
    h = np.full((1, 32), 7, np.uint8)
    k = np.full((1, 32), 9, np.uint8)
    xy = EC.xy_rows([(gx, gy)])
    for call in (lambda c: ctx.custom_ed_verify(c, h, k, k, xy), lambda c: ctx.custom_ed_sign(c, h, k, k),
                 lambda c: ctx.custom_ed_sign_det(c, h, k)):
        call(dom)
        for cid in (plain, short, mont):
            assert _code(lambda: call(cid)) == -5
        for cid in (0, 6, 7, 31, 99):
            assert _code(lambda: call(cid)) == -2
    for call in (lambda c: ctx.ecdsa_verify(c, h, k, k, xy), lambda c: ctx.mul_fixed(c, k), lambda c: ctx.mul_add2(c, k, None, k, xy),
                 lambda c: ctx.custom_sign(c, h, k, k), lambda c: ctx.custom_validate(c, xy, check_order=True)):
        assert _code(lambda: call(dom)) == _code(lambda: call(plain)) == -5
    for nn, x, y in ((n + 1, gx, gy), (1, gx, gy), (n, gx, (gy + 1) % p), (n, gx + p, gy), (n, 0, 1)):
        assert _code(lambda: ctx.define_edwards_domain(p, a, d, nn, x, y)) == -2
    assert _code(lambda: ctx.custom_ed_sign_det(EC.define(ctx, EC.spec_of("toy_p65521")), h, k)) == -5
    # the domain id is a plain Edwards id too: the same product from both
    r1, r2 = ctx.mul_var(dom, k, xy), ctx.mul_var(plain, k, xy)
    assert (r1[0] == r2[0]).all() and (r1[1] == r2[1]).all()
