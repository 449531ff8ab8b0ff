"""EC#sign on user-defined ECDSA domains on the MI355X: the reference's recorded answers
(tests/golden/custom_sign.json) through the host and the device-buffer forms, random batches at
n = 1, 63, 64, 65, 257 and 4 099 -- a lone lane, the wave edge, a partial workgroup, and a grid of
many workgroups with a ragged tail, the shapes at which a kernel of one item per lane with one
inversion per K items goes wrong -- against EC#sign restated over Python integers
(tests/custom_sign_checks.py), the round trip through the domain's verify and recovery, and the
argument and refusal pins."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import custom_sign_checks as CS  # noqa: E402

pytestmark = pytest.mark.gpu

DOMAINS = [c["name"] for c in CS.curves()]
# domain -> (hash, digest bytes, canonical).  secp224k1: n > p, 29-byte draws shifted by 7, about
# half of them out of range; w25519_like: cofactor 8, a 253-bit n, x mod n several-fold
RANDOM = {"brainpoolP256r1": ("sha256", 32, 1), "secp224k1": ("sha384", 48, 0), "w25519_like": ("sha512", 64, 1),
          "p224_user": ("sha256", 28, 0)}
SIZES = [1, 63, 64, 65, 257, 4099]


@pytest.fixture(scope="module")
def ctx():
    c = elliptic_amd.Context(0)          # raises if libellgpu.so or the GPU is missing
    yield c
    c.close()


@pytest.mark.parametrize("name", DOMAINS)
def test_golden_on_device(ctx, name):
    spec = CS.spec_of(name)
    CS.check_model_against_golden(spec)
    cid = CS.define(ctx, spec)
    for form in ("host", "dev_torch"):
        assert CS.check_golden(ctx, spec, form=form, cid=cid) == len(spec["det"]) + len(spec["sup"])


@pytest.fixture(scope="module", params=sorted(RANDOM))
def batch(request, ctx):
    """one 4 099-item batch per domain and call with the model's answers, shared by every size"""
    name = request.param
    spec = CS.spec_of(name)
    hname, hl, can = RANDOM[name]
    seed = sum(map(ord, name))
    det = CS.det_batch(spec, 4099, seed, hname, hl, can)
    sup = CS.sup_batch(spec, 4099, seed + 1, hl, 1 - can)
    return spec, CS.define(ctx, spec), det, sup


@pytest.mark.parametrize("n", SIZES)
def test_random_batch_matches_model(ctx, batch, n):
    spec, cid, det, sup = batch
    hname, hl, can = RANDOM[spec["name"]]
    if spec["name"] in ("secp224k1", "w25519_like") and n >= 63:
        assert (det["draws"][:n] >= 2).sum() >= n // 5
    assert det["draws"].max() <= CS.MAX_DRAWS
    form = "dev_torch" if n in (64, 4099) else "host"
    CS.check_det_batch(ctx, spec, det, n, hname, can, form=form, cid=cid)
    CS.check_sup_batch(ctx, spec, sup, n, 1 - can, form=form, cid=cid)
    if n in (65, 4099):
        other = "host" if n == 4099 else "dev_torch"
        CS.check_det_batch(ctx, spec, det, n, hname, can, form=other, cid=cid)
        CS.check_sup_batch(ctx, spec, sup, n, 1 - can, form=other, cid=cid)


def test_round_trip_on_device(ctx, batch):
    spec, cid, det, sup = batch
    hname, hl, can = RANDOM[spec["name"]]
    n = 257
    got = CS.check_det_batch(ctx, spec, det, n, hname, can, cid=cid)
    assert CS.check_round_trip(ctx, spec, det, n, got, cid=cid) == n
    got = CS.check_sup_batch(ctx, spec, sup, n, 1 - can, cid=cid)
    assert CS.check_round_trip(ctx, spec, sup, n, got, cid=cid) == got[3].sum() >= n // 4


def _code(call):
    with pytest.raises(_lib.EllgpuError) as e:
        call()
    return e.value.code


def test_refusals_on_device(ctx):
    spec = CS.spec_of("brainpoolP256r1")
    p, a, b = CS.CD.params(spec)[:3]
    dom = CS.define(ctx, spec)
    small = CS.define(ctx, CS.spec_of("secp112r1"))
    plain = ctx.define_short(p, a, b)
    ed = ctx.define_edwards((1 << 255) - 19, -1 % ((1 << 255) - 19), 121665)
    h = np.full((1, 32), 7, np.uint8)
    d = np.full((1, 32), 1, np.uint8)
    for cid, code in [(plain, -5), (ed, -5), (0, -2), (3, -2)]:
        assert _code(lambda: ctx.custom_sign(cid, h, d, d)) == code
        assert _code(lambda: ctx.custom_sign_det(cid, h, d)) == code
    for bad in (np.zeros((1, 0), np.uint8), np.zeros((1, 65), np.uint8)):
        assert _code(lambda: ctx.custom_sign(dom, bad, d, d)) == -2
        assert _code(lambda: ctx.custom_sign_det(dom, bad, d)) == -2
    assert _code(lambda: ctx.custom_sign_det(dom, h, d, drbg_hash=3)) == -2
    assert _code(lambda: ctx.custom_sign_det(small, h, d)) == -5
    nine = np.zeros((1, 32), np.uint8)
    nine[0, 31] = 9
    assert ctx.custom_sign(small, h, d, nine)[3][0] == 1
    assert _code(lambda: ctx.ecdsa_sign(dom, h, d, d)) == -5
    assert _code(lambda: ctx.ecdsa_sign_det(dom, h, d)) == -5
    empty = np.zeros((0, 32), np.uint8)
    assert ctx.custom_sign(dom, empty, empty, empty)[3].shape == (0,)
    assert ctx.custom_sign_det(dom, empty, empty)[3].shape == (0,)
