"""ECDH, key validation and SEC1 encoding on user-defined short-curve domains on the MI355X: the
reference's recorded answers (tests/golden/custom_ecdh.json) through the host and the device-buffer
forms, and random batches at n = 1, 63, 64, 65, 257 and 4 099 -- a lone lane, the wave edge, a
partial workgroup, and a grid of many workgroups with a ragged tail, the shapes at which a kernel of
one item per lane with one inversion per K items goes wrong -- against KeyPair#derive / #validate /
BasePoint#encode restated over Python integers (tests/custom_ecdh_checks.py)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elliptic_amd  # noqa: E402
import custom_ecdh_checks as CE  # noqa: E402

pytestmark = pytest.mark.gpu

DOMAINS = [c["name"] for c in CE.curves()]
# p = 3 (mod 4) with p > 2^255; n > p with Tonelli-Shanks; cofactor 8 with low-order points; the
# deep Tonelli-Shanks schedule
RANDOM = ["brainpoolP256r1", "secp224k1", "w25519_like", "p224_user"]
SIZES = [1, 63, 64, 65, 257, 4099]


@pytest.fixture(scope="module")
def ctx():
    c = elliptic_amd.Context(0)          # raises if libellgpu.so or the GPU is missing
    yield c
    c.close()


@pytest.mark.parametrize("form", ["host", "dev_torch"])
@pytest.mark.parametrize("name", DOMAINS)
def test_golden_on_device(ctx, name, form):
    seen = CE.check_golden(ctx, CE.spec_of(name), form=form)
    assert seen["derive"] == {0, 1, 2} and seen["wire"] == {0, 1, 2, 3}


@pytest.fixture(scope="module", params=RANDOM)
def batch(request):
    """one 4 099-item batch per domain and the model's answers, shared by every size"""
    spec = CE.spec_of(request.param)
    bt = CE.random_batch(spec, 4099, seed=sum(map(ord, request.param)))
    assert CE.model_meets_conditions(bt, 257) and CE.model_meets_conditions(bt, 4099)
    return spec, bt


@pytest.mark.parametrize("n", SIZES)
def test_random_batch_matches_model(ctx, batch, n):
    spec, bt = batch
    form, other = ("dev_torch", "host") if n in (64, 4099) else ("host", "dev_torch")
    cid = CE.define(ctx, spec)
    CE.check_batch(ctx, spec, bt, n, form, cid)
    CE.check_wire_batch(ctx, spec, bt, n, form, cid)
    CE.check_encode_batch(ctx, spec, bt, n, other, cid)
    if n in (65, 4099):
        CE.check_batch(ctx, spec, bt, n, other, cid)
        CE.check_wire_batch(ctx, spec, bt, n, other, cid)


def test_ecdh_symmetry_on_device(ctx, batch):
    """derive(a, b G) = derive(b, a G) through the engine alone"""
    spec, bt = batch
    CE.check_symmetry(ctx, spec, bt, 257, "host")
    CE.check_symmetry(ctx, spec, bt, 4099, "dev_torch")
