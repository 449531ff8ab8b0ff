"""EC#recoverPubKey on user-defined ECDSA domains on the MI355X: the reference's recorded answers
(tests/golden/custom_recover.json) through the host and the device-buffer forms, and random
batches at n = 1, 63, 64, 65, 257 and 4 099 -- a lone lane, the wave edge, a partial workgroup, and
a grid of many workgroups with a ragged tail, the shapes at which a kernel of one item per lane
with one inversion per K items goes wrong -- against recoverPubKey restated over Python integers
(tests/custom_recover_checks.py)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elliptic_amd  # noqa: E402
import custom_recover_checks as CR  # noqa: E402

pytestmark = pytest.mark.gpu

DOMAINS = [c["name"] for c in CR.curves()]
# n < p < 2n and p = 3 (mod 4); n > p with Tonelli-Shanks; cofactor 8; the deep Tonelli-Shanks schedule
RANDOM = {"brainpoolP256r1": 32, "secp224k1": 28, "w25519_like": 64, "p224_user": 33}      # digest bytes
SIZES = [1, 63, 64, 65, 257, 4099]


@pytest.fixture(scope="module")
def ctx():
    c = elliptic_amd.Context(0)          # raises if libellgpu.so or the GPU is missing
    yield c
    c.close()


@pytest.mark.parametrize("form", ["host", "dev_torch"])
@pytest.mark.parametrize("name", DOMAINS)
def test_golden_on_device(ctx, name, form):
    assert CR.check_golden(ctx, CR.spec_of(name), form=form) == {0, 1, 2, 3}


@pytest.fixture(scope="module", params=sorted(RANDOM))
def batch(request):
    """one 4 099-item batch per domain and the model's answers, shared by every size"""
    spec = CR.spec_of(request.param)
    return spec, CR.random_batch(spec, 4099, seed=sum(map(ord, request.param)), hash_len=RANDOM[request.param])


@pytest.mark.parametrize("n", SIZES)
def test_random_batch_matches_model(ctx, batch, n):
    spec, bt = batch
    CR.check_batch(ctx, spec, bt, n, form="dev_torch" if n in (64, 4099) else "host")
    if n in (65, 4099):
        CR.check_batch(ctx, spec, bt, n, form="host" if n == 4099 else "dev_torch")
