"""Wire formats on user-defined short curves on the MI355X: the reference's recorded answers
(tests/golden/custom_wire.json) through the host and the device-buffer forms, and random pointFromX
and EC#verify(msg, der, key) batches at n = 1, 63, 64, 65, 257 and 4 099 -- a lone lane, the wave
edge, a partial workgroup, and a grid of many workgroups with a ragged tail, the shapes at which a
kernel of one item per lane goes wrong -- against pointFromX over Python integers, against
ellgpu_ecdsa_verify on the decoded rows and against the C oracle."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elliptic_amd  # noqa: E402
import custom_wire_checks as CW  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in CW.curves()]
ROOTS = ["brainpoolP256r1", "secp224k1", "plain_s3", "plain_s32", "p224_user"]      # s = 1, 2, 3, 32, 96
SIZES = [1, 63, 64, 65, 257, 4099]


@pytest.fixture(scope="module")
def ctx():
    c = elliptic_amd.Context(0)          # raises if libellgpu.so or the GPU is missing
    yield c
    c.close()


@pytest.mark.parametrize("form", ["host", "dev_torch"])
@pytest.mark.parametrize("name", NAMES)
def test_golden_on_device(ctx, name, form):
    spec = CW.spec_of(name)
    assert CW.check_decode_golden(ctx, spec, form=form) >= 50
    if CW.is_domain(spec):
        assert CW.check_wire_golden(ctx, spec, form=form) >= 57


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ROOTS)
def test_random_decompress_matches_model(ctx, name, n):
    spec = CW.spec_of(name)
    form = "dev_torch" if n in (64, 4099) else "host"
    good = CW.check_random_decompress(ctx, spec, n, seed=3000 + n, form=form)
    if n >= 257:
        assert 0.3 * n <= good <= 0.7 * n, good
    CW.check_random_decode(ctx, spec, n, seed=4000 + n, form="host" if form != "host" else "dev_torch")


@pytest.fixture(scope="module", params=["brainpoolP256r1", "secp224k1"])
def wire(request, ctx):
    """one 4 099-item batch per curve and its reference verdicts (raw-form verify on the device ==
    C oracle), shared by every size"""
    spec = CW.spec_of(request.param)
    batch = CW.wire_batch(spec, 4099, seed=sum(map(ord, request.param)))
    return spec, batch, CW.wire_reference(ctx, spec, batch)


@pytest.mark.parametrize("n", SIZES)
def test_random_wire_host(ctx, wire, n):
    spec, batch, want = wire
    CW.check_wire_batch(ctx, spec, batch, want, n)


@pytest.mark.parametrize("n", SIZES)
def test_random_wire_dev(ctx, wire, n):
    spec, batch, want = wire
    CW.check_wire_batch(ctx, spec, batch, want, n, form="dev_torch")


def test_random_wire_null_err(ctx, wire):
    spec, batch, want = wire
    CW.check_wire_batch(ctx, spec, batch, want, 4099, want_err=False)
    CW.check_wire_batch(ctx, spec, batch, want, 65, form="dev_torch", want_err=False)
