"""User-defined Montgomery curves on the MI355X: the reference's recorded answers
(tests/golden/custom_mont.json) through the host and the device-buffer forms, and one 4 099-item
batch per curve checked at n = 1, 63, 64, 65, 257 and 4 099 -- a lone lane, the wave edge, a partial
workgroup, and a grid of many workgroups with a ragged tail, the shapes at which a kernel of one
item per lane with one inversion per K items goes wrong -- against mont.js restated over Python
integers (tests/custom_mont_checks.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elliptic_amd  # noqa: E402
import custom_mont_checks as CM  # noqa: E402

pytestmark = pytest.mark.gpu

CURVES = [c["name"] for c in CM.curves()]
SIZES = [1, 63, 64, 65, 257, 4099]


@pytest.fixture(scope="module")
def ctx():
    c = elliptic_amd.Context(0)          # raises if libellgpu.so or the GPU is missing
    yield c
    c.close()


@pytest.mark.parametrize("form", ["host", "dev_torch"])
@pytest.mark.parametrize("name", CURVES)
def test_golden_on_device(ctx, name, form):
    spec = CM.spec_of(name)
    assert CM.check_golden(ctx, spec, form=form) == CM.statuses_of(spec)


@pytest.fixture(scope="module", params=CM.BIG)
def batch(request):
    """one 4 099-item batch per curve and the model's answers, shared by every size"""
    spec = CM.spec_of(request.param)
    bt = CM.random_batch(spec, 4099, seed=sum(map(ord, request.param)))
    assert CM.model_meets_conditions(bt, 257) and CM.model_meets_conditions(bt, 4099)
    return spec, bt


@pytest.mark.parametrize("n", SIZES)
def test_random_batch_matches_model(ctx, batch, n):
    spec, bt = batch
    form, other = ("dev_torch", "host") if n in (64, 4099) else ("host", "dev_torch")
    cid = CM.define(ctx, spec)
    CM.check_batch(ctx, spec, bt, n, form, cid)
    if n in (65, 4099):
        CM.check_batch(ctx, spec, bt, n, other, cid)


def test_c25519_user_equals_the_preset_on_device(ctx):
    """curve25519 written out by hand against the preset's ladder on the same rows, item for item"""
    spec = CM.spec_of("c25519_user")
    bt = CM.random_batch(spec, 257, seed=7)
    cid = CM.define(ctx, spec)
    for n in (65, 257):
        ox, inf = CM.run_ladder(ctx, cid, bt["k"][:n], bt["x"][:n])
        px, pinf = ctx.x25519(bt["k"][:n], bt["x"][:n])
        assert (ox == px).all() and (inf == pinf).all() and (ox == bt["ox"][:n]).all()
        dx, dst = CM.run_derive(ctx, cid, bt["k"][:n], bt["x"][:n])
        qx, qst = ctx.x25519_derive(bt["k"][:n], bt["x"][:n])
        assert (np.where(dst == 3, 1, dst) == qst).all() and (dx[dst == 0] == qx[dst == 0]).all()


def test_ecdh_symmetry_on_device(ctx, batch):
    """derive(a, x(b G)) = derive(b, x(a G)) through the engine alone"""
    spec, _ = batch
    CM.check_symmetry(ctx, spec, 65, seed=1, form="host")
    CM.check_symmetry(ctx, spec, 257, seed=2, form="dev_torch")
