"""The key side of user-defined Edwards curves on the MI355X: the reference's recorded answers
(tests/golden/custom_ed.json) through the host and the device-buffer forms, and one 4 099-item batch
per large curve checked at n = 1, 63, 64, 65, 257 and 4 099 -- a lone lane, the wave edge, a partial
workgroup, and a ragged tail across inversion groups, the shapes at which kernels of one item per
lane with one inversion per K items go wrong -- against edwards.js, base.js and key.js restated over
Python integers (tests/custom_ed_checks.py); ed25519's a and d written out by hand against the
preset's own pointFromY; ECDH symmetry through the engine alone."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elliptic_amd  # noqa: E402
import custom_ed_checks as CK  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 4099]


@pytest.fixture(scope="module")
def ctx():
    c = elliptic_amd.Context(0)          # raises if libellgpu.so or the GPU is missing
    yield c
    c.close()


@pytest.mark.parametrize("form", ["host", "dev_torch"])
@pytest.mark.parametrize("name", CK.BIG)
def test_golden_on_device(ctx, name, form):
    spec = CK.spec_of(name)
    seen = CK.check_golden(ctx, spec, form=form)
    assert {("validate", 0), ("validate", 1), ("validate", 2), ("validate", 3), ("derive", 0), ("derive", 1),
            ("derive_wire", 3), ("fromy", 2), ("fromx", 3 if spec["pmod4"] == 1 else 2)} <= seen


@pytest.mark.parametrize("form", ["host", "dev_torch"])
@pytest.mark.parametrize("name", CK.TOY)
def test_toy_exhaustive_on_device(ctx, name, form):
    spec = CK.spec_of(name)
    seen, dseen = CK.check_toy(ctx, spec, form)
    assert seen == ({0, 2, 3} if spec["pmod4"] == 1 else {0, 2}) and dseen == ({0, 2} if name == "p13_d4" else {0})


@pytest.fixture(scope="module", params=CK.BIG)
def batch(request):
    """one 4 099-item batch per curve and the model's answers, shared by every size"""
    spec = CK.spec_of(request.param)
    bt = CK.random_batch(spec, 4099, seed=sum(map(ord, request.param)))
    assert CK.model_meets_conditions(bt, 257) and CK.model_meets_conditions(bt, 4099)
    return spec, bt


@pytest.mark.parametrize("n", SIZES)
def test_random_batch_matches_model(ctx, batch, n):
    spec, bt = batch
    form, other = ("dev_torch", "host") if n in (64, 4099) else ("host", "dev_torch")
    cid = CK.define(ctx, spec)
    CK.check_batch(ctx, spec, bt, n, form, cid)
    if n in (65, 4099):
        CK.check_batch(ctx, spec, bt, n, other, cid)


def test_derive_wire_while_the_scratch_regrows():
    """one context, one curve, n = 3, 257, 3 through both forms, each against a context of its own"""
    spec = CK.spec_of("curve1174")
    bt = CK.random_batch(spec, 257, seed=sum(map(ord, "curve1174")), distinct=31)
    got = CK.check_derive_wire_regrow(lambda: elliptic_amd.Context(0), spec, bt["wire"]["comp"], ["host", "dev_torch"])
    assert len(got) == 6 and set(bt["wire"]["comp"]["st"].tolist()) == {0, 3}      # shared secrets, and keys that do not decode


def test_ed25519_by_hand_equals_the_preset(ctx):
    """a = -1 and d = -121665 / 121666 over 2^255 - 19 as a user-defined curve: pointFromY against
    ellgpu_decompress on ed25519, row for row"""
    p = (1 << 255) - 19
    d = -121665 * pow(121666, -1, p) % p
    cid = ctx.define_edwards(p, p - 1, d)
    rng = random.Random("custom-ed:ed25519-by-hand")
    ys = [0, 1, p - 1, 2, 4 * pow(5, -1, p) % p] + [rng.randrange(p) for _ in range(252)]
    odd = np.array([rng.getrandbits(1) for _ in ys], np.uint8)
    odd[:3] = [0, 1, 1]                       # y = 1 and y = -1 asked for an odd x: 'invalid point' before any root
    for form in ("host", "dev_torch"):
        xy, st = CK.run_decompress(ctx, cid, CK.rows(ys), odd, True, form)
        pxy, ok = ctx.decompress("ed25519", CK.rows(ys), odd)
        assert (ok == (st == 0)).all() and (xy == pxy).all()
        assert set(st.tolist()) == {0, 2, 3} and 0.3 * len(ys) < ok.sum() < 0.7 * len(ys)


@pytest.mark.parametrize("name", CK.BIG)
def test_ecdh_symmetry_on_device(ctx, name):
    CK.check_symmetry(ctx, CK.spec_of(name), 65, seed=3)
    CK.check_symmetry(ctx, CK.spec_of(name), 9, seed=4, form="dev_torch")
