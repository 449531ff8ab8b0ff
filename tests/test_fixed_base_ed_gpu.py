"""Fixed-base tables of caller-chosen points on Edwards curves, on the device: the reference's
recorded answers (tests/golden/fixed_base_ed.json), and per curve one 4 099-item batch whose answers
are the engine's own ellgpu_mul_var (the base tiled) and ellgpu_mul_add2, which ellgpu_mul_base and
ellgpu_mul_base2 must give byte for byte at n = 1 ... 4 099 through alternating memory kinds; the two
widths of a user-defined id, two widths in one call, and ed25519's generator as an alias and by
coordinates against ellgpu_mul_fixed."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fixed_base_checks as FB  # noqa: E402
import fixed_base_ed_checks as FE  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 257, 4099]


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import elliptic_amd
    c = elliptic_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batches():
    return {}


def _batch(batches, name):
    if name not in batches:
        batches[name] = FE.random_batch(FE.spec_of(name), 4099, 2)
    return batches[name]


@pytest.fixture(scope="module")
def answers(ctx, batches):
    """name -> (curve id, the batch through mul_var and mul_add2), computed once per curve"""
    made = {}

    def get(name):
        if name not in made:
            spec = FE.spec_of(name)
            cid = FE.curve_id(ctx, spec)
            made[name] = (cid, FE.variable_base_answers(ctx, cid, spec, _batch(batches, name)))
        return made[name]
    return get


@pytest.mark.parametrize("name", FE.NAMES)
def test_model_meets_the_conditions(batches, name):
    """an identity answer and a B1 = B2 item among the first four rows, by construction (CPU)"""
    assert FE.model_meets_conditions(FE.spec_of(name), _batch(batches, name))


@pytest.mark.parametrize("name", FE.NAMES)
def test_golden(ctx, name):
    spec = FE.spec_of(name)
    _, hs = FE.define_bases(ctx, spec)
    try:
        a = FE.check_golden(ctx, spec, hs, "host")
        b = FE.check_golden(ctx, spec, hs, "dev_torch")
        assert all((u[0] == v[0]).all() and (u[1] == v[1]).all() for u, v in zip(a, b))
    finally:
        FE.release(ctx, hs)


@pytest.mark.parametrize("name", FE.NAMES)
def test_batch_sizes(ctx, batches, answers, name):
    """one batch, checked at n = 1 ... 4 099, the memory kinds alternating"""
    spec, bt = FE.spec_of(name), _batch(batches, name)
    cid, want = answers(name)
    # (the rows by construction came out as the model says: the identity first)
    assert not want["xy"][0, :63].any() and want["xy"][0, 63] == 1 and not want["xy2"][0, :63].any() and want["xy2"][0, 63] == 1
    assert want["inf"][0] == want["inf2"][0] == (1 if spec["kind"] == "preset" else 0) and not want["inf"][2:].any()
    _, hs = FE.define_bases(ctx, spec, 0, cid, which=(0, 2, 3))
    try:
        for j, n in enumerate(SIZES):
            FE.check_batch(ctx, spec, bt, want, n, hs, "dev_torch" if j & 1 else "host")
            if n == 65:
                FE.check_batch(ctx, spec, bt, want, n, hs, "host")
    finally:
        FE.release(ctx, hs)


@pytest.mark.parametrize("width", [8, 16])
@pytest.mark.parametrize("name", ["curve1174", "e222"])
def test_widths(ctx, batches, answers, name, width):
    spec, bt = FE.spec_of(name), _batch(batches, name)
    cid, want = answers(name)
    _, hs = FE.define_bases(ctx, spec, width, cid, which=(0, 2, 3))
    try:
        entries = (256 // width) * ((1 << width) - 1)
        assert all(ctx.base_info(h) == (cid, width, (entries + 1) * 64) for h in hs.values())
        FE.check_batch(ctx, spec, bt, want, 257, hs, "dev_torch")
        FE.check_batch(ctx, spec, bt, want, 65, hs, "host")
    finally:
        FE.release(ctx, hs)


@pytest.mark.parametrize("name", ["curve1174", "e222"])
def test_two_widths_in_one_call(ctx, batches, answers, name):
    spec, bt = FE.spec_of(name), _batch(batches, name)
    cid, want = answers(name)
    pts = FE.bases_of(spec)
    h1 = ctx.define_ed_base(cid, FB.xy_bytes(pts[0], 32), 16)
    h2 = ctx.define_ed_base(cid, FB.xy_bytes(pts[2], 32), 8)
    try:
        assert ctx.base_info(h1)[1] == 16 and ctx.base_info(h2)[1] == 8
        for mem in ("host", "dev_torch"):
            xy, inf = FB.run_mul2(ctx, h1, h2, bt["k1"][:257], bt["k2"][:257], 32, mem)
            assert (inf == want["inf2"][:257]).all() and (xy == want["xy2"][:257]).all()
    finally:
        ctx.release_base(h1)
        ctx.release_base(h2)


def test_ed25519_alias_equals_mul_fixed(ctx, batches):
    """the NULL alias equals ellgpu_mul_fixed, and G by coordinates equals the alias, n = 4 099"""
    spec, bt = FE.spec_of("ed25519"), _batch(batches, "ed25519")
    want = ctx.mul_fixed("ed25519", bt["k"])
    alias = ctx.define_ed_base("ed25519")
    g = ctx.define_ed_base("ed25519", FB.xy_bytes(FE.bases_of(spec)[0], 32), 16)
    try:
        assert ctx.base_info(g)[1:] == ctx.base_info(alias)[1:] == (16, 16 * 65535 * 128)
        for h in (alias, g):
            for mem in ("host", "dev_torch"):
                xy, inf = FB.run_mul(ctx, h, bt["k"], 32, mem)
                assert (xy == want[0]).all() and (inf == want[1]).all()
        a = FB.run_mul2(ctx, alias, g, bt["k1"][:257], bt["k2"][:257], 32, "dev_torch")
        b = FB.run_mul2(ctx, g, alias, bt["k2"][:257], bt["k1"][:257], 32, "host")
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    finally:
        ctx.release_base(g)
        ctx.release_base(alias)


def test_device_operands_are_checked(ctx):
    import torch
    spec = FE.spec_of("e222")
    cid = FE.curve_id(ctx, spec)
    h = ctx.define_ed_base(cid, FB.xy_bytes(FE.bases_of(spec)[0], 32))
    try:
        k = torch.ones((3, 32), dtype=torch.uint8, device="cuda")
        xy = torch.zeros((3, 64), dtype=torch.uint8, device="cuda")
        inf = torch.zeros(3, dtype=torch.uint8, device="cuda")
        for bad in (None, (xy,), (xy[:2], inf), (xy, inf.cpu()), (xy.to(torch.int32), inf)):
            with pytest.raises(ValueError):
                ctx.mul_base(h, k, out=bad)
            with pytest.raises(ValueError):
                ctx.mul_base2(h, h, k, k, out=bad)
        with pytest.raises(ValueError):
            ctx.mul_base(h, k[:, :31], out=(xy, inf))
        ctx.mul_base(h, k, out=(xy, inf))
    finally:
        ctx.release_base(h)
