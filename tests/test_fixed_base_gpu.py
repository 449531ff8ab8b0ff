"""Fixed-base tables of caller-chosen points on the device: the reference's recorded answers
(tests/golden/fixed_base.json) through both memory kinds on every curve, one 4 099-item batch per
curve at the sizes where the forms change, the signed comb's widths, two widths in one call, and
the generator by coordinates and as an alias against ellgpu_mul_fixed / ellgpu_mul_add2."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fixed_base_checks as FB  # noqa: E402

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
        batches[name] = FB.random_batch(FB.spec_of(name), 4099, 2)
    return batches[name]


@pytest.mark.parametrize("name", FB.NAMES)
def test_model_meets_the_conditions(batches, name):
    """an infinity and a doubling-branch item among the first four rows, by construction (CPU)"""
    assert FB.model_meets_conditions(FB.spec_of(name), _batch(batches, name))


@pytest.mark.parametrize("name", FB.NAMES)
def test_golden(ctx, name):
    spec = FB.spec_of(name)
    a = FB.check_golden(ctx, spec, 8, "host")
    b = FB.check_golden(ctx, spec, 8, "dev_torch")
    assert all((u[0] == v[0]).all() and (u[1] == v[1]).all() for u, v in zip(a, b))


@pytest.mark.parametrize("name", FB.NAMES)
def test_batch_sizes(ctx, batches, name):
    """one batch, checked at n = 1 ... 4 099, the memory kinds alternating"""
    spec, bt = FB.spec_of(name), _batch(batches, name)
    _, hs = FB.define_bases(ctx, spec, 0)
    try:
        for j, n in enumerate(SIZES):
            FB.check_batch(ctx, spec, bt, n, hs, "dev_torch" if j & 1 else "host")
            if n == 65:
                FB.check_batch(ctx, spec, bt, n, hs, "host")
    finally:
        for h in hs:
            ctx.release_base(h)


@pytest.mark.parametrize("width", [4, 12, 16])
@pytest.mark.parametrize("name", FB.SIGNED)
def test_signed_widths(ctx, batches, name, width):
    spec, bt = FB.spec_of(name), _batch(batches, name)
    _, hs = FB.define_bases(ctx, spec, width)
    try:
        assert all(ctx.base_info(h)[1] == width for h in hs)
        FB.check_batch(ctx, spec, bt, 257, hs, "dev_torch")
        FB.check_batch(ctx, spec, bt, 65, hs, "host")
        FB.check_batch(ctx, spec, bt, 1, hs, "host")                 # the lanes-per-item form of mul_base
        FB.check_batch(ctx, spec, bt, 9, hs, "dev_torch")
    finally:
        for h in hs:
            ctx.release_base(h)


def test_device_operands_are_checked(ctx):
    import torch
    spec = FB.spec_of("p192")
    h = ctx.define_base("p192", FB.xy_bytes(FB.bases_of(spec)[0], 24))
    try:
        k = torch.ones((3, 24), dtype=torch.uint8, device="cuda")
        xy = torch.zeros((3, 48), dtype=torch.uint8, device="cuda")
        inf = torch.zeros(3, dtype=torch.uint8, device="cuda")
        for bad in (None, (xy,), (xy[:2], inf), (xy, inf.cpu()), (xy.to(torch.int32), inf)):
            with pytest.raises(ValueError):
                ctx.mul_base(h, k, out=bad)
            with pytest.raises(ValueError):
                ctx.mul_base2(h, h, k, k, out=bad)
        with pytest.raises(ValueError):
            ctx.mul_base(h, k[:, :23], out=(xy, inf))
        ctx.mul_base(h, k, out=(xy, inf))
    finally:
        ctx.release_base(h)


@pytest.mark.parametrize("name", FB.SIGNED)
def test_two_widths_in_one_call(ctx, batches, name):
    spec, bt = FB.spec_of(name), _batch(batches, name)
    pts, B = FB.bases_of(spec), spec["B"]
    h1 = ctx.define_base(name, FB.xy_bytes(pts[0], B), 12)
    h2 = ctx.define_base(name, FB.xy_bytes(pts[2], B), 4)
    try:
        for mem in ("host", "dev_torch"):
            xy, inf = FB.run_mul2(ctx, h1, h2, bt["k1"][:257], bt["k2"][:257], B, mem)
            assert (inf == bt["inf2"][:257]).all() and (xy == bt["xy2"][:257]).all()
    finally:
        ctx.release_base(h1)
        ctx.release_base(h2)


def test_generator_by_coordinates_equals_mul_fixed(ctx, batches):
    """secp256k1: G by coordinates at the width of the curve's own table, byte for byte, n = 4 099"""
    spec, bt = FB.spec_of("secp256k1"), _batch(batches, "secp256k1")
    want = ctx.mul_fixed("secp256k1", bt["k"])
    bits = ctx.comb_bits("secp256k1")
    assert bits in (4, 8, 12, 16, 22)
    h = ctx.define_base("secp256k1", FB.xy_bytes(FB.bases_of(spec)[0], 32), bits)
    try:
        assert ctx.base_info(h)[1] == bits
        for mem in ("host", "dev_torch"):
            xy, inf = FB.run_mul(ctx, h, bt["k"], 32, mem)
            assert (xy == want[0]).all() and (inf == want[1]).all()
    finally:
        ctx.release_base(h)


def test_alias_and_h_equals_mul_add2_on_a_domain(ctx, batches):
    """mul_base2(G alias, H) against mul_add2(k1, NULL -> G, k2, H) on brainpoolP256r1"""
    spec, bt = FB.spec_of("brainpoolP256r1"), _batch(batches, "brainpoolP256r1")
    cid = FB.curve_id(ctx, spec)
    H = FB.bases_of(spec)[3]
    g = ctx.define_base(cid)
    h = ctx.define_base(cid, FB.xy_bytes(H, 32))
    try:
        n = 257
        hxy = np.tile(np.frombuffer(FB.xy_bytes(H, 32), np.uint8), (n, 1))
        want = ctx.mul_add2(cid, bt["k1"][:n], None, bt["k2"][:n], hxy)
        for mem in ("host", "dev_torch"):
            xy, inf = FB.run_mul2(ctx, g, h, bt["k1"][:n], bt["k2"][:n], 32, mem)
            assert (xy == want[0]).all() and (inf == want[1]).all()
        fx = ctx.mul_fixed(cid, bt["k"][:n])
        xy, inf = FB.run_mul(ctx, g, bt["k"][:n], 32)
        assert (xy == fx[0]).all() and (inf == fx[1]).all()
    finally:
        ctx.release_base(h)
        ctx.release_base(g)


def test_small_order_base_is_refused(ctx):
    from elliptic_amd import _lib
    spec = FB.spec_of("cof_p10007")
    cid = FB.curve_id(ctx, spec)
    T = tuple(FB.I(v) for v in spec["refused"][0])
    with pytest.raises(_lib.EllgpuError) as e:
        ctx.define_base(cid, FB.xy_bytes(T, 32))
    assert e.value.code == -2 and "point at infinity" in str(e.value)
    with pytest.raises(_lib.EllgpuError) as e:
        ctx.define_base(cid, FB.xy_bytes((T[0], 1), 32))
    assert e.value.code == -2
