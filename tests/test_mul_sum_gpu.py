"""Sums of many k * P terms (ellgpu_mul_sum) on the device: the reference's recorded answers
(tests/golden/mul_sum.json) on all eight curves through host memory and device tensors, the
Python-integer model of tests/mul_sum_checks.py at shapes with one long sum, many middling ones and
thousands of two-term ones, a context whose slices hold 48 pairs, a non-default stream, and the call
in flight on one stream while other device-memory calls run on a second."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mul_sum_checks as MS  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = [(1, 257), (65, 33), (4099, 2)]


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
def ctx48(ctx):
    """a second context, created under ELLGPU_SUM_SLICE=48 (read when a context is created)"""
    import elliptic_amd
    os.environ["ELLGPU_SUM_SLICE"] = "48"
    try:
        c = elliptic_amd.Context(0)
    finally:
        del os.environ["ELLGPU_SUM_SLICE"]
    yield c
    c.close()


@pytest.mark.parametrize("name", MS.NAMES)
def test_golden(ctx, name):
    cid = MS.curve_id(ctx, name)
    for shuffled in (False, True):
        for bt in MS.fixture_batches(name, shuffled):
            a = MS.check(ctx, cid, bt, "host")
            b = MS.check(ctx, cid, bt, "dev_torch")
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("name", ["secp256k1", "p256", "p521"])
def test_shapes_match_model(ctx, name, n, m):
    bt = MS.pool_batch(name, n, m)
    MS.check(ctx, name, bt, "dev_torch")
    MS.check(ctx, name, bt, "host")


@pytest.mark.parametrize("name", ["secp256k1", "p256", "p521", "brainpoolP256r1"])
def test_slices_of_48_pairs(ctx48, name):
    """(2, 257): 129 pairs per sum, two slices of 48 and one of 33 whose last pair is a lone term;
    (3, 33) and (5, 96): whole sums, groups of two and of one"""
    cid = MS.curve_id(ctx48, name)
    for n, m in ((2, 257), (3, 33), (5, 96)):
        MS.check(ctx48, cid, MS.pool_batch(name, n, m), "dev_torch")
    bt = MS.with_off_curve(name, MS.pool_batch(name, 2, 257), [(1, 200)])
    MS.check(ctx48, cid, bt, "dev_torch")
    MS.check(ctx48, cid, bt, "host")


def test_off_curve_terms(ctx):
    for name in ("secp256k1", "p384"):
        bt = MS.pool_batch(name, 65, 33)
        marked = MS.with_off_curve(name, bt, [(0, 0), (7, 16), (64, 32)])
        got = MS.check(ctx, name, marked, "dev_torch")
        keep = np.ones(65, bool)
        keep[[0, 7, 64]] = False
        assert (got[0][keep] == bt.want_xy[keep]).all() and (got[1][keep] == bt.want_inf[keep]).all()


def _dev(bt):
    import torch
    return torch.from_numpy(bt.k).cuda(), torch.from_numpy(bt.xy).cuda()


def _outs(n, B2):
    import torch
    return (torch.full((n, B2), MS.FILL, dtype=torch.uint8, device="cuda"),
            torch.full((n,), MS.FILL, dtype=torch.uint8, device="cuda"))


def test_torch_tensors_on_a_non_default_stream(ctx):
    import torch
    bt = MS.pool_batch("secp256k1", 65, 33)
    k, xy = _dev(bt)
    out = _outs(65, 64)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = ctx.mul_sum("secp256k1", k, xy, out=out)
    s.synchronize()
    assert got[0] is out[0] and (out[0].cpu().numpy() == bt.want_xy).all() and (out[1].cpu().numpy() == bt.want_inf).all()
    with pytest.raises(ValueError):
        ctx.mul_sum("secp256k1", k, xy)                                  # device tensors need out=
    with pytest.raises(ValueError):
        ctx.mul_sum("secp256k1", k, xy[:, :32], out=out)
    from elliptic_amd import _lib
    with pytest.raises(_lib.EllgpuError) as e:
        ctx.mul_sum("secp256k1", k, xy, out=(xy.view(-1)[:65 * 64].view(65, 64), out[1]))
    assert e.value.code == -2 and "overlap" in str(e.value)


def test_in_flight_beside_other_device_calls(ctx):
    """three rounds of mul_sum on one stream while mul_var_dev and ecdsa_verify_dev run on a second,
    no host synchronisation in between and one at the end: every output is that of the call issued
    alone (the model's bytes for the sums)"""
    import torch
    shapes = [("secp256k1", 65, 33), ("p256", 1, 257), ("secp256k1", 4099, 2)]
    sums = [(name, MS.pool_batch(name, n, m)) for name, n, m in shapes]
    sum_in = [_dev(bt) for _, bt in sums]
    # the other stream's work: k * P on the first terms of the 4099 sums, and verifies of garbage
    # signatures under those points as keys (verdicts 0 or 1: whatever they are alone)
    bt = sums[2][1]
    n = bt.n
    k1 = torch.from_numpy(np.ascontiguousarray(bt.k[:, 0])).cuda()
    p1 = torch.from_numpy(np.ascontiguousarray(bt.xy[:, 0])).cuda()
    r = torch.from_numpy(np.ascontiguousarray(bt.k[:, 1])).cuda()

    def others(outs):
        ctx.mul_var_dev("secp256k1", k1, p1, outs[0], outs[1])
        ctx.ecdsa_verify_dev("secp256k1", k1, r, r, p1, outs[2])

    def other_outs():
        return _outs(n, 64) + (torch.full((n,), MS.FILL, dtype=torch.uint8, device="cuda"),)

    alone_other = other_outs()
    others(alone_other)
    alone_sum = []
    for (name, b), (k, xy) in zip(sums, sum_in):
        o = _outs(b.n, b.want_xy.shape[1])
        ctx.mul_sum(name, k, xy, out=o)
        alone_sum.append(o)
    torch.cuda.synchronize()
    for (name, b), o in zip(sums, alone_sum):
        assert (o[0].cpu().numpy() == b.want_xy).all() and (o[1].cpu().numpy() == b.want_inf).all(), name
    assert alone_other[1].cpu().numpy().max() <= 2 and alone_other[2].cpu().numpy().max() <= 1

    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    got_sum, got_other = [], []
    for rnd in range(3):
        for (name, b), (k, xy) in zip(sums, sum_in):
            o = _outs(b.n, b.want_xy.shape[1])
            with torch.cuda.stream(sa):
                ctx.mul_sum(name, k, xy, out=o)
            got_sum.append(o)
            oo = other_outs()
            with torch.cuda.stream(sb):
                others(oo)
            got_other.append(oo)
    torch.cuda.synchronize()
    for i, o in enumerate(got_sum):
        want = alone_sum[i % len(sums)]
        assert torch.equal(o[0], want[0]) and torch.equal(o[1], want[1]), ("mul_sum", i)
    for i, oo in enumerate(got_other):
        assert all(torch.equal(a, b) for a, b in zip(oo, alone_other)), ("other stream", i)
