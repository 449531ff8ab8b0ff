"""Sums of many k * P terms on Edwards curves (ellgpu_ed_mul_sum) on the device: the reference's
recorded answers (tests/golden/ed_mul_sum.json) on all four curves through host memory and device
tensors, the Python-integer model of tests/ed_mul_sum_checks.py at shapes with one long sum, many
middling ones and thousands of two-term ones, a context whose slices hold 48 pairs, a non-default
stream, and the call in flight on one stream while other device-memory calls run on a second."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ed_mul_sum_checks as ES  # noqa: E402

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


@pytest.fixture(scope="module")
def cids(ctx):
    return {name: ES.curve_id(ctx, name) for name in ES.NAMES}


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("name", ES.NAMES)
def test_golden(ctx, cids, name):
    for shuffled in (False, True):
        for bt in ES.fixture_batches(name, shuffled):
            assert _same(ES.check(ctx, cids[name], bt, "host"), ES.check(ctx, cids[name], bt, "dev_torch"))


@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("name", ["ed25519", "curve1174"])
def test_shapes_match_model(ctx, cids, name, n, m):
    bt = ES.pool_batch(name, n, m)
    ES.check(ctx, cids[name], bt, "dev_torch")
    ES.check(ctx, cids[name], bt, "host")


@pytest.mark.parametrize("name", ["ed25519", "curve1174", "ed25519_by_hand"])
def test_slices_of_48_pairs(ctx48, name):
    """(2, 257): 129 pairs per sum, two slices of 48 and one of 33 whose last pair is a lone term;
    (3, 33) and (5, 96): whole sums, groups of two and of one"""
    cid = ES.curve_id(ctx48, name)
    for n, m in ((2, 257), (3, 33), (5, 96)):
        ES.check(ctx48, cid, ES.pool_batch(name, n, m, seed=3), "dev_torch")
    bt = ES.with_off_curve(name, ES.pool_batch(name, 2, 257, seed=3), [(1, 200)])
    ES.check(ctx48, cid, bt, "dev_torch")
    ES.check(ctx48, cid, bt, "host")


@pytest.mark.parametrize("name", ["ed25519", "e222"])
def test_off_curve_terms(ctx, cids, name):
    bt = ES.pool_batch(name, 65, 33)
    marked = ES.with_off_curve(name, bt, [(0, 0), (7, 16), (64, 32)])
    got = ES.check(ctx, cids[name], marked, "dev_torch")
    keep = np.ones(65, bool)
    keep[[0, 7, 64]] = False
    assert (got[0][keep] == bt.want_xy[keep]).all() and (got[1][keep] == bt.want_inf[keep]).all()
    assert not got[0][~keep].any() and (got[1][~keep] == 2).all()


def _dev(bt):
    import torch
    return torch.from_numpy(bt.k).cuda(), torch.from_numpy(bt.xy).cuda()


def _outs(n):
    import torch
    return (torch.full((n, 64), ES.FILL, dtype=torch.uint8, device="cuda"),
            torch.full((n,), ES.FILL, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("name", ["ed25519", "curve1174"])
def test_torch_tensors_on_a_non_default_stream(ctx, cids, name):
    import torch
    cid = cids[name]
    bt = ES.pool_batch(name, 65, 33)
    k, xy = _dev(bt)
    out = _outs(65)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = ctx.ed_mul_sum(cid, k, xy, out=out)
    s.synchronize()
    assert got[0] is out[0] and (out[0].cpu().numpy() == bt.want_xy).all() and (out[1].cpu().numpy() == bt.want_inf).all()
    with pytest.raises(ValueError):
        ctx.ed_mul_sum(cid, k, xy)                                       # device tensors need out=
    with pytest.raises(ValueError):
        ctx.ed_mul_sum(cid, k, xy[:, :32], out=out)
    from elliptic_amd import _lib
    with pytest.raises(_lib.EllgpuError) as e:
        ctx.ed_mul_sum(cid, k, xy, out=(xy.view(-1)[:65 * 64].view(65, 64), out[1]))
    assert e.value.code == -2 and "overlap" in str(e.value)


def test_in_flight_beside_other_device_calls(ctx, cids):
    """three rounds of ed_mul_sum on one stream while mul_var_dev and eddsa_verify_dev run on a second,
    no host synchronisation in between and one at the end: every output is that of the call issued
    alone (the model's bytes for the sums)"""
    import torch
    shapes = [("ed25519", 65, 33), ("ed25519", 1, 257), ("ed25519", 4099, 2)]
    sums = [(name, ES.pool_batch(name, n, m)) for name, n, m in shapes]
    sum_in = [_dev(bt) for _, bt in sums]
    # the other stream's work: k * P on the first terms of the 4099 sums, and EdDSA verifies of
    # garbage (32-byte messages, signatures and keys cut from the same bytes: verdicts 0 / 1 and
    # errors 0 / 1, whatever they are alone)
    bt = sums[2][1]
    n = bt.n
    k1 = torch.from_numpy(np.ascontiguousarray(bt.k[:, 0])).cuda()
    p1 = torch.from_numpy(np.ascontiguousarray(bt.xy[:, 0])).cuda()
    sig = torch.from_numpy(np.ascontiguousarray(bt.xy[:, 1])).cuda()
    pub = torch.from_numpy(np.ascontiguousarray(bt.k[:, 1])).cuda()

    def others(outs):
        ctx.mul_var_dev("ed25519", k1, p1, outs[0], outs[1])
        ctx.eddsa_verify_dev(k1, 32, sig, pub, outs[2], outs[3])

    def other_outs():
        fill = lambda: torch.full((n,), ES.FILL, dtype=torch.uint8, device="cuda")  # noqa: E731
        return _outs(n) + (fill(), fill())

    alone_other = other_outs()
    others(alone_other)
    alone_sum = []
    for (name, b), (k, xy) in zip(sums, sum_in):
        o = _outs(b.n)
        ctx.ed_mul_sum(cids[name], k, xy, out=o)
        alone_sum.append(o)
    torch.cuda.synchronize()
    for (name, b), o in zip(sums, alone_sum):
        assert (o[0].cpu().numpy() == b.want_xy).all() and (o[1].cpu().numpy() == b.want_inf).all(), name
    assert alone_other[1].cpu().numpy().max() <= 2 and alone_other[2].cpu().numpy().max() <= 1
    assert alone_other[3].cpu().numpy().max() <= 1

    # every round's result buffers are filled first, on the current stream, and the two side streams
    # wait for that once: a fill that is not ordered before the call on the side stream may land
    # after the call's results
    got_sum = [_outs(b.n) for rnd in range(3) for _, b in sums]
    got_other = [other_outs() for _ in got_sum]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    sa.wait_stream(torch.cuda.current_stream())
    sb.wait_stream(torch.cuda.current_stream())
    for i, (o, oo) in enumerate(zip(got_sum, got_other)):
        (name, b), (k, xy) = sums[i % len(sums)], sum_in[i % len(sums)]
        with torch.cuda.stream(sa):
            ctx.ed_mul_sum(cids[name], k, xy, out=o)
        with torch.cuda.stream(sb):
            others(oo)
    torch.cuda.synchronize()
    for i, o in enumerate(got_sum):
        want = alone_sum[i % len(sums)]
        assert torch.equal(o[0], want[0]) and torch.equal(o[1], want[1]), ("ed_mul_sum", i)
    for i, oo in enumerate(got_other):
        assert all(torch.equal(a, b) for a, b in zip(oo, alone_other)), ("other stream", i)
