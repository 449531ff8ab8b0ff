"""ECDSA on user-defined domains (ellgpu_curve_define_short_domain) on the MI355X: the reference's
recorded verdicts and points (tests/golden/custom_ecdsa.json), a 2^18-item brainpoolP256r1 verify
batch through the host and the device-buffer forms, and k*G against k*G by the variable-base
ladder at 2^18."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elliptic_amd  # noqa: E402
import custom_domain_checks as CD  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in CD.curves()]
BIG = 1 << 18


@pytest.fixture(scope="module")
def ctx():
    c = elliptic_amd.Context(0)          # raises if libellgpu.so or the GPU is missing
    yield c
    c.close()


def _spec(name):
    return next(c for c in CD.curves() if c["name"] == name)


@pytest.mark.parametrize("name", NAMES)
def test_domain_golden_on_device(ctx, name):
    spec = _spec(name)
    assert CD.check_verify_golden(ctx, spec) >= 38
    assert CD.check_points_golden(ctx, spec) == 32


@pytest.fixture(scope="module")
def brainpool_batch():
    """2^16 distinct items (half valid signatures, the rest disturbed), repeated four times to
    2^18 with each copy shifted by one item; expected verdicts: 1 by construction for the valid
    ones, the C oracle's for the disturbed"""
    spec = _spec("brainpoolP256r1")
    u = 1 << 16
    h, r, s, q, expect = CD.random_batch(spec, u, seed=2018)
    want = CD.oracle_verify(spec, h, r, s, q)
    known = np.array([e is not None for e in expect])
    assert (want[known] == 1).all()
    idx = np.concatenate([np.roll(np.arange(u), j) for j in range(BIG // u)])
    return spec, h[idx], r[idx], s[idx], q[idx], want[idx]


def test_brainpool_2e18_verify_host(ctx, brainpool_batch):
    spec, h, r, s, q, want = brainpool_batch
    cid = CD.define(ctx, spec)
    ok, st = ctx.ecdsa_verify(cid, h, r, s, q, status=True)
    assert not st.any()
    assert (ok == want).all(), np.nonzero(ok != want)[0][:10]
    # and 10 240 items straight against the C oracle
    sel = slice(BIG - 10240, BIG)
    assert (ok[sel] == CD.oracle_verify(spec, h[sel], r[sel], s[sel], q[sel])).all()
    assert 0.3 < ok.mean() < 0.7


def test_brainpool_2e18_verify_dev(ctx, brainpool_batch):
    import torch
    spec, h, r, s, q, want = brainpool_batch
    cid = CD.define(ctx, spec)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dh, dr, ds, dq = dev(h), dev(r), dev(s), dev(q)
    ok = torch.full((BIG,), 7, dtype=torch.uint8, device="cuda")
    st = torch.full((BIG,), 7, dtype=torch.uint8, device="cuda")
    ctx.ecdsa_verify_dev(cid, dh, dr, ds, dq, ok, out_status=st)
    torch.cuda.synchronize()
    ok = ok.cpu().numpy()
    assert not st.cpu().numpy().any()
    assert (ok == want).all(), np.nonzero(ok != want)[0][:10]


def test_brainpool_2e18_mul_fixed_matches_mul_var(ctx):
    """k*G through the domain's comb equals k*G through the variable-base ladder, for 2^18 random
    32-byte k (not reduced mod n), and a slice equals the C oracle"""
    from oracle import c_oracle
    spec = _spec("brainpoolP256r1")
    cid = CD.define(ctx, spec)
    rng = np.random.default_rng(18)
    k = rng.integers(0, 256, size=(BIG, 32), dtype=np.uint8)
    k[:4] = 0
    k[1, 31] = 1
    k[2] = CD.b32(CD.I(spec["n"]))
    k[3] = 0xFF
    g = np.concatenate([CD.b32(CD.I(spec["g"]["x"])), CD.b32(CD.I(spec["g"]["y"]))])
    a, ia = ctx.mul_fixed(cid, k)
    b, ib = ctx.mul_var(cid, k, np.tile(g, (BIG, 1)))
    assert (ia == ib).all() and (a == b).all()
    assert ia[0] == 1 and ia[2] == 1 and not ia[3:].any()
    sel = slice(0, 4096)
    want, winf = c_oracle.mul_mt(CD.oracle_name(spec), k[sel], threads=8)
    assert (a[sel] == want).all() and (ia[sel] == winf).all()
