"""The scalars of test_glv_split_bound.py (glv_split_vectors.py: the edges of secp256k1's GLV split)
through the device-pointer entry points on the GPU, at one batch size in each kernel form -- 64
(a wave per part), 4 608 + 1 (a lane per part) and 196 608 + 64 (the full grid, whose ladder runs
32 four-bit windows) -- byte for byte against the C oracle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elliptic_amd  # noqa: E402
import glv_split_vectors as GV  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [64, 4608 + 1, 196608 + 64]


@pytest.fixture(scope="module")
def ctx():
    c = elliptic_amd.Context(0)
    yield c
    c.close()


def batches(m, n):
    """row indices of the batches of n items that cover rows [0, m): the rows in order, cyclically,
    in as many batches as it takes (one, where n >= m)"""
    count = (m + n - 1) // n
    return [np.arange(b * n, (b + 1) * n) % m for b in range(count)]


@pytest.mark.parametrize("n", SIZES)
def test_mul_var_dev(ctx, n):
    import torch
    cs = GV.engine_cases()
    for rows in batches(cs["k"].shape[0], n):
        k, pts = (torch.from_numpy(np.ascontiguousarray(cs[x][rows])).cuda() for x in ("k", "pts"))
        xy = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
        inf = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        ctx.mul_var_dev("secp256k1", k, pts, xy, inf)
        ctx.synchronize()
        assert inf.cpu().numpy().tobytes() == cs["want_inf"][rows].tobytes()
        assert xy.cpu().numpy().tobytes() == cs["want_xy"][rows].tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_ecdsa_verify_dev(ctx, n):
    import torch
    cs = GV.engine_cases()
    for rows in batches(cs["z"].shape[0], n):
        z, r, s, pub = (torch.from_numpy(np.ascontiguousarray(cs[x][rows])).cuda() for x in ("z", "r", "s", "pub"))
        ok = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        ctx.ecdsa_verify_dev("secp256k1", z, r, s, pub, ok)
        ctx.synchronize()
        assert ok.cpu().numpy().tobytes() == cs["want_ok"][rows].tobytes()
