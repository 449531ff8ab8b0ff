"""secp256k1 verify and P*k on the GPU over the group law whose Y3 is one folded difference of two wide
products (FpK256::mul_sub_sqr in the doubling; mul_sub_mul in the mixed addition where
ELL_K256_PAIR_MADD compiles it in), byte for byte against the C oracle at one batch size in each
kernel form: 64 (row / parted), 4 608 + 1 (small grid) and 196 608 + 64 (the smallest batch that runs
the full-grid kernel).  The inputs are the exceptional-key
tuples of parity_checks.check_exceptional_keys -- recorded from that function itself by handing it a
context that answers with the oracle -- and the edge scalars of glv_split_vectors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elliptic_amd  # noqa: E402
import glv_split_vectors as GV  # noqa: E402
import parity_checks as PC  # noqa: E402

pytestmark = pytest.mark.gpu

CURVE = "secp256k1"
SIZES = [64, 4608 + 1, 196608 + 64]


class Recorder:
    """stands in for a context in check_exceptional_keys: keeps the operands it is asked about and
    answers with the C oracle, so that the function's own assertions hold and its vectors are kept"""

    def __init__(self):
        self.mul_add = None
        self.verify = None

    def mul_add2(self, curve, k1, p1, k2, p2):
        from oracle import c_oracle
        xy, inf = c_oracle.mul_add(curve, k1, p1, k2, p2)
        if p1 is None:
            self.mul_add = (k1, k2, p2, xy, np.asarray(inf, np.uint8))
        return xy, inf

    def ecdsa_verify(self, curve, z, r, s, pub):
        from oracle import c_oracle
        ok = np.asarray(c_oracle.verify(curve, z, r, s, pub), np.uint8)
        self.verify = (z, r, s, pub, ok)
        return ok


_cases = None


def cases():
    """inputs and the oracle's results, computed once and left unchanged"""
    global _cases
    if _cases is not None:
        return _cases
    from oracle import c_oracle
    rec = Recorder()
    assert PC.check_exceptional_keys(rec, CURVE) > 400
    gv = GV.engine_cases()
    ez, er, es, epub, eok = rec.verify
    _, k2, keys, _, _ = rec.mul_add
    kxy, kinf = c_oracle.mul(CURVE, k2, keys)                 # P*k over the exceptional keys: k2 Q
    cat = lambda *a: np.ascontiguousarray(np.concatenate(a))
    _cases = dict(z=cat(ez, gv["z"]), r=cat(er, gv["r"]), s=cat(es, gv["s"]), pub=cat(epub, gv["pub"]),
                  want_ok=cat(eok, gv["want_ok"]),
                  k=cat(k2, gv["k"]), pts=cat(keys, gv["pts"]), want_xy=cat(kxy, gv["want_xy"]),
                  want_inf=cat(np.asarray(kinf, np.uint8), gv["want_inf"]))
    assert 0 < int(_cases["want_ok"].sum()) < len(_cases["want_ok"])
    return _cases


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
def test_ecdsa_verify_dev(ctx, n):
    import torch
    cs = cases()
    for rows in batches(cs["z"].shape[0], n):
        z, r, s, pub = (torch.from_numpy(np.ascontiguousarray(cs[x][rows])).cuda() for x in ("z", "r", "s", "pub"))
        ok = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        ctx.ecdsa_verify_dev(CURVE, z, r, s, pub, ok)
        ctx.synchronize()
        assert ok.cpu().numpy().tobytes() == cs["want_ok"][rows].tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_mul_var_dev(ctx, n):
    import torch
    cs = cases()
    for rows in batches(cs["k"].shape[0], n):
        k, pts = (torch.from_numpy(np.ascontiguousarray(cs[x][rows])).cuda() for x in ("k", "pts"))
        xy = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
        inf = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        ctx.mul_var_dev(CURVE, k, pts, xy, inf)
        ctx.synchronize()
        assert inf.cpu().numpy().tobytes() == cs["want_inf"][rows].tobytes()
        assert xy.cpu().numpy().tobytes() == cs["want_xy"][rows].tobytes()
