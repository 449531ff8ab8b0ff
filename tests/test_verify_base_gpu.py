"""ECDSA verification against a fixed-base table of the signer's key, on the device: the reference's
recorded verdicts (tests/golden/verify_base.json), and per curve one 4 099-item batch whose expected
verdicts are the engine's own ellgpu_ecdsa_verify with the key repeated per item (held to the
Python-integer model on its first 64 rows), which ellgpu_ecdsa_verify_base must give byte for byte at
n = 1 ... 4 099 through alternating memory kinds; two widths of the key's table beside G's own, the
generator alias as a key, and the checks of device operands."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import verify_base_checks as VB  # noqa: E402

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
def cids(ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = VB.curve_id(ctx, VB.spec_of(name))
        return made[name]
    return get


@pytest.fixture(scope="module")
def batches():
    return {}


def _batch(batches, name, key=3):
    if (name, key) not in batches:
        batches[(name, key)] = VB.random_batch(VB.spec_of(name), 4099, 2, key=key, model=False)
    return batches[(name, key)]


@pytest.fixture(scope="module")
def answers(ctx, cids, batches):
    """(name, key) -> the batch through ellgpu_ecdsa_verify with the key tiled, computed once"""
    made = {}

    def get(name, key=3):
        if (name, key) not in made:
            bt = _batch(batches, name, key)
            want = VB.tiled_verify(ctx, cids(name), bt, 4099)
            assert (want[:64] == bt["want"]).all() and set(want.tolist()) == {0, 1}
            made[(name, key)] = want
        return made[(name, key)]
    return get


@pytest.mark.parametrize("name", VB.NAMES)
def test_batch_meets_the_conditions(batches, name):
    """both verdicts, u1 = 0, R = O and an out-of-range r among the first rows, by construction (CPU)"""
    assert VB.batch_meets_conditions(VB.spec_of(name), _batch(batches, name))


@pytest.mark.parametrize("name", VB.NAMES)
def test_golden(ctx, cids, name):
    spec = VB.spec_of(name)
    _, hs = VB.define_keys(ctx, spec, 0, cids(name))
    try:
        a = VB.check_golden(ctx, spec, hs, "host")
        b = VB.check_golden(ctx, spec, hs, "dev_torch")
        assert all((u == v).all() for u, v in zip(a, b))
    finally:
        for h in hs:
            ctx.release_base(h)


@pytest.mark.parametrize("name", VB.NAMES)
def test_batch_sizes(ctx, cids, batches, answers, name):
    """one batch, checked at n = 1 ... 4 099, the memory kinds alternating"""
    bt, want = _batch(batches, name), answers(name)
    h = ctx.define_base(cids(name), bt["pub"].tobytes())
    try:
        for j, n in enumerate(SIZES):
            for mem in (("dev_torch" if j & 1 else "host"),) + (("host",) if n == 65 else ()):
                ok = VB.run_verify(ctx, h, bt["h"][:n], bt["r"][:n], bt["s"][:n], 0, mem)
                assert ok.tobytes() == want[:n].tobytes(), (name, n, mem, np.flatnonzero(ok != want[:n])[:8])
    finally:
        ctx.release_base(h)


@pytest.mark.parametrize("width", [8, 16])
def test_key_table_widths(ctx, batches, answers, width):
    """the key's table at 8 and 16 bits beside G's table as it stands (each walk reads its own header)"""
    bt, want = _batch(batches, "secp256k1"), answers("secp256k1")
    h = ctx.define_base("secp256k1", bt["pub"].tobytes(), width)
    try:
        assert ctx.base_info(h)[1] == width
        for mem, n in (("dev_torch", 4099), ("host", 257)):
            ok = VB.run_verify(ctx, h, bt["h"][:n], bt["r"][:n], bt["s"][:n], 0, mem)
            assert ok.tobytes() == want[:n].tobytes()
        assert ctx.comb_bits("secp256k1") != 0          # (G's table: built by the call, at its own width)
    finally:
        ctx.release_base(h)


@pytest.mark.parametrize("name", ["secp256k1", "p384", "brainpoolP256r1", "cof_p10007"])
def test_alias_as_a_key(ctx, cids, batches, answers, name):
    """the generator alias is the key with d = 1: G's table walked twice, by the alias, by G's
    coordinates and by -G's (the accumulator meets +- an entry, passes through O, ends on O)"""
    spec = VB.spec_of(name)
    bt, want = _batch(batches, name, 0), answers(name, 0)
    alias = ctx.define_base(cids(name), None)
    g = ctx.define_base(cids(name), bt["pub"].tobytes())
    try:
        for h, mem in ((alias, "dev_torch"), (alias, "host"), (g, "dev_torch")):
            ok = VB.run_verify(ctx, h, bt["h"], bt["r"], bt["s"], 0, mem)
            assert ok.tobytes() == want.tobytes(), (name, h, mem)
        assert ctx.base_info(alias)[1] == (ctx.comb_bits(name) if name in VB.PRESETS else 8) != 0
    finally:
        ctx.release_base(g)
        ctx.release_base(alias)
    _, hs = VB.define_keys(ctx, spec, 0, cids(name))
    try:
        VB.check_golden(ctx, {**spec, "cases": spec["cases"][:2]}, hs[:2], "dev_torch")
    finally:
        for h in hs:
            ctx.release_base(h)


def test_device_operands_are_checked(ctx, batches):
    import torch
    bt = _batch(batches, "p192")
    h = ctx.define_base("p192", bt["pub"].tobytes())
    try:
        hh, r, s = (torch.from_numpy(bt[k][:3].copy()).cuda() for k in ("h", "r", "s"))
        ok = torch.zeros(3, dtype=torch.uint8, device="cuda")
        for bad in (None, (), (ok, ok), (ok[:2],), (ok.cpu(),), (ok.to(torch.int32),)):
            with pytest.raises(ValueError):
                ctx.ecdsa_verify_base(h, hh, r, s, out=bad)
        for bad in ((hh, r[:, :23], s), (hh, r, s[:2]), (hh, r.cpu(), s), (hh, r, s.to(torch.int16)), (hh.reshape(-1), r, s)):
            with pytest.raises(ValueError):
                ctx.ecdsa_verify_base(h, *bad, out=(ok,))
        with pytest.raises(ValueError):
            ctx.ecdsa_verify_base(h, hh, bt["r"][:3], s, out=(ok,))          # a host array among device tensors
        assert ctx.ecdsa_verify_base(h, hh, r, s, out=(ok,)) is ok
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == bt["want"][:3]).all()
    finally:
        ctx.release_base(h)
