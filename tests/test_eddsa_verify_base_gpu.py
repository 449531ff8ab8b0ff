"""EdDSA verification against a fixed-base table of the signer's key, on the device: the reference's
recorded verdicts (tests/golden/eddsa_verify_base.json), and per key one 4 099-item batch whose
expected bytes are the engine's own ellgpu_eddsa_verify with encodePoint(A) repeated per item (held
to the Python-integer model on its first 64 rows), which ellgpu_eddsa_verify_base must give byte for
byte, ok and err, at n = 1 ... 4 099 through alternating memory kinds; both message forms on device
tensors, out=(ok,), the generator alias as a key, and the checks of device operands."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eddsa_verify_base_checks as EB  # noqa: E402

SIZES = [1, 63, 64, 65, 257, 4099]
BATCH_KEYS = ["aG1", "aG_T8", "G"]                 # ("G" runs on the generator alias)
_batches = {}


def _batch(key):
    if key not in _batches:
        _batches[key] = EB.random_batch(4099, 2, key, model_rows=64)
    return _batches[key]


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
def answers(ctx):
    """key -> the batch through ellgpu_eddsa_verify with the key tiled, computed once"""
    made = {}

    def get(key):
        if key not in made:
            bt = _batch(key)
            ok, err = EB.tiled_verify(ctx, bt, 4099)
            assert (ok[:64] == bt["want"][0]).all() and (err[:64] == bt["want"][1]).all()
            assert set(ok.tolist()) == {0, 1} and set(err.tolist()) == {0, 1}
            made[key] = (ok, err)
        return made[key]
    return get


def _handle(ctx, key):
    return ctx.define_ed_base("ed25519", None) if key == "G" else EB.define_key(ctx, key)


@pytest.mark.parametrize("key", BATCH_KEYS)
def test_batch_meets_the_conditions(key):
    """both verdicts, an err, and S = n, an undecodable R, the non-canonical identity and S = 0 among
    the first rows, by construction (CPU: the model alone)"""
    assert EB.batch_meets_conditions(_batch(key))


@pytest.mark.gpu
@pytest.mark.parametrize("name", EB.KEYS)
def test_golden(ctx, name):
    h = EB.define_key(ctx, name)
    try:
        a = EB.check_golden(ctx, name, h, "host")
        b = EB.check_golden(ctx, name, h, "dev_torch")
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    finally:
        ctx.release_base(h)


@pytest.mark.gpu
@pytest.mark.parametrize("key", BATCH_KEYS)
def test_batch_sizes(ctx, answers, key):
    """one batch, checked at n = 1 ... 4 099, the memory kinds alternating (device tensors: the
    messages flat with offsets on the device); once with out=(ok,)"""
    bt, (wok, werr) = _batch(key), answers(key)
    h = _handle(ctx, key)
    try:
        for j, n in enumerate(SIZES):
            for mem in (("dev_torch" if j & 1 else "host"),) + (("host",) if n == 65 else ()):
                ok, err = EB.run_verify(ctx, h, bt["msgs"][:n], bt["sigs"][:n], mem, offsets=True)
                assert ok.tobytes() == wok[:n].tobytes(), (key, n, mem, np.flatnonzero(ok != wok[:n])[:8])
                assert err.tobytes() == werr[:n].tobytes(), (key, n, mem, np.flatnonzero(err != werr[:n])[:8])
        ok, none = EB.run_verify(ctx, h, bt["msgs"], bt["sigs"], "dev_torch", offsets=True, want_err=False)
        assert none is None and ok.tobytes() == wok.tobytes()
    finally:
        ctx.release_base(h)


@pytest.mark.gpu
def test_uniform_stride_on_the_device(ctx):
    """(n, len) messages on device tensors and on the host against the offsets form of the same items"""
    bt = _batch("aG_T8")
    n = 257
    msgs = [m.ljust(48, b"\5")[:48] for m in bt["msgs"][:n]]
    h = EB.define_key(ctx, "aG_T8")
    try:
        wok, werr = EB.tiled_verify(ctx, {**bt, "msgs": msgs}, n)
        mok, merr = EB.model_many(msgs[:16], [s.tobytes() for s in bt["sigs"][:16]], bt["enc"].tobytes())
        assert (wok[:16] == mok).all() and (werr[:16] == merr).all()
        for mem, offsets in (("dev_torch", False), ("host", False), ("dev_torch", True)):
            ok, err = EB.run_verify(ctx, h, msgs, bt["sigs"][:n], mem, offsets=offsets)
            assert ok.tobytes() == wok.tobytes() and err.tobytes() == werr.tobytes(), (mem, offsets)
    finally:
        ctx.release_base(h)


@pytest.mark.gpu
def test_device_operands_are_checked(ctx):
    import torch
    bt = _batch("aG1")
    h = EB.define_key(ctx, "aG1")
    try:
        msgs = [m.ljust(8, b"\2")[:8] for m in bt["msgs"][:3]]
        m = torch.from_numpy(np.frombuffer(b"".join(msgs), np.uint8).reshape(3, 8).copy()).cuda()
        s = torch.from_numpy(bt["sigs"][:3].copy()).cuda()
        ok = torch.zeros(3, dtype=torch.uint8, device="cuda")
        err = torch.zeros(3, dtype=torch.uint8, device="cuda")
        off = torch.arange(0, 32, 8, dtype=torch.int64, device="cuda")
        for bad in (None, (), (ok, err, ok), (ok[:2],), (ok.cpu(),), (ok.to(torch.int32),), (ok, err[:2]), (ok, err.cpu())):
            with pytest.raises(ValueError):
                ctx.eddsa_verify_base(h, m, s, out=bad)
        for bad in ((m, s[:, :63]), (m[:2], s), (m.cpu(), s), (m.to(torch.int16), s), (m.reshape(-1), s), (m[:, ::2], s)):
            with pytest.raises(ValueError):
                ctx.eddsa_verify_base(h, *bad, out=(ok, err))
        for bad in (off[:3], off.cpu(), off.to(torch.int32), off.cpu().numpy()):
            with pytest.raises(ValueError):
                ctx.eddsa_verify_base(h, m.reshape(-1), s, msg_off=bad, out=(ok, err))
        with pytest.raises(ValueError):
            ctx.eddsa_verify_base(h, m, s, msg_off=off, out=(ok, err))            # offsets go with flat messages
        want = EB.model_many(msgs, [x.tobytes() for x in bt["sigs"][:3]], bt["enc"].tobytes())
        got = ctx.eddsa_verify_base(h, m, s, out=(ok, err))
        assert got[0] is ok and got[1] is err
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == want[0]).all() and (err.cpu().numpy() == want[1]).all()
        ok.fill_(EB.FILL)
        got = ctx.eddsa_verify_base(h, m.reshape(-1), s, msg_off=off, out=(ok,))
        assert got[0] is ok and got[1] is None
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == want[0]).all()
    finally:
        ctx.release_base(h)
