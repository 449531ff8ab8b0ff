"""EdDSA verification against a fixed-base table of the signer's key (ellgpu_eddsa_verify_base) on the
CPU: the hostsim build of the device code (tests/hostsim) against the reference's recorded verdicts
(tests/golden/eddsa_verify_base.json), against the Python-integer model of
tests/eddsa_verify_base_checks.py and against ellgpu_eddsa_verify with encodePoint(A) repeated per
item; torsion keys, the generator alias, both message forms, and every refusal."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import eddsa_verify_base_checks as EB  # noqa: E402

OPTIONAL = ("ellgpu_probe_valu", "ellgpu_ctx_set_timing", "ellgpu_ctx_get_timing", "ellgpu_debug_field_op")
E_ARG, E_UNSUPPORTED = -2, -5
BATCH_KEYS = ["aG1", "aG_T8", "G", "negG"]          # ("G" runs on the generator alias)


@pytest.fixture(scope="module")
def hs():
    return _lib.load(build_hostsim(), optional=OPTIONAL)


@pytest.fixture(scope="module")
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batches():
    """one 203-item batch per key and the model's verdicts, shared by every test"""
    return {k: EB.random_batch(203, 1, k) for k in BATCH_KEYS}


def _handle(ctx, key):
    return ctx.define_ed_base("ed25519", None) if key == "G" else EB.define_key(ctx, key)


def test_fixture_shape():
    EB.check_fixture_shape()


def test_model_is_pinned_to_the_fixture():
    EB.check_model_pinned()


@pytest.mark.parametrize("name", EB.KEYS)
def test_golden(ctx, name):
    """every recorded case of the key through both memory kinds and both message forms"""
    h = EB.define_key(ctx, name)
    try:
        a = EB.check_golden(ctx, name, h, "host")
        b = EB.check_golden(ctx, name, h, "dev_np")
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    finally:
        ctx.release_base(h)


@pytest.mark.parametrize("key", BATCH_KEYS)
def test_batch_meets_the_conditions(batches, key):
    assert EB.batch_meets_conditions(batches[key])


@pytest.mark.parametrize("key", BATCH_KEYS)
def test_random_batch_matches_model_and_verify(ctx, batches, key):
    """203 items on one key: the model's (ok, err), and byte for byte what ellgpu_eddsa_verify writes
    with the key repeated, at n = 1, 8, 9, 41 and 203 through both memory kinds; and with out_err NULL"""
    bt = batches[key]
    h = _handle(ctx, key)
    try:
        tok, terr = EB.tiled_verify(ctx, bt, 203)
        assert (tok == bt["want"][0]).all() and (terr == bt["want"][1]).all()
        for n in (1, 8, 9, 41, 203):
            for mem in ("host", "dev_np"):
                ok, err = EB.run_verify(ctx, h, bt["msgs"][:n], bt["sigs"][:n], mem, offsets=True)
                assert (ok == bt["want"][0][:n]).all() and (err == bt["want"][1][:n]).all(), (key, n, mem)
                assert ok.tobytes() == tok[:n].tobytes() and err.tobytes() == terr[:n].tobytes(), (key, n, mem)
                ok2, none = EB.run_verify(ctx, h, bt["msgs"][:n], bt["sigs"][:n], mem, offsets=True, want_err=False)
                assert none is None and ok2.tobytes() == ok.tobytes()
    finally:
        ctx.release_base(h)


def test_alias_against_g_by_coordinates(ctx, batches):
    """the generator alias (both walks read the curve's own table) and G given by coordinates -- a
    handle of its own with a table of its own, as test_fixed_base_ed_hostsim.py has it -- are the
    same key: the recorded verdicts of G, and the same bytes on a batch"""
    alias = ctx.define_ed_base("ed25519", None)
    g = ctx.define_ed_base("ed25519", EB.xy_bytes("G"))
    assert g != alias and ctx.define_ed_base("ed25519", None) == alias
    try:
        bt = batches["G"]
        ok, err = EB.run_verify(ctx, alias, bt["msgs"][:41], bt["sigs"][:41], "host", offsets=True)
        assert (ok == bt["want"][0][:41]).all() and (err == bt["want"][1][:41]).all()
        ok2, err2 = EB.run_verify(ctx, g, bt["msgs"][:41], bt["sigs"][:41], "dev_np", offsets=True)
        assert ok2.tobytes() == ok.tobytes() and err2.tobytes() == err.tobytes()
        EB.check_golden(ctx, "G", alias, "host")
    finally:
        ctx.release_base(g)


def _code(call):
    with pytest.raises(_lib.EllgpuError) as e:
        call()
    return e.value.code, str(e.value)


def test_refusals(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        P = lambda a: a.ctypes.data  # noqa: E731
        bt = EB.random_batch(4, 4, "aG2")
        msgs = [m.ljust(8, b"\7")[:8] for m in bt["msgs"]]              # a uniform stride of 8
        flat, off = EB.pack(msgs)
        sigs = bt["sigs"].copy()
        ok, err = np.full(4, EB.FILL, np.uint8), np.full(4, EB.FILL, np.uint8)
        h = EB.define_key(c, "aG2")
        call = lambda base, n, *a: hs.ellgpu_eddsa_verify_base(c._ctx, base, n, *a)  # noqa: E731
        good = (P(flat), None, 8, P(sigs), P(ok), P(err))
        want = EB.model_many(msgs, [s.tobytes() for s in sigs], bt["enc"].tobytes())
        assert call(h, 4, *good, 0, None) == 0 and (ok == want[0]).all() and (err == want[1]).all()
        # a short-curve handle, and an Edwards handle on a user-defined id -- at n == 0 too
        from oracle import ec_oracle as O
        g256 = O.get_curve("p256").g
        sh = c.define_base("p256", g256.x.to_bytes(32, "big") + g256.y.to_bytes(32, "big"))
        p1174 = 2 ** 251 - 9
        ce = c.define_edwards(p1174, 1, p1174 - 1174)
        ue = c.define_ed_base(ce, (0).to_bytes(32, "big") + (1).to_bytes(32, "big"))
        for base, word in ((sh, b"ellgpu_ed_base_define"), (ue, b"no EdDSA")):
            for n in (4, 0):
                for mem in (0, 1):
                    assert call(base, n, *good, mem, None) == E_UNSUPPORTED and word in hs.ellgpu_last_error(), (base, n, mem)
            assert call(base, 0, None, None, 0, None, None, None, 0, None) == E_UNSUPPORTED
        # ecdsa_verify_base keeps refusing the ed25519 handle, in its own words
        hh = np.zeros((4, 32), np.uint8)
        code, msg = _code(lambda: c.ecdsa_verify_base(h, hh, hh, hh))
        assert code == E_UNSUPPORTED and "short Weierstrass" in msg
        # an unknown handle, a released handle
        assert call(12345, 4, *good, 0, None) == E_ARG and b"unknown base handle" in hs.ellgpu_last_error()
        h2 = EB.define_key(c, "aG1")
        c.release_base(h2)
        assert call(h2, 4, *good, 0, None) == E_ARG and call(h2, 0, *good, 0, None) == E_ARG
        # mem, and a stream with host memory
        for mem in (-1, 2, 7):
            assert call(h, 4, *good, mem, None) == E_ARG
        stream = ctypes.c_void_p(hs.ellgpu_ctx_stream(c._ctx) or 1)
        assert call(h, 4, *good, 0, stream) == E_ARG
        assert call(h, 4, *good, 1, None) == 0
        # null pointers, either memory kind: msgs, sigs, out_ok -- not out_err, and not a null msgs
        # where the total length is zero
        for mem in (0, 1):
            for miss in (0, 3, 4):
                args = list(good)
                args[miss] = None
                assert call(h, 4, *args, mem, None) == E_ARG, (mem, miss)
            args = list(good)
            args[5] = None
            assert call(h, 4, *args, mem, None) == 0
            assert call(h, 4, None, None, 0, P(sigs), P(ok), P(err), mem, None) == 0
            assert call(h, 4, None, P(off), 0, P(sigs), P(ok), P(err), mem, None) == E_ARG
            assert hs.ellgpu_eddsa_verify_base(None, h, 4, *good, mem, None) == E_ARG
        zoff = np.zeros(5, np.uint64)
        assert call(h, 4, None, P(zoff), 0, P(sigs), P(ok), P(err), 0, None) == 0      # four empty messages
        # decreasing offsets (a host call reads them)
        bad = off.copy()
        bad[2] = bad[1] - 1
        assert call(h, 4, P(flat), P(bad), 0, P(sigs), P(ok), P(err), 0, None) == E_ARG
        assert b"non-decreasing" in hs.ellgpu_last_error()
        assert call(h, 4, P(flat), P(off), 0, P(sigs), P(ok), P(err), 0, None) == 0 and (ok == want[0]).all()
        # each overlap pair on device memory: sigs / msgs against out_ok / out_err, out_ok against out_err
        buf = np.zeros(4 * 64 + 8, np.uint8)
        buf[:256] = sigs.reshape(-1)
        for inp in (0, 3):
            for res in (4, 5):
                size = 32 if inp == 0 else 256
                args = list(good)
                args[inp] = P(buf)
                args[res] = P(buf) + size - 1
                assert call(h, 4, *args, 1, None) == E_ARG and b"overlap" in hs.ellgpu_last_error(), (inp, res)
                args[res] = P(buf) + size
                assert call(h, 4, *args, 1, None) == 0, (inp, res)
        both = np.zeros(8, np.uint8)
        args = list(good)
        args[4], args[5] = P(both), P(both) + 3
        assert call(h, 4, *args, 1, None) == E_ARG and b"overlap" in hs.ellgpu_last_error()
        args[5] = P(both) + 4
        assert call(h, 4, *args, 1, None) == 0
        # n == 0: nothing is touched, whatever the pointers are
        ok[:], err[:] = EB.FILL, EB.FILL
        for mem in (0, 1):
            assert call(h, 0, None, None, 0, None, None, None, mem, None) == 0
            assert call(h, 0, *good, mem, None) == 0
        assert (ok == EB.FILL).all() and (err == EB.FILL).all()
        for x in (h, sh, ue):
            c.release_base(x)
    finally:
        c.close()


def test_sharded_over_a_group(hs):
    """a group of two members shards a host batch of uniform stride; with offsets the call runs on
    the first member -- the same bytes either way"""
    g = elliptic_amd.Context(lib_path=hs, devices=[0, 0])
    try:
        bt = EB.random_batch(41, 3, "aG_T8")
        want = bt["want"]
        h = EB.define_key(g, "aG_T8")
        for n in (1, 2, 41):
            ok, err = EB.run_verify(g, h, bt["msgs"][:n], bt["sigs"][:n], "host", offsets=True)
            assert (ok == want[0][:n]).all() and (err == want[1][:n]).all()
        msgs = [m.ljust(16, b"\1")[:16] for m in bt["msgs"]]
        wok, werr = EB.model_many(msgs, [s.tobytes() for s in bt["sigs"]], bt["enc"].tobytes())
        for n in (1, 2, 41):
            ok, err = EB.run_verify(g, h, msgs[:n], bt["sigs"][:n], "host", offsets=False)
            assert (ok == wok[:n]).all() and (err == werr[:n]).all()
            ok, _ = EB.run_verify(g, h, msgs[:n], bt["sigs"][:n], "host", offsets=False, want_err=False)
            assert (ok == wok[:n]).all()
        assert g._lib.ellgpu_eddsa_verify_base(g._ctx, h, 0, None, None, 16, None, None, None, 0, None) == 0
        g.release_base(h)
    finally:
        g.close()


def test_python_argument_checks(ctx, batches):
    bt = batches["aG1"]
    h = EB.define_key(ctx, "aG1")
    try:
        msgs, sigs = bt["msgs"][:3], bt["sigs"][:3]
        with pytest.raises(ValueError):
            ctx.eddsa_verify_base(h, msgs, sigs[:, :63])
        with pytest.raises(ValueError):
            ctx.eddsa_verify_base(h, np.zeros((2, 5), np.uint8), sigs)
        with pytest.raises(ValueError):
            ctx.eddsa_verify_base(h, msgs, sigs, msg_off=np.zeros(4, np.uint64))
        with pytest.raises(AssertionError):
            ctx.eddsa_verify_base(h, msgs, sigs, out=(np.zeros(2, np.uint8), np.zeros(3, np.uint8)))
        ok, err = ctx.eddsa_verify_base(h, msgs, sigs)
        assert ok.dtype == np.uint8 and ok.shape == (3,) and (ok == bt["want"][0][:3]).all() and (err == bt["want"][1][:3]).all()
    finally:
        ctx.release_base(h)


def test_kernel_launches(hs, ctx, batches):
    """the call is eddsa_base, one launch per chunk: no per-item verify kernel, no lanes-per-item
    parts, no separate comb walk, no normalisation"""
    if not hasattr(hs, "hs_launches"):
        pytest.skip("this hostsim build does not count launches")
    hs.hs_launches.restype = ctypes.c_long
    hs.hs_launches.argtypes = [ctypes.c_char_p]
    names = [b"eddsa_base", b"eddsa_verify", b"eddsa_parts_c", b"eddsa_join", b"ed_mul_base2", b"ed_normalize"]
    bt = batches["aG1"]
    h = EB.define_key(ctx, "aG1")
    EB.run_verify(ctx, h, bt["msgs"][:9], bt["sigs"][:9], "host", offsets=True)     # (G's table exists from here on)
    for n in (1, 41):
        before = [hs.hs_launches(nm) for nm in names]
        EB.run_verify(ctx, h, bt["msgs"][:n], bt["sigs"][:n], "host", offsets=True)
        d = [hs.hs_launches(nm) - b for nm, b in zip(names, before)]
        assert d == [1, 0, 0, 0, 0, 0], (n, d)
    ctx.release_base(h)
