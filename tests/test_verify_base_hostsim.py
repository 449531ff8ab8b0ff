"""ECDSA verification against a fixed-base table of the signer's key (ellgpu_ecdsa_verify_base) on the
CPU: the hostsim build of the device code (tests/hostsim) against the reference's recorded verdicts
(tests/golden/verify_base.json), against the Python-integer model of tests/verify_base_checks.py and
against ellgpu_ecdsa_verify with the key repeated per item; keys +-G against G's own table, two
table widths, and every refusal."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import verify_base_checks as VB  # noqa: E402

OPTIONAL = ("ellgpu_probe_valu", "ellgpu_ctx_set_timing", "ellgpu_ctx_get_timing", "ellgpu_debug_field_op")
E_ARG, E_UNSUPPORTED = -2, -5


@pytest.fixture(scope="module")
def hs():
    return _lib.load(build_hostsim(), optional=OPTIONAL)


@pytest.fixture(scope="module")
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cids(ctx):
    """one curve id per fixture entry: a user-defined domain is defined once for the whole module"""
    return {name: VB.curve_id(ctx, VB.spec_of(name)) for name in VB.NAMES}


@pytest.fixture(scope="module")
def batches():
    """one 203-item batch per curve and the model's verdicts, shared by every test"""
    return {name: VB.random_batch(VB.spec_of(name), 203, 1) for name in VB.NAMES}


def _code(call):
    with pytest.raises(_lib.EllgpuError) as e:
        call()
    return e.value.code, str(e.value)


def test_curve_set():
    assert [c["name"] for c in VB.curves()] == VB.NAMES
    for name in VB.NAMES:
        VB.check_fixture_shape(VB.spec_of(name))
    D = VB.domain_of(VB.spec_of("secp224k1"))
    assert D.n > D.p and D.maxwell
    D = VB.domain_of(VB.spec_of("cof_p10007"))
    assert D.p // D.n == 2 and D.maxwell


@pytest.mark.parametrize("name", VB.NAMES)
def test_model_is_pinned_to_the_fixture(name):
    VB.check_model_pinned(VB.spec_of(name))


@pytest.mark.parametrize("name", VB.NAMES)
def test_golden(ctx, cids, name):
    """every recorded case of every key through both memory kinds: the reference's verdicts, the
    same bytes, nothing but 0 and 1"""
    spec = VB.spec_of(name)
    _, hs_ = VB.define_keys(ctx, spec, 0, cids[name])
    try:
        a = VB.check_golden(ctx, spec, hs_, "host")
        b = VB.check_golden(ctx, spec, hs_, "dev_np")
        assert all((u == v).all() for u, v in zip(a, b))
        assert set(np.concatenate(a).tolist()) == {0, 1}
    finally:
        for h in hs_:
            ctx.release_base(h)


@pytest.mark.parametrize("name", VB.NAMES)
def test_batch_meets_the_conditions(batches, name):
    assert VB.batch_meets_conditions(VB.spec_of(name), batches[name])


@pytest.mark.parametrize("name", VB.NAMES)
def test_random_batch_matches_model_and_verify(ctx, cids, batches, name):
    """203 items on one key: the model's verdicts, and byte for byte what ellgpu_ecdsa_verify writes
    with the key repeated, at n = 1, 8, 9, 41 and 203 through both memory kinds"""
    spec, bt = VB.spec_of(name), batches[name]
    h = ctx.define_base(cids[name], bt["pub"].tobytes(), 0)
    try:
        tiled = VB.tiled_verify(ctx, cids[name], bt, 203)
        assert (tiled == bt["want"]).all()
        for n in (1, 8, 9, 41, 203):
            for mem in ("host", "dev_np"):
                ok = VB.run_verify(ctx, h, bt["h"][:n], bt["r"][:n], bt["s"][:n], 0, mem)
                assert (ok == bt["want"][:n]).all() and ok.tobytes() == tiled[:n].tobytes(), (name, n, mem)
                assert set(ok.tolist()) <= {0, 1}
    finally:
        ctx.release_base(h)


@pytest.mark.parametrize("name", VB.NAMES)
def test_keys_plus_minus_g_against_gs_table(ctx, cids, name):
    """Q = G (by coordinates and as the generator alias) and Q = -G at every width the CPU build
    walks, beside G's own table: the second walk meets +- an entry of the first, passes through O
    and ends on O.  The recorded cases of the keys d = 1 and d = n - 1, and a batch signed with d = 1."""
    spec = VB.spec_of(name)
    B = spec["B"]
    keys = VB.keys_of(spec)
    bt = VB.random_batch(spec, 41, 2, key=0)
    assert VB.batch_meets_conditions(spec, bt)
    alias = ctx.define_base(cids[name], None)
    handles = [alias]
    try:
        for width in VB.FB.widths_of(name):
            hs_ = [ctx.define_base(cids[name], VB.xy_bytes(keys[i][1], B), width) for i in (0, 1)]
            handles += hs_
            assert [ctx.base_info(h)[1] for h in hs_] == [width, width]
            for h, cs in zip(hs_, spec["cases"][:2]):
                for (hl, bits), idx in VB.case_groups(cs):
                    hh = np.stack([np.frombuffer(bytes.fromhex(cs[j][1]), np.uint8) for j in idx])
                    ok = VB.run_verify(ctx, h, hh, VB.rows([VB.I(cs[j][3]) for j in idx], B),
                                       VB.rows([VB.I(cs[j][4]) for j in idx], B), bits)
                    assert ok.tolist() == [cs[j][5] for j in idx], (name, width, hl, bits)
            assert (VB.run_verify(ctx, hs_[0], bt["h"], bt["r"], bt["s"]) == bt["want"]).all()
        assert (VB.run_verify(ctx, alias, bt["h"], bt["r"], bt["s"]) == bt["want"]).all()
        assert (VB.run_verify(ctx, alias, bt["h"], bt["r"], bt["s"], 0, "dev_np") == bt["want"]).all()
    finally:
        for h in set(handles):
            ctx.release_base(h)


@pytest.mark.parametrize("name", VB.SIGNED)
def test_two_key_table_widths_give_the_same_verdicts(ctx, cids, batches, name):
    """the key's table at 4 and at 8 bits beside G's table as it stands: each walk reads its own header"""
    spec, bt = VB.spec_of(name), batches[name]
    hs_ = [ctx.define_base(name, bt["pub"].tobytes(), w) for w in (4, 8)]
    try:
        assert [ctx.base_info(h)[1] for h in hs_] == [4, 8] and ctx.comb_bits(name) == 8
        a, b = (VB.run_verify(ctx, h, bt["h"], bt["r"], bt["s"]) for h in hs_)
        assert (a == bt["want"]).all() and a.tobytes() == b.tobytes()
    finally:
        for h in hs_:
            ctx.release_base(h)


def test_sharded_over_a_group(hs):
    """a group of two members shards a host batch as ellgpu_mul_base2's is sharded"""
    g = elliptic_amd.Context(lib_path=hs, devices=[0, 0])
    try:
        spec = VB.spec_of("p192")
        bt = VB.random_batch(spec, 41, 3)
        h = g.define_base("p192", bt["pub"].tobytes())
        for n in (1, 2, 41):
            assert (VB.run_verify(g, h, bt["h"][:n], bt["r"][:n], bt["s"][:n]) == bt["want"][:n]).all()
        assert g._lib.ellgpu_ecdsa_verify_base(g._ctx, h, 0, None, 24, 0, None, None, None, 0, None) == 0
        g.release_base(h)
    finally:
        g.close()


def test_refusals(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        P = lambda a: a.ctypes.data  # noqa: E731
        spec = VB.spec_of("p256")
        bt = VB.random_batch(spec, 4, 4)
        hh, r, s = bt["h"].copy(), bt["r"].copy(), bt["s"].copy()
        ok = np.full(4, VB.FILL, np.uint8)
        h = c.define_base("p256", bt["pub"].tobytes())
        call = lambda base, n, *a: hs.ellgpu_ecdsa_verify_base(c._ctx, base, n, *a)  # noqa: E731
        good = (P(hh), 32, 0, P(r), P(s), P(ok))
        assert call(h, 4, *good, 0, None) == 0 and (ok == bt["want"]).all()
        # an Edwards handle
        ed = c.define_ed_base("ed25519", None)
        code, msg = _code(lambda: c.ecdsa_verify_base(ed, hh, r, s))
        assert code == E_UNSUPPORTED and "short Weierstrass" in msg
        # a plain user-defined short id: the wording of ellgpu_ecdsa_verify
        s192 = VB.spec_of("secp192k1")
        plain = c.define_short(VB.I(s192["p"]), VB.I(s192["a"]), VB.I(s192["b"]))
        hp = c.define_base(plain, VB.xy_bytes(VB.keys_of(s192)[2][1], 32))
        code, msg = _code(lambda: c.ecdsa_verify_base(hp, hh, r, s))
        assert code == E_UNSUPPORTED and "needs its domain" in msg
        pub = np.ascontiguousarray(np.broadcast_to(np.frombuffer(VB.xy_bytes(VB.keys_of(s192)[2][1], 32), np.uint8), (4, 64)))
        code2, msg2 = _code(lambda: c.ecdsa_verify(plain, hh, r, s, pub))
        assert code2 == E_UNSUPPORTED and msg2 == msg
        # ... and both at n == 0 too: the handle is looked up whatever n is
        assert call(ed, 0, None, 32, 0, None, None, None, 0, None) == E_UNSUPPORTED
        assert call(hp, 0, None, 32, 0, None, None, None, 1, None) == E_UNSUPPORTED
        # an unknown handle, a released handle
        assert call(12345, 4, *good, 0, None) == E_ARG and b"unknown base handle" in hs.ellgpu_last_error()
        h2 = c.define_base("p256", VB.xy_bytes(VB.keys_of(spec)[2][1], 32))
        c.release_base(h2)
        assert call(h2, 4, *good, 0, None) == E_ARG and call(h2, 0, *good, 0, None) == E_ARG
        # mem, and a stream with host memory
        for mem in (-1, 2, 7):
            assert call(h, 4, *good, mem, None) == E_ARG
        stream = ctypes.c_void_p(hs.ellgpu_ctx_stream(c._ctx) or 1)
        assert call(h, 4, *good, 0, stream) == E_ARG
        assert call(h, 4, *good, 1, None) == 0
        # null pointers, either memory kind
        for mem in (0, 1):
            for miss in (0, 3, 4, 5):
                args = list(good)
                args[miss] = None
                assert call(h, 4, *args, mem, None) == E_ARG, (mem, miss)
            assert hs.ellgpu_ecdsa_verify_base(None, h, 4, *good, mem, None) == E_ARG
        # overlap of an operand and the verdicts (device memory)
        buf = np.zeros(4 * 32 + 4, np.uint8)
        for which in (0, 3, 4):
            args = list(good)
            args[which] = P(buf)
            args[5] = P(buf) + 4 * 32 - 1
            assert call(h, 4, *args, 1, None) == E_ARG and b"overlap" in hs.ellgpu_last_error()
            args[5] = P(buf) + 4 * 32
            assert call(h, 4, *args, 1, None) == 0
        # hash_len / msg_bits beyond truncate_shift's limit, as in ellgpu_ecdsa_verify
        wide = np.zeros((4, 72), np.uint8)
        pub = np.ascontiguousarray(np.broadcast_to(bt["pub"], (4, 64)))
        for mem in (0, 1):
            assert call(h, 4, P(wide), 72, 0, P(r), P(s), P(ok), mem, None) == 0      # 72 bytes shift down to 256 bits
            assert call(h, 4, P(wide), 40, 300, P(r), P(s), P(ok), mem, None) == E_ARG   # 320 - 44 bits are left
            assert b"more bits than the order width" in hs.ellgpu_last_error()
            assert call(h, 4, P(wide), 0, 0, P(r), P(s), P(ok), mem, None) == E_ARG
            assert call(h, 4, P(wide), 32, -1, P(r), P(s), P(ok), mem, None) == E_ARG
        assert hs.ellgpu_ecdsa_verify(c._ctx, 3, 4, P(wide), 40, 300, P(r), P(s), P(pub), P(ok), None) == E_ARG
        # n == 0: nothing is touched, whatever the pointers are
        ok[:] = VB.FILL
        for mem in (0, 1):
            assert call(h, 0, None, 32, 0, None, None, None, mem, None) == 0
            assert call(h, 0, *good, mem, None) == 0
        assert (ok == VB.FILL).all()
        for x in (h, ed, hp):
            c.release_base(x)
    finally:
        c.close()


def test_python_argument_checks(ctx, cids):
    spec = VB.spec_of("p224")
    bt = VB.random_batch(spec, 3, 5)
    h = ctx.define_base("p224", bt["pub"].tobytes())
    try:
        with pytest.raises(ValueError):
            ctx.ecdsa_verify_base(h, bt["h"], bt["r"][:, :27], bt["s"])
        with pytest.raises(ValueError):
            ctx.ecdsa_verify_base(h, bt["h"].reshape(-1), bt["r"], bt["s"])
        with pytest.raises(AssertionError):
            ctx.ecdsa_verify_base(h, bt["h"], bt["r"], bt["s"], out=(np.zeros(2, np.uint8),))
        ok = ctx.ecdsa_verify_base(h, bt["h"], bt["r"], bt["s"])
        assert ok.dtype == np.uint8 and ok.shape == (3,) and (ok == bt["want"]).all()
    finally:
        ctx.release_base(h)


def test_kernel_launches(hs, ctx, cids, batches):
    """the call is ecdsa_prep and ecdsa_base, one launch of each per chunk: no ladder, no normalisation"""
    if not hasattr(hs, "hs_launches"):
        pytest.skip("this hostsim build does not count launches")
    hs.hs_launches.restype = ctypes.c_long
    hs.hs_launches.argtypes = [ctypes.c_char_p]
    names = [b"ecdsa_prep", b"ecdsa_base", b"ecdsa_main", b"mul_var", b"normalize", b"mul_base2"]
    for name in ("p256", "brainpoolP256r1"):
        bt = batches[name]
        h = ctx.define_base(cids[name], bt["pub"].tobytes())
        VB.run_verify(ctx, h, bt["h"][:9], bt["r"][:9], bt["s"][:9])           # (G's table exists from here on)
        before = [hs.hs_launches(nm) for nm in names]
        VB.run_verify(ctx, h, bt["h"][:41], bt["r"][:41], bt["s"][:41])
        d = [hs.hs_launches(nm) - b for nm, b in zip(names, before)]
        assert d[0] == d[1] >= 1 and d[2:] == [0, 0, 0, 0], d
        ctx.release_base(h)
