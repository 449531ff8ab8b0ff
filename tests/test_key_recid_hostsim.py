"""The recovery id of a signature under a known key in one pass (ellgpu_ecdsa_recid) on the CPU: the
hostsim build of the device code (tests/hostsim) against the reference's recorded answers
(tests/golden/key_recid.json) and against the Python-integer model of tests/key_recid_checks.py, with
the cross-checks through ellgpu_ecdsa_recover and ellgpu_ecdsa_verify, every refusal, and a run with
three items per shared inversion."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import key_recid_checks as KR  # noqa: E402
import verify_base_checks as VB  # noqa: E402

E_ARG, E_UNSUPPORTED = -2, -5


@pytest.fixture(scope="module")
def hs():
    return _lib.load(build_hostsim(), optional=KR.OPTIONAL)


@pytest.fixture(scope="module")
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batches():
    """one 257-item batch per curve with the model's answers, shared by every test"""
    return {name: KR.random_batch(name, 257) for name in KR.PRESETS}


def test_curve_set():
    assert [c["name"] for c in KR.curves()] == KR.PRESETS
    for name in KR.PRESETS:
        KR.check_fixture_shape(KR.spec_of(name))


@pytest.mark.parametrize("name", KR.PRESETS)
def test_model_is_pinned_to_the_fixture(name):
    KR.check_model_pinned(KR.spec_of(name))


@pytest.mark.parametrize("name", KR.PRESETS)
def test_golden(ctx, name):
    """every recorded row, in fixture order and shuffled, through both memory kinds: the reference's
    answers; ecdsa_recover gives the key back for every id; on the curves whose n fills its bytes
    status 0 <=> ecdsa_verify accepts"""
    spec = KR.spec_of(name)
    for shuffled in (False, True):
        for bt in KR.fixture_batches(spec, shuffled):
            a = KR.check(ctx, name, bt, "dev_np")
            if not shuffled:
                b = KR.check(ctx, name, bt, "host")
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
                KR.check_recover_agrees(ctx, name, bt)
                if name in ("secp256k1", "p256", "p384") and bt.h.shape[1] == spec["B"]:
                    KR.check_verify_agrees(ctx, name, bt)


@pytest.mark.parametrize("name", KR.PRESETS)
def test_batch_meets_the_conditions(batches, name):
    assert KR.meets_conditions(batches[name])


@pytest.mark.parametrize("name", KR.PRESETS)
def test_random_batch_matches_model(ctx, batches, name):
    bt = batches[name]
    for n in (1, 2, 65, 257):
        for mem in ("host", "dev_np") if n < 257 else ("dev_np",):
            KR.check(ctx, name, bt.first(n), mem)
    KR.check_recover_agrees(ctx, name, bt.first(65))
    if name in ("secp256k1", "p256", "p384"):
        KR.check_verify_agrees(ctx, name, bt.first(65))


@pytest.mark.parametrize("name", ["secp256k1", "p224"])
def test_status_3_rows_poison_no_neighbour(ctx, batches, name):
    KR.check_no_poison(ctx, name, batches[name].first(65), "dev_np")


def test_three_items_per_inversion():
    """a fresh process with ELLGPU_PREP_K=3 ELLGPU_NORM_K=3: groups of three with a status-3 item
    first, in the middle and last"""
    KR.run_child(["dev_np", 65, "secp256k1", "p256", "p192"], KR.K3_ENV, lib_path=build_hostsim())


def test_sharded_over_a_group(hs, batches):
    g = elliptic_amd.Context(lib_path=hs, devices=[0, 0])
    try:
        bt = batches["p192"]
        for n in (1, 2, 65):
            KR.check(g, "p192", bt.first(n), "host")
        assert hs.ellgpu_ecdsa_recid(g._ctx, 1, 0, None, 24, None, None, None, None, None, 0, None) == E_ARG
    finally:
        g.close()


def test_refusals(hs, batches):
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        P = lambda a: a.ctypes.data  # noqa: E731
        bt = batches["p256"].first(4)
        rec, st = np.full(4, KR.FILL, np.uint8), np.full(4, KR.FILL, np.uint8)
        call = lambda curve, n, *a: hs.ellgpu_ecdsa_recid(c._ctx, curve, n, *a)  # noqa: E731
        good = (P(bt.h), 32, P(bt.r), P(bt.s), P(bt.pub), P(rec), P(st))
        assert call(3, 4, *good, 0, None) == 0 and (rec == bt.recid).all() and (st == bt.status).all()
        # curves the rule is not proved for: Edwards, Montgomery, every user-defined id
        for curve in (6, 7):
            for mem in (0, 1):
                assert call(curve, 4, *good, mem, None) == E_UNSUPPORTED
        s192 = VB.spec_of("secp192k1")
        plain = c.define_short(VB.I(s192["p"]), VB.I(s192["a"]), VB.I(s192["b"]))
        dom = VB.curve_id(c, VB.spec_of("brainpoolP256r1"))
        for curve in (plain, dom):
            for mem in (0, 1):
                assert call(curve, 4, *good, mem, None) == E_UNSUPPORTED and b"user-defined" in hs.ellgpu_last_error()
            assert call(curve, 0, *good, 0, None) == E_UNSUPPORTED
        with pytest.raises(_lib.EllgpuError) as e:
            c.ecdsa_recid(dom, bt.h, bt.r, bt.s, bt.pub)
        assert e.value.code == E_UNSUPPORTED
        # an unknown id, a user-defined id that was never defined
        for curve in (-1, 8, 15, 31, 32, 99):
            assert call(curve, 4, *good, 0, None) == E_ARG and b"unknown curve id" in hs.ellgpu_last_error()
        # null pointers, either memory kind; out_status may not be NULL whatever n is
        for mem in (0, 1):
            for miss in (0, 2, 3, 4, 5, 6):
                args = list(good)
                args[miss] = None
                assert call(3, 4, *args, mem, None) == E_ARG, (mem, miss)
            assert call(3, 0, *good[:6], None, mem, None) == E_ARG
            assert hs.ellgpu_ecdsa_recid(None, 3, 4, *good, mem, None) == E_ARG
        # mem, and a stream with host memory
        for mem in (-1, 2, 7):
            assert call(3, 4, *good, mem, None) == E_ARG
        stream = ctypes.c_void_p(hs.ellgpu_ctx_stream(c._ctx) or 1)
        assert call(3, 4, *good, 0, stream) == E_ARG
        # hash_len: 1 .. twice the order width, as in ellgpu_ecdsa_recover
        wide = np.zeros((4, 72), np.uint8)
        for mem in (0, 1):
            assert call(3, 4, P(wide), 64, *good[2:], mem, None) == 0
            assert call(3, 4, P(wide), 65, *good[2:], mem, None) == E_ARG and b"hash_len" in hs.ellgpu_last_error()
            assert call(3, 4, P(wide), 0, *good[2:], mem, None) == E_ARG
        # overlap of an operand and a result, and of the results (device memory)
        buf = np.zeros(4 * 64 + 8, np.uint8)
        for which in (0, 2, 3, 4):
            for res in (5, 6):
                args = list(good)
                args[which] = P(buf)
                args[res] = P(buf) + 4 * (64 if which == 4 else 32) - 1
                assert call(3, 4, *args, 1, None) == E_ARG and b"overlap" in hs.ellgpu_last_error()
                args[res] = P(buf) + 4 * 64
                assert call(3, 4, *args, 1, None) == 0
        args = list(good)
        args[5], args[6] = P(buf), P(buf) + 3
        assert call(3, 4, *args, 1, None) == E_ARG and b"overlap" in hs.ellgpu_last_error()
        # n == 0: nothing is touched
        rec[:] = KR.FILL
        st[:] = KR.FILL
        for mem in (0, 1):
            assert call(3, 0, *good, mem, None) == 0
            assert call(3, 0, None, 32, None, None, None, None, P(st), mem, None) == 0
        assert (rec == KR.FILL).all() and (st == KR.FILL).all()
    finally:
        c.close()


def test_python_argument_checks(ctx, batches):
    bt = batches["p224"].first(3)
    with pytest.raises(ValueError):
        ctx.ecdsa_recid("p224", bt.h, bt.r[:, :27], bt.s, bt.pub)
    with pytest.raises(ValueError):
        ctx.ecdsa_recid("p224", bt.h.reshape(-1), bt.r, bt.s, bt.pub)
    with pytest.raises(AssertionError):
        ctx.ecdsa_recid("p224", bt.h, bt.r, bt.s, bt.pub, out=(np.zeros(2, np.uint8), np.zeros(3, np.uint8)))
    rec, st = ctx.ecdsa_recid("p224", bt.h, bt.r, bt.s, bt.pub)
    assert rec.dtype == st.dtype == np.uint8 and rec.shape == st.shape == (3,)
    assert (rec == bt.recid).all() and (st == bt.status).all()


def test_kernel_launches(hs, ctx, batches):
    """the call is recid_prep, the kernels of k1 G + k2 P at this n, and recid_finish: no square root"""
    if not hasattr(hs, "hs_launches"):
        pytest.skip("this hostsim build does not count launches")
    hs.hs_launches.restype = ctypes.c_long
    hs.hs_launches.argtypes = [ctypes.c_char_p]
    names = [b"recid_prep", b"recid_finish", b"decompress", b"recover_prep", b"ecdsa_prep"]
    bt = batches["p256"].first(41)
    KR.check(ctx, "p256", bt, "dev_np")
    before = [hs.hs_launches(nm) for nm in names]
    KR.check(ctx, "p256", bt, "dev_np")
    d = [hs.hs_launches(nm) - b for nm, b in zip(names, before)]
    assert d == [1, 1, 0, 0, 0], d
