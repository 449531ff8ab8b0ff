"""Sums of many k * P terms (ellgpu_mul_sum) on the CPU: the hostsim build of the device code
(tests/hostsim) against the reference's recorded answers (tests/golden/mul_sum.json) and against the
Python-integer model of tests/mul_sum_checks.py, with the cross-checks through ellgpu_mul_var +
ellgpu_point_add and ellgpu_mul_add2, a context whose slices hold three pairs, every refusal, and the
call issued alone and behind another device-memory call."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import mul_sum_checks as MS  # noqa: E402

E_ARG, E_UNSUPPORTED = -2, -5
SHAPES = [(n, m) for n in (1, 2, 65) for m in (1, 2, 3, 5, 8, 33)]


@pytest.fixture(scope="module")
def hs():
    return _lib.load(build_hostsim(), optional=MS.OPTIONAL)


@pytest.fixture(scope="module")
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx3(hs):
    """a second context, created under ELLGPU_SUM_SLICE=3 (the override is read when a context is
    created): at most three pairs per launch, longer sums are walked in slices"""
    os.environ["ELLGPU_SUM_SLICE"] = "3"
    try:
        c = elliptic_amd.Context(0, lib_path=hs)
    finally:
        del os.environ["ELLGPU_SUM_SLICE"]
    yield c
    c.close()


@pytest.fixture(scope="module")
def cids(ctx):
    return {name: MS.curve_id(ctx, name) for name in MS.NAMES}


def test_curve_set():
    assert [c["name"] for c in MS.curves()] == MS.NAMES
    for name in MS.NAMES:
        MS.check_fixture_shape(MS.spec_of(name))


@pytest.mark.parametrize("name", MS.NAMES)
def test_model_is_pinned_to_the_fixture(name):
    MS.check_model_pinned(MS.spec_of(name))


@pytest.mark.parametrize("name", MS.NAMES)
def test_golden(ctx, cids, name):
    """every recorded row, in fixture order and shuffled, through both memory kinds: the reference's
    answers, status 2 for the sums with a term off the curve, identical bytes"""
    for shuffled in (False, True):
        for bt in MS.fixture_batches(name, shuffled):
            a = MS.check(ctx, cids[name], bt, "dev_np")
            b = MS.check(ctx, cids[name], bt, "host")
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("name", MS.NAMES)
def test_shapes_match_model(ctx, cids, name):
    for n, m in SHAPES:
        bt = MS.pool_batch(name, n, m)
        MS.check(ctx, cids[name], bt, "dev_np")
        if n < 65 or m <= 3:
            MS.check(ctx, cids[name], bt, "host")


@pytest.mark.parametrize("name", ["secp256k1", "p224", "p521", "secp192k1"])
def test_agrees_with_mul_var_and_point_add(ctx, cids, name):
    """the same operands through ellgpu_mul_var per term and ellgpu_point_add in order"""
    bt = MS.pool_batch(name, 9, 5)
    xy, inf = MS.check(ctx, cids[name], bt, "host")
    B = xy.shape[1] // 2
    pr, pinf = ctx.mul_var(cids[name], bt.k.reshape(-1, B), bt.xy.reshape(-1, 2 * B))
    pr, pinf = pr.reshape(bt.n, bt.m, 2 * B), pinf.reshape(bt.n, bt.m)
    acc, ainf = pr[:, 0].copy(), pinf[:, 0].copy()
    for i in range(1, bt.m):
        acc, ainf = ctx.point_add(cids[name], acc, pr[:, i], ainf, pinf[:, i])
    assert acc.tobytes() == xy.tobytes() and ainf.tobytes() == inf.tobytes()


@pytest.mark.parametrize("name", MS.NAMES)
def test_two_terms_are_mul_add2(ctx, cids, name):
    bt = MS.pool_batch(name, 65, 2)
    xy, inf = MS.check(ctx, cids[name], bt, "dev_np")
    xy2, inf2 = ctx.mul_add2(cids[name], bt.k[:, 0], bt.xy[:, 0], bt.k[:, 1], bt.xy[:, 1])
    assert xy2.tobytes() == xy.tobytes() and inf2.tobytes() == inf.tobytes()


@pytest.mark.parametrize("name", ["secp256k1", "p256", "p384", "brainpoolP256r1"])
def test_slices_of_three_pairs(ctx, ctx3, name):
    """m = 6: three pairs, a group of one sum per chunk; 7: a last slice of one pair that is a lone
    term; 13: slices that divide with a last slice of one lone term; 33: five slices and a last one of
    two pairs, the second a lone term.  The bytes are those of the context without the override."""
    cid3 = MS.curve_id(ctx3, name)
    cid = MS.curve_id(ctx, name)
    for m in (6, 7, 13, 33):
        for n in (1, 3):
            bt = MS.pool_batch(name, n, m, seed=3)
            a = MS.check(ctx3, cid3, bt, "dev_np")
            b = MS.check(ctx3, cid3, bt, "host")
            c = MS.check(ctx, cid, bt, "dev_np")
            assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1].tobytes() == b[1].tobytes() == c[1].tobytes()
    for bt in MS.fixture_batches(name):
        MS.check(ctx3, cid3, bt, "dev_np")


def test_slice_launches(hs, ctx, ctx3):
    """the kernels of one sum of 33 terms: whole, sum_pairs once and ceil(log2 17) = 5 halving steps;
    in slices of three pairs, six sum_pairs, two steps for each of the five slices of three pairs, one
    for the last slice's two, and three more over the six partial sums"""
    if not hasattr(hs, "hs_launches"):
        pytest.skip("this hostsim build does not count launches")
    hs.hs_launches.restype = ctypes.c_long
    hs.hs_launches.argtypes = [ctypes.c_char_p]
    names = [b"sum_pairs", b"sum_fold", b"normalize", b"sum_mark", b"mul_add2"]
    bt = MS.pool_batch("p256", 1, 33, seed=3)
    for c, want in ((ctx, [1, 5, 1, 1, 0]), (ctx3, [6, 5 * 2 + 1 + 3, 1, 1, 0])):
        before = [hs.hs_launches(nm) for nm in names]
        MS.check(c, "p256", bt, "dev_np")
        assert [hs.hs_launches(nm) - b for nm, b in zip(names, before)] == want
    # m = 2 and m = 1: the ladder and a copy step
    for m in (1, 2):
        before = [hs.hs_launches(nm) for nm in names]
        MS.check(ctx, "p256", MS.pool_batch("p256", 65, m), "dev_np")
        assert [hs.hs_launches(nm) - b for nm, b in zip(names, before)] == [1, 1, 1, 1, 0]


@pytest.mark.parametrize("name", ["secp256k1", "p192", "secp192k1"])
def test_off_curve_terms_in_any_slice(ctx, ctx3, name):
    """a term off the curve in the first, a middle and the last slice (and as the lone last term) is
    status 2 with zeroed bytes; its neighbours in the batch are undisturbed"""
    bt = MS.pool_batch(name, 7, 13, seed=5)
    marked = MS.with_off_curve(name, bt, [(1, 0), (3, 7), (5, 12)])
    assert list(marked.want_inf[[1, 3, 5]]) == [2, 2, 2] and (marked.want_inf[[0, 2, 4, 6]] != 2).all()
    for c in (ctx, ctx3):
        cid = MS.curve_id(c, name)
        clean = MS.check(c, cid, bt, "dev_np")
        got = MS.check(c, cid, marked, "dev_np")
        MS.check(c, cid, marked, "host")
        keep = [0, 2, 4, 6]
        assert got[0][keep].tobytes() == clean[0][keep].tobytes() and got[1][keep].tobytes() == clean[1][keep].tobytes()
        assert not got[0][[1, 3, 5]].any()


def test_sharded_over_a_group(hs):
    g = elliptic_amd.Context(lib_path=hs, devices=[0, 0, 0])
    try:
        for n, m in ((1, 5), (2, 3), (3, 2), (65, 3)):          # fewer sums than members: the first member
            MS.check(g, "p192", MS.pool_batch("p192", n, m), "host")
        assert hs.ellgpu_mul_sum(g._ctx, 1, 4, 0, None, None, None, None, 0, None) == E_ARG
    finally:
        g.close()


def test_refusals(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        P = lambda a: a.ctypes.data  # noqa: E731
        bt = MS.pool_batch("p256", 4, 3)
        oxy, inf = np.full((4, 64), MS.FILL, np.uint8), np.full(4, MS.FILL, np.uint8)
        call = lambda curve, n, m, *a: hs.ellgpu_mul_sum(c._ctx, curve, n, m, *a)  # noqa: E731
        good = (P(bt.k), P(bt.xy), P(oxy), P(inf))
        assert call(3, 4, 3, *good, 0, None) == 0 and (oxy == bt.want_xy).all() and (inf == bt.want_inf).all()
        # Edwards and Montgomery curves, presets and user-defined
        ed = c.define_edwards(2 ** 251 - 9, 1, -1174)                   # curve1174
        mont = c.define_mont(2 ** 255 - 19, 486662)
        for curve in (6, 7, ed, mont):
            for mem in (0, 1):
                for n in (4, 0):
                    assert call(curve, n, 3, *good, mem, None) == E_UNSUPPORTED
        assert call(6, 4, 3, *good, 0, None) == E_UNSUPPORTED and b"Edwards curves are a later change" in hs.ellgpu_last_error()
        with pytest.raises(_lib.EllgpuError) as e:
            c.mul_sum("ed25519", bt.k, bt.xy)
        assert e.value.code == E_UNSUPPORTED
        # an unknown id, a user-defined id that was never defined
        for curve in (-1, 8, 15, 18, 31, 32, 99):
            assert call(curve, 4, 3, *good, 0, None) == E_ARG and b"unknown curve id" in hs.ellgpu_last_error()
        # m == 0, whatever n is
        for mem in (0, 1):
            for n in (0, 4):
                assert call(3, n, 0, *good, mem, None) == E_ARG and b"m must be" in hs.ellgpu_last_error()
        # null pointers with n > 0, either memory kind; a null context
        for mem in (0, 1):
            for miss in range(4):
                args = list(good)
                args[miss] = None
                assert call(3, 4, 3, *args, mem, None) == E_ARG, (mem, miss)
            assert hs.ellgpu_mul_sum(None, 3, 4, 3, *good, mem, None) == E_ARG
        # mem, and a stream with host memory
        for mem in (-1, 2, 7):
            assert call(3, 4, 3, *good, mem, None) == E_ARG
        stream = ctypes.c_void_p(hs.ellgpu_ctx_stream(c._ctx) or 1)
        assert call(3, 4, 3, *good, 0, stream) == E_ARG
        # n m, or n m 2 B, does not fit size_t
        top = ctypes.c_size_t(-1).value
        for n, m in ((top, 2), (2, top), (top // 2 + 1, 2), (1 << 40, 1 << 40), (top // 64 + 1, 1), (1, top // 64 + 1)):
            for mem in (0, 1):
                assert call(3, n, m, *good, mem, None) == E_ARG and b"size_t" in hs.ellgpu_last_error(), (n, m)
        # overlap of an operand and a result, and of the results (device memory)
        buf = np.zeros(4 * 3 * 64 + 4 * 64 + 8, np.uint8)
        for which, nbytes in ((0, 4 * 3 * 32), (1, 4 * 3 * 64)):
            for res in (2, 3):
                args = list(good)
                args[which] = P(buf)
                args[res] = P(buf) + nbytes - 1
                assert call(3, 4, 3, *args, 1, None) == E_ARG and b"overlap" in hs.ellgpu_last_error()
        args = list(good)
        args[2], args[3] = P(buf), P(buf) + 4 * 64 - 1
        assert call(3, 4, 3, *args, 1, None) == E_ARG and b"overlap" in hs.ellgpu_last_error()
        args[3] = P(buf) + 4 * 64
        assert call(3, 4, 3, *args, 1, None) == 0 and (buf[:4 * 64].reshape(4, 64) == bt.want_xy).all()
        # n == 0: success, nothing is touched
        oxy[:] = MS.FILL
        inf[:] = MS.FILL
        for mem in (0, 1):
            assert call(3, 0, 3, *good, mem, None) == 0
            assert call(3, 0, 3, None, None, None, None, mem, None) == 0
        assert (oxy == MS.FILL).all() and (inf == MS.FILL).all()
    finally:
        c.close()


def test_python_argument_checks(ctx):
    bt = MS.pool_batch("p224", 3, 2)
    with pytest.raises(ValueError):
        ctx.mul_sum("p224", bt.k.reshape(6, 28), bt.xy)
    with pytest.raises(ValueError):
        ctx.mul_sum("p224", bt.k, bt.xy[:, :1])
    with pytest.raises(ValueError):
        ctx.mul_sum("p224", bt.k[:, :, :27], bt.xy)
    with pytest.raises(AssertionError):
        ctx.mul_sum("p224", bt.k, bt.xy, out=(np.zeros((3, 56), np.uint8), np.zeros(2, np.uint8)))
    xy, inf = ctx.mul_sum("p224", bt.k, bt.xy)
    assert xy.dtype == inf.dtype == np.uint8 and xy.shape == (3, 56) and inf.shape == (3,)
    assert (xy == bt.want_xy).all() and (inf == bt.want_inf).all()
    xy, inf = ctx.mul_sum(2, bt.k, bt.xy)                               # a preset by its integer id
    assert (xy == bt.want_xy).all() and (inf == bt.want_inf).all()


def test_alone_and_behind_another_device_call(ctx):
    """the call is kept from the stream schedules of tests/dev_stream_checks.py by its fixture's name:
    here the same operands issued alone, and again after another device-memory call on the same
    context (which leaves its own bytes in the shared scratch), give the same bytes"""
    for name in ("secp256k1", "p256"):
        bt = MS.pool_batch(name, 65, 5)
        alone = MS.check(ctx, name, bt, "dev_np")
        B = bt.want_xy.shape[1] // 2
        P = lambda a: a.ctypes.data  # noqa: E731
        k1, p1, k2, p2 = (np.ascontiguousarray(a) for a in (bt.k[:, 0], bt.xy[:, 0], bt.k[:, 1], bt.xy[:, 1]))
        o1, o2 = np.zeros((65, 2 * B), np.uint8), np.zeros(65, np.uint8)
        lib, cid = ctx._lib, ctx._cid(name)
        assert lib.ellgpu_mul_var_dev(ctx._ctx, cid, 65, P(k1), P(p1), P(o1), P(o2), None) == 0
        assert lib.ellgpu_mul_add2_dev(ctx._ctx, cid, 65, P(k1), P(p1), P(k2), P(p2), P(o1), P(o2), None) == 0
        again = MS.check(ctx, name, bt, "dev_np")
        assert alone[0].tobytes() == again[0].tobytes() and alone[1].tobytes() == again[1].tobytes()
