"""Sums of many k * P terms on Edwards curves (ellgpu_ed_mul_sum) on the CPU: the hostsim build of
the device code (tests/hostsim) against the reference's recorded answers
(tests/golden/ed_mul_sum.json) and against the Python-integer model of tests/ed_mul_sum_checks.py on
ed25519 and three user-defined Edwards ids, with a context whose slices hold 48 pairs, the
cross-checks through ellgpu_mul_add2 and ellgpu_mul_var, every refusal and a device group."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import ed_mul_sum_checks as ES  # noqa: E402

E_ARG, E_UNSUPPORTED = -2, -5
SHAPES = [(1, 257), (65, 33), (259, 2)]
ED25519, CURVE25519 = 6, 7


@pytest.fixture(scope="module")
def hs():
    return _lib.load(build_hostsim(), optional=ES.OPTIONAL)


@pytest.fixture(scope="module")
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx48(hs):
    """a second context, created under ELLGPU_SUM_SLICE=48 (the override is read when a context is
    created): at most 48 pairs per launch, longer sums are walked in slices"""
    os.environ["ELLGPU_SUM_SLICE"] = "48"
    try:
        c = elliptic_amd.Context(0, lib_path=hs)
    finally:
        del os.environ["ELLGPU_SUM_SLICE"]
    yield c
    c.close()


@pytest.fixture(scope="module")
def cids(ctx):
    return {name: ES.curve_id(ctx, name) for name in ES.NAMES}


@pytest.fixture(scope="module")
def cids48(ctx48):
    return {name: ES.curve_id(ctx48, name) for name in ES.NAMES}


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_curve_set():
    assert [c["name"] for c in ES.curves()] == ES.NAMES
    kinds = [c["kind"] for c in ES.curves()]
    assert kinds[0] == "preset" and "plain" in kinds and "domain" in kinds
    for name in ES.NAMES:
        ES.check_fixture_shape(ES.spec_of(name))


@pytest.mark.parametrize("name", ES.NAMES)
def test_model_is_pinned_to_the_fixture(name):
    ES.check_model_pinned(ES.spec_of(name))


@pytest.mark.parametrize("name", ES.NAMES)
def test_golden(ctx, cids, name):
    """every recorded row, in fixture order and shuffled, one batch per m, through both memory kinds:
    the reference's answers, status 2 for the sums with a term off the curve, identical bytes"""
    for shuffled in (False, True):
        for bt in ES.fixture_batches(name, shuffled):
            assert _same(ES.check(ctx, cids[name], bt, "dev_np"), ES.check(ctx, cids[name], bt, "host"))


@pytest.mark.parametrize("name", ES.NAMES)
def test_shapes_match_model(ctx, cids, name):
    for n, m in SHAPES:
        bt = ES.pool_batch(name, n, m)
        assert _same(ES.check(ctx, cids[name], bt, "dev_np"), ES.check(ctx, cids[name], bt, "host"))


@pytest.mark.parametrize("name", ES.NAMES)
def test_slices_of_48_pairs(ctx, cids, ctx48, cids48, name):
    """(2, 257): 129 pairs per sum, two slices of 48 and one of 33 whose last pair is a lone term;
    (3, 33): 17 pairs, groups of two sums and one; (5, 96): 48 pairs, a group of one sum per chunk.
    The bytes are those of the context without the override."""
    for n, m in ((2, 257), (3, 33), (5, 96)):
        bt = ES.pool_batch(name, n, m, seed=3)
        a = ES.check(ctx48, cids48[name], bt, "dev_np")
        assert _same(a, ES.check(ctx48, cids48[name], bt, "host"))
        assert _same(a, ES.check(ctx, cids[name], bt, "dev_np"))
    # a term off the curve in the last slice (the lone last term) of the second sum, and in a middle one of the first
    bt = ES.pool_batch(name, 2, 257, seed=3)
    marked = ES.with_off_curve(name, bt, [(1, 256)])
    got = ES.check(ctx48, cids48[name], marked, "dev_np")
    assert got[1][1] == 2 and got[0][0].tobytes() == bt.want_xy[0].tobytes()
    marked = ES.with_off_curve(name, bt, [(0, 100)])
    assert _same(ES.check(ctx48, cids48[name], marked, "dev_np"), ES.check(ctx48, cids48[name], marked, "host"))


def test_slice_launches(hs, ctx, ctx48):
    """the kernels of one sum of 257 terms on ed25519: whole, the pair kernel once and ceil(log2 129)
    = 8 halving steps; in slices of 48 pairs, three pair launches, 6 + 6 + 6 steps for the slices of
    48, 48 and 33 pairs and two more over the three partial sums"""
    if not hasattr(hs, "hs_launches"):
        pytest.skip("this hostsim build does not count launches")
    hs.hs_launches.restype = ctypes.c_long
    hs.hs_launches.argtypes = [ctypes.c_char_p]
    names = [b"ed_sum_pairs", b"ed_sum_fold", b"ed_normalize", b"ed_sum_mark", b"ed_mul_add2"]
    bt = ES.pool_batch("ed25519", 1, 257)
    for c, want in ((ctx, [1, 8, 1, 1, 0]), (ctx48, [3, 6 + 6 + 6 + 2, 1, 1, 0])):
        before = [hs.hs_launches(nm) for nm in names]
        ES.check(c, "ed25519", bt, "dev_np")
        assert [hs.hs_launches(nm) - b for nm, b in zip(names, before)] == want


@pytest.mark.parametrize("name", ES.NAMES)
def test_off_curve_terms(ctx, cids, name):
    """a term off the curve in the first sum's first pair, in a middle sum and as the lone last term
    of the last sum is status 2 with zeroed bytes; every other sum's bytes are unchanged"""
    bt = ES.pool_batch(name, 65, 33)
    places = [(0, 0), (7, 16), (64, 32)]
    marked = ES.with_off_curve(name, bt, places)
    hit = [j for j, _ in places]
    keep = [j for j in range(65) if j not in hit]
    assert list(marked.want_inf[hit]) == [2, 2, 2] and (marked.want_inf[keep] != 2).all()
    clean = ES.check(ctx, cids[name], bt, "dev_np")
    got = ES.check(ctx, cids[name], marked, "dev_np")
    assert _same(got, ES.check(ctx, cids[name], marked, "host"))
    assert got[0][keep].tobytes() == clean[0][keep].tobytes() and got[1][keep].tobytes() == clean[1][keep].tobytes()
    assert not got[0][hit].any()


@pytest.mark.parametrize("name", ES.NAMES)
def test_two_terms_are_mul_add2_and_one_is_mul_var(ctx, cids, name):
    """byte for byte, out_inf included; the golden rows of two terms and of one (identities, torsion
    and wide coordinates among them) go the same way"""
    pairs = [ES.pool_batch(name, 259, 2)] + [bt for bt in ES.fixture_batches(name) if bt.m == 2]
    for bt in pairs:
        xy, inf = ES.run(ctx, cids[name], bt, "dev_np")
        k1, p1, k2, p2 = (np.ascontiguousarray(a) for a in (bt.k[:, 0], bt.xy[:, 0], bt.k[:, 1], bt.xy[:, 1]))
        xy2, inf2 = ctx.mul_add2(cids[name], k1, p1, k2, p2)
        assert xy2.tobytes() == xy.tobytes() and inf2.tobytes() == inf.tobytes()
    ones = [ES.pool_batch(name, 65, 1)] + [bt for bt in ES.fixture_batches(name) if bt.m == 1]
    for bt in ones:
        xy, inf = ES.run(ctx, cids[name], bt, "dev_np")
        xy1, inf1 = ctx.mul_var(cids[name], np.ascontiguousarray(bt.k[:, 0]), np.ascontiguousarray(bt.xy[:, 0]))
        assert xy1.tobytes() == xy.tobytes() and inf1.tobytes() == inf.tobytes()


def test_a_domain_id_is_its_plain_id(ctx):
    spec = ES.spec_of("curve1174")
    assert spec["kind"] == "domain"
    plain = ctx.define_edwards(ES.I(spec["p"]), ES.I(spec["a"]), ES.I(spec["d"]))
    dom = ES.curve_id(ctx, "curve1174")
    assert plain != dom
    for bt in ES.fixture_batches("curve1174")[:4] + [ES.pool_batch("curve1174", 65, 33)]:
        assert _same(ES.check(ctx, plain, bt, "dev_np"), ES.check(ctx, dom, bt, "dev_np"))


def test_sharded_over_a_group(hs, ctx):
    g = elliptic_amd.Context(lib_path=hs, devices=[0, 0])
    try:
        assert hs.ellgpu_group_size(g._ctx) == 2
        for name in ("ed25519", "e222"):
            gid = ES.curve_id(g, name)
            for n, m in ((1, 5), (2, 3), (65, 33)):          # fewer sums than members: the first member
                bt = ES.pool_batch(name, n, m)
                assert _same(ES.check(g, gid, bt, "host"), ES.check(ctx, ES.curve_id(ctx, name), bt, "host"))
        assert hs.ellgpu_ed_mul_sum(g._ctx, ED25519, 4, 0, None, None, None, None, 0, None) == E_ARG
    finally:
        g.close()


def test_refusals(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    try:
        P = lambda a: a.ctypes.data  # noqa: E731
        bt = ES.pool_batch("ed25519", 4, 3)
        oxy, inf = np.full((4, 64), ES.FILL, np.uint8), np.full(4, ES.FILL, np.uint8)
        call = lambda curve, n, m, *a: hs.ellgpu_ed_mul_sum(c._ctx, curve, n, m, *a)  # noqa: E731
        good = (P(bt.k), P(bt.xy), P(oxy), P(inf))
        assert call(ED25519, 4, 3, *good, 0, None) == 0 and (oxy == bt.want_xy).all() and (inf == bt.want_inf).all()
        # the short curves, presets and user-defined, plain and domain: ellgpu_mul_sum's
        short = c.define_short(0xfffffffffffffffffffffffffffffffffffffffeffffee37, 0, 3)          # secp192k1
        for curve in (0, 1, 2, 3, 4, 5, short):
            for mem in (0, 1):
                for n in (4, 0):
                    assert call(curve, n, 3, *good, mem, None) == E_UNSUPPORTED
                    assert b"ellgpu_mul_sum" in hs.ellgpu_last_error()
        with pytest.raises(_lib.EllgpuError) as e:
            c.ed_mul_sum("p256", bt.k, bt.xy)
        assert e.value.code == E_UNSUPPORTED and "ellgpu_mul_sum" in str(e.value)
        # Montgomery curves
        mont = c.define_mont(2 ** 255 - 19, 486662)
        for curve in (CURVE25519, mont):
            for mem in (0, 1):
                for n in (4, 0):
                    assert call(curve, n, 3, *good, mem, None) == E_UNSUPPORTED
                    assert b"Not supported on Montgomery curve" in hs.ellgpu_last_error()
        # ... and ellgpu_mul_sum still refuses the Edwards ids, with its message
        ed = c.define_edwards(2 ** 251 - 9, 1, -1174)
        for curve in (ED25519, ed):
            assert hs.ellgpu_mul_sum(c._ctx, curve, 4, 3, *good, 0, None) == E_UNSUPPORTED
            assert b"Edwards curves are a later change" in hs.ellgpu_last_error()
        assert call(ed, 4, 3, *good, 0, None) == 0
        # an unknown id, a user-defined id that was never defined
        for curve in (-1, 8, 15, 31, 32, 99):
            assert call(curve, 4, 3, *good, 0, None) == E_ARG and b"unknown curve id" in hs.ellgpu_last_error()
        # m == 0, whatever n is
        for mem in (0, 1):
            for n in (0, 4):
                assert call(ED25519, n, 0, *good, mem, None) == E_ARG and b"m must be" in hs.ellgpu_last_error()
        # null pointers with n > 0, either memory kind; a null context
        for mem in (0, 1):
            for miss in range(4):
                args = list(good)
                args[miss] = None
                assert call(ED25519, 4, 3, *args, mem, None) == E_ARG, (mem, miss)
            assert hs.ellgpu_ed_mul_sum(None, ED25519, 4, 3, *good, mem, None) == E_ARG
        # mem, and a stream with host memory
        for mem in (-1, 2, 7):
            assert call(ED25519, 4, 3, *good, mem, None) == E_ARG
        stream = ctypes.c_void_p(hs.ellgpu_ctx_stream(c._ctx) or 1)
        assert call(ED25519, 4, 3, *good, 0, stream) == E_ARG
        # n m, or n m 64, does not fit size_t
        top = ctypes.c_size_t(-1).value
        for n, m in ((top, 2), (2, top), (top // 2 + 1, 2), (1 << 40, 1 << 40), (top // 64 + 1, 1), (1, top // 64 + 1)):
            for mem in (0, 1):
                assert call(ED25519, n, m, *good, mem, None) == E_ARG and b"size_t" in hs.ellgpu_last_error(), (n, m)
        # overlap of an operand and a result, and of the results (device memory)
        buf = np.zeros(4 * 3 * 64 + 4 * 64 + 8, np.uint8)
        for which, nbytes in ((0, 4 * 3 * 32), (1, 4 * 3 * 64)):
            for res in (2, 3):
                args = list(good)
                args[which] = P(buf)
                args[res] = P(buf) + nbytes - 1
                assert call(ED25519, 4, 3, *args, 1, None) == E_ARG and b"overlap" in hs.ellgpu_last_error()
        args = list(good)
        args[2], args[3] = P(buf), P(buf) + 4 * 64 - 1
        assert call(ED25519, 4, 3, *args, 1, None) == E_ARG and b"overlap" in hs.ellgpu_last_error()
        args[3] = P(buf) + 4 * 64
        assert call(ED25519, 4, 3, *args, 1, None) == 0 and (buf[:4 * 64].reshape(4, 64) == bt.want_xy).all()
        # n == 0: success, nothing is touched
        oxy[:] = ES.FILL
        inf[:] = ES.FILL
        for mem in (0, 1):
            assert call(ED25519, 0, 3, *good, mem, None) == 0
            assert call(ED25519, 0, 3, None, None, None, None, mem, None) == 0
        assert (oxy == ES.FILL).all() and (inf == ES.FILL).all()
    finally:
        c.close()


def test_python_argument_checks(ctx):
    bt = ES.pool_batch("ed25519", 3, 2)
    with pytest.raises(ValueError):
        ctx.ed_mul_sum("ed25519", bt.k.reshape(6, 32), bt.xy)
    with pytest.raises(ValueError):
        ctx.ed_mul_sum("ed25519", bt.k, bt.xy[:, :1])
    with pytest.raises(ValueError):
        ctx.ed_mul_sum("ed25519", bt.k[:, :, :31], bt.xy)
    with pytest.raises(AssertionError):
        ctx.ed_mul_sum("ed25519", bt.k, bt.xy, out=(np.zeros((3, 64), np.uint8), np.zeros(2, np.uint8)))
    xy, inf = ctx.ed_mul_sum("ed25519", bt.k, bt.xy)
    assert xy.dtype == inf.dtype == np.uint8 and xy.shape == (3, 64) and inf.shape == (3,)
    assert (xy == bt.want_xy).all() and (inf == bt.want_inf).all()
    xy, inf = ctx.ed_mul_sum(ED25519, bt.k, bt.xy)                         # the preset by its integer id
    assert (xy == bt.want_xy).all() and (inf == bt.want_inf).all()
