"""secp256k1's GLV split with both halves odd and below 2^128 (csrc/ladder.h: glv_split's ROT form),
which lets the full-grid ladder run 32 four-bit windows.  The integer model (glv_split_vectors.py)
pins the bound; the CPU build of the device headers (tests/hostsim) must then compute P*k and
EC#verify as the C oracle does on the scalars where the split is at its edges."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402
import glv_split_vectors as GV  # noqa: E402


def test_lattice_constants():
    """the constants the proof argues over: the basis, its determinant, lambda, beta, the multipliers"""
    assert (GV.LAMBDA * GV.LAMBDA + GV.LAMBDA + 1) % GV.N == 0 and pow(GV.BETA, 3, GV.P) == 1 and GV.BETA != 1
    assert (GV.A1 - GV.MB1 * GV.LAMBDA) % GV.N == 0 and (GV.A2 + GV.B2 * GV.LAMBDA) % GV.N == 0
    assert GV.A1 * GV.B2 + GV.A2 * GV.MB1 == GV.N
    assert (GV.A1 & 1, GV.MB1 & 1, GV.A2 & 1, GV.B2 & 1) == (1, 1, 0, 1)
    from oracle import ec_oracle as O
    cur = O.get_curve("secp256k1")
    assert int(cur.n) == GV.N and int(cur.p) == GV.P
    words = lambda v, n: [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]       # noqa: E731
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "curve_consts.h")).read()
    for name, v, n in (("glv_g1", GV.G1, 8), ("glv_g2", GV.G2, 8), ("glv_a1", GV.A1, 4), ("glv_mb1", GV.MB1, 4),
                       ("glv_a2", GV.A2, 5), ("glv_b2", GV.B2, 4), ("beta", GV.BETA, 8), ("lambda", GV.LAMBDA, 8)):
        line = "%s[%d] = {%s};" % (name, n, ", ".join("0x%08Xu" % w for w in words(v, n)))
        assert line in src, name


def test_bound_of_the_proof():
    """the inequalities of the comment above glv_split, in exact integers: with |t_i| <= 1/2 + 2^-129
    every component of the reduced pair, of its two rotations and of the (even, even) translate is
    below 2^128"""
    from fractions import Fraction as Fr
    h = Fr(1, 2) + Fr(1, 2 ** 129)
    assert h * (GV.A1 + GV.A2) < GV.BOUND                       # |k1|
    assert h * (GV.MB1 + GV.B2) < GV.BOUND                      # |k2|
    assert h * (GV.A1 + GV.MB1 + GV.A2 - GV.B2) < GV.BOUND      # |k1 - k2|
    assert h * (GV.MB1 + GV.B2) < GV.MB1 < GV.BOUND             # |k2 -+ |b1|| = |b1| - |k2| <= |b1|
    assert h * (GV.A1 + GV.A2) + GV.A1 < GV.BOUND               # |k1 +- a1|
    # translations alone cannot do it: no lattice vector with the parities (0, 1) fits 128 bits
    for m1 in range(-4, 5, 2):
        for m2 in range(-15, 16, 2):
            assert max(abs(1 + m1 * GV.A1 + m2 * GV.A2), abs(2 - m1 * GV.MB1 + m2 * GV.B2)) >= GV.BOUND


def test_model_edges_and_boundaries():
    top = [0, 0]
    for k in GV.edge_scalars() + GV.half_scalars() + GV.boundary_scalars():
        a, b = GV.check(k)
        top = [max(top[0], a), max(top[1], b)]
    # the boundary scalars reach the proven maximum, 0.9865 * 2^128, to within a few units
    worst = (GV.MB1 + GV.A2) // 2
    assert worst - 8 <= max(top) <= worst + 8


def test_model_random():
    rnd = random.Random(19)
    for _ in range(10 ** 6):
        k1, k2, _rot = GV.split_rot(rnd.getrandbits(256))
        assert k1 & k2 & 1 and -GV.BOUND < k1 < GV.BOUND and -GV.BOUND < k2 < GV.BOUND


@pytest.fixture(scope="module")
def hs():
    return _lib.load(build_hostsim(), optional=("ellgpu_probe_valu", "ellgpu_ctx_set_timing",
                                                "ellgpu_ctx_get_timing", "ellgpu_debug_field_op"))


@pytest.fixture(scope="module")
def full_ctx(hs):
    """every batch on the full-grid tuning: the 32-window ladder (the thresholds are read at creation)"""
    old = os.environ.get("ELLGPU_SMALL_GRID")
    os.environ["ELLGPU_SMALL_GRID"] = "0"
    try:
        c = elliptic_amd.Context(0, lib_path=hs)
    finally:
        if old is None:
            del os.environ["ELLGPU_SMALL_GRID"]
        else:
            os.environ["ELLGPU_SMALL_GRID"] = old
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx(hs):
    """the default thresholds: these batches take the small-grid tuning, whose split is unchanged"""
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


@pytest.mark.parametrize("which", ["full", "default"])
def test_mul_var_against_oracle(full_ctx, ctx, which):
    c, cs = (full_ctx if which == "full" else ctx), GV.engine_cases()
    xy, inf = c.mul_var("secp256k1", cs["k"], cs["pts"])
    assert np.array_equal(np.asarray(inf, np.uint8), cs["want_inf"])
    assert xy.tobytes() == cs["want_xy"].tobytes()


@pytest.mark.parametrize("which", ["full", "default"])
def test_ecdsa_verify_against_oracle(full_ctx, ctx, which):
    c, cs = (full_ctx if which == "full" else ctx), GV.engine_cases()
    ok = c.ecdsa_verify("secp256k1", cs["z"], cs["r"], cs["s"], cs["pub"])
    assert np.asarray(ok, np.uint8).tobytes() == cs["want_ok"].tobytes()
