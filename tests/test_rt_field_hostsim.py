"""The run-time-modulus field (csrc/fp_rt.h) and the group law on user-defined curves across the
prime range, on the CPU: the hostsim build of the device code (tests/hostsim) through the checks
of tests/rt_field_checks.py -- field operations against Python integers on twenty moduli from 5
to 2^256 - 189 and five orders, presets defined again as user-defined curves against the preset
ids, recorded verdicts and the C oracle, and primes no fixture has against an affine law."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

from elliptic_amd import _lib  # noqa: E402
import rt_field_checks as RT  # noqa: E402


@pytest.fixture(scope="module")
def env():
    hs = _lib.load(build_hostsim(), optional=("ellgpu_probe_valu", "ellgpu_ctx_set_timing",
                                              "ellgpu_ctx_get_timing", "ellgpu_debug_field_op"))
    e = RT.Env(hs, hostsim=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ctx(env):
    return env.new_ctx()


def test_moduli_are_prime():
    for p in RT.MODULI_P + [RT.order_modulus(n) for n in RT.MODULI_N]:
        assert RT.is_prime(p), hex(p)
    assert all(p % 4 == 3 for p in RT.NEW_PRIMES)
    assert 0 < 5 * RT.P08 - 4 * 2 ** 256 < 2 ** 16                # just above 0.8 * 2^256


@pytest.mark.parametrize("p", RT.MODULI_P, ids=lambda p: "p%d_%x" % (p.bit_length(), p & 0xFFFF))
def test_rt_field_ops(env, p):
    """FpMontRT over p: add, sub, mul, sqr, neg, the doublings and inv on edge, unreduced, directed
    and 1500 random operands; the vectors reach every branch of redc and mod_add that exists for p"""
    ctx, field = env.field_p(p)
    RT.check_field(env, ctx, field, p, seed=4242 + p % 9973)


@pytest.mark.parametrize("label", RT.MODULI_N)
def test_rt_order_field_ops(env, label):
    """FpMontRTn over the order of a domain (secp256k1, P-256 -- top word all ones --, P-224,
    brainpoolP256r1, 2^61 - 1)"""
    ctx, field = env.field_n(label)
    RT.check_field(env, ctx, field, RT.order_modulus(label), seed=77 + len(label))


def test_rt_probe_refusals(env):
    RT.check_probe_refusals(env)


@pytest.mark.parametrize("name", RT.PRESETS)
def test_preset_as_custom_curve(ctx, name):
    assert RT.check_preset_as_custom(ctx, name) == 307


@pytest.mark.parametrize("name", RT.PRESETS)
def test_preset_as_custom_domain_verify(ctx, name):
    assert RT.check_preset_verify(ctx, name) >= 15


def test_ed25519_as_custom_edwards(ctx):
    assert RT.check_ed25519_as_custom(ctx) == 200


@pytest.mark.parametrize("p", RT.NEW_PRIMES, ids=lambda p: "p%d_%x" % (p.bit_length(), p & 0xFFFF))
def test_new_prime_group_law(env, p):
    assert RT.check_new_prime(env.new_ctx(), p) == 400


@pytest.mark.parametrize("p", RT.TOY_PRIMES)
def test_toy_prime_exhaustive(env, p):
    assert RT.check_toy_exhaustive(env.new_ctx(), p) > 100
