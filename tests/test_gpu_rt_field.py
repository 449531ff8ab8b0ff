"""The run-time-modulus field (csrc/fp_rt.h) and the group law on user-defined curves across the
prime range, on the MI355X: the checks of tests/rt_field_checks.py (shared with
tests/test_rt_field_hostsim.py) through libellgpu.so -- the field probe ids 100+slot / 200+slot of
ellgpu_debug_field_op against Python integers, presets defined again as user-defined curves, and
primes no fixture has against an affine law."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rt_field_checks as RT  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    e = RT.Env(None, hostsim=False)          # Context(0) raises if libellgpu.so or the GPU is missing
    yield e
    e.close()


@pytest.fixture(scope="module")
def ctx(env):
    return env.new_ctx()


@pytest.mark.parametrize("p", RT.MODULI_P, ids=lambda p: "p%d_%x" % (p.bit_length(), p & 0xFFFF))
def test_rt_field_ops_gpu(env, p):
    ctx, field = env.field_p(p)
    RT.check_field(env, ctx, field, p, seed=4242 + p % 9973)


@pytest.mark.parametrize("label", RT.MODULI_N)
def test_rt_order_field_ops_gpu(env, label):
    ctx, field = env.field_n(label)
    RT.check_field(env, ctx, field, RT.order_modulus(label), seed=77 + len(label))


def test_rt_probe_refusals_gpu(env):
    RT.check_probe_refusals(env)


@pytest.mark.parametrize("name", RT.PRESETS)
def test_preset_as_custom_curve_gpu(ctx, name):
    assert RT.check_preset_as_custom(ctx, name) == 307


@pytest.mark.parametrize("name", RT.PRESETS)
def test_preset_as_custom_domain_verify_gpu(ctx, name):
    assert RT.check_preset_verify(ctx, name) >= 15


def test_ed25519_as_custom_edwards_gpu(ctx):
    assert RT.check_ed25519_as_custom(ctx) == 200


@pytest.mark.parametrize("p", RT.NEW_PRIMES, ids=lambda p: "p%d_%x" % (p.bit_length(), p & 0xFFFF))
def test_new_prime_group_law_gpu(env, p):
    assert RT.check_new_prime(env.new_ctx(), p) == 400


@pytest.mark.parametrize("p", RT.TOY_PRIMES)
def test_toy_prime_exhaustive_gpu(env, p):
    assert RT.check_toy_exhaustive(env.new_ctx(), p) > 100
