"""Device-memory calls in flight on several streams (-m gpu): the schedules of tests/dev_stream_checks.py
on the device, with no host synchronisation between the calls of a repetition.  The expected bytes of
every (operation, m) are that same call issued alone on the default stream; a sample of each -- the
first 16 items and every faulty item -- is held to the model of the operation's check module.  Each
test is one schedule; a mismatch names the schedule, the repetition, the position in the queue, the
operation, the stream and m."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dev_stream_checks as DS  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    P = DS.TorchPlatform()
    cx = DS.Cx(P, DS.COMB_MAX_BYTES)               # raises if libellgpu.so or the GPU is missing
    exp = DS.Expected(P, cx, everything=False)
    yield P, exp
    P.sync()
    cx.close()


def test_expected_values_against_the_models(env):
    """every (operation, m) of schedule 1 alone on the default stream: no output is all zeros, the
    sample agrees with the model, statuses and verdicts included"""
    P, exp = env
    sizes = set()
    for nstreams in (2, 3):
        for pos, o in enumerate(DS.interleaved()):
            m = DS._size(o, pos + nstreams)
            sizes.add((o.curve == "secp256k1", m))
            _, want = exp.get(o, m)
            assert DS.check_against_model(o, m, want, everything=False) >= 16
    # secp256k1 met every batch size, and with them the row, wave, lane, small-grid and full-grid forms
    assert {m for k, m in sizes if k} == set(DS.SIZES_256)
    assert exp.cx.ctx.comb_bits("secp256k1") == 16                 # the tables stay at 8 or 16 bits, never 22


@pytest.mark.parametrize("nstreams", [2, 3])
def test_schedule_1_round_robin(env, nstreams):
    assert DS.schedule_round_robin(*env, nstreams) == len(DS.OPS())


def test_schedule_2_arena_grows(env):
    assert DS.schedule_grow(*env) == 6


def test_schedule_3_tables_built_on_first_use(env):
    assert DS.schedule_first_use(*env) == 3


def test_schedule_4_handle_released_under_a_walk(env):
    assert DS.schedule_release(*env) == 2 * env[0].reps


def test_schedule_5_user_defined_curves_take_turns(env):
    assert DS.schedule_custom_turns(*env) == 12


def test_schedule_6_host_and_deferred_calls_in_the_queue(env):
    assert DS.schedule_round_robin(*env, 2, with_host_calls=True) == len(DS.OPS())


@pytest.mark.parametrize("default_stream", [False, True])
def test_schedule_7_callers_own_work(env, default_stream):
    assert DS.schedule_callers_work(*env, default_stream) == 3 * env[0].reps
