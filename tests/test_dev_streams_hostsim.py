"""The schedules of tests/dev_stream_checks.py run serially through the host simulation (device memory
is host memory, one null stream, every batch capped at 96 items): the schedules, their operands and
their expected values are right -- every operation of the table is held to the model of its check
module over ALL its items, every faulty-item class is present, no expected output is all zeros.  This
run raises no claim about ordering; tests/test_dev_streams_gpu.py does."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

from elliptic_amd import _lib  # noqa: E402
import dev_stream_checks as DS  # noqa: E402
import key_recid_checks as KR  # noqa: E402


@pytest.fixture(scope="module")
def env():
    lib = _lib.load(build_hostsim(), optional=KR.OPTIONAL)
    P = DS.HostsimPlatform(lib)
    cx = DS.Cx(P)
    yield P, DS.Expected(P, cx, everything=True)
    cx.close()


def test_table_covers_the_binding_tables():
    """every `_dev` symbol and every `mem`-taking entry point of the recorded binding tables is an
    operation of the table or an exclusion with its reason: a new entry point fails here until it is scheduled"""
    symbols = DS.device_memory_symbols()
    assert len(symbols) >= 45 and {"ellgpu_mul_base", "ellgpu_ecdsa_recid", "ellgpu_eddsa_verify_base"} <= symbols
    scheduled = {s for o in DS.OPS() for s in o.symbols}
    assert not scheduled & set(DS.EXCLUDED)
    assert all(len(reason) > 20 for reason in DS.EXCLUDED.values())
    assert scheduled | set(DS.EXCLUDED) == symbols, (sorted(symbols - scheduled - set(DS.EXCLUDED)),
                                                      sorted((scheduled | set(DS.EXCLUDED)) - symbols))


def test_table_holds_what_the_schedules_name():
    have = {(o.name, o.curve) for o in DS.OPS()}
    for c in DS.PRESETS:
        for n in ("mul_fixed_dev", "mul_var_dev", "mul_add2_dev", "mul_add2_dev[p1=None]", "ecdsa_verify_dev", "ecdsa_sign_det_dev",
                  "ecdsa_recover_dev", "decompress_dev", "ecdsa_verify_wire_dev"):
            assert (n, c) in have, (n, c)
    for n in ("eddsa_verify_dev", "eddsa_sign_dev", "mul_base[ed25519]", "mul_base2[ed25519]", "eddsa_verify_base"):
        assert (n, "ed25519") in have, n
    assert ("x25519_dev", "curve25519") in have
    for n in ("mul_base", "mul_base2", "ecdsa_verify_base", "ecdsa_recid"):
        assert (n, "secp256k1") in have, n
    for c in DS.SHORT_DOMAINS:
        for n in ("custom_verify_wire_dev", "custom_recover_dev", "custom_sign_det_dev", "custom_derive_dev"):
            assert (n, c) in have, (n, c)
    assert {("custom_ed_verify_dev", DS.EDWARDS), ("custom_mont_ladder_dev", DS.MONT), ("mul_base[plain id]", DS.PLAIN)} <= have
    # the faulty-item classes of the reused check modules
    want = {"off_curve", "r_range", "sum_inf", "u1_zero", "flip_r", "flip_s", "flip_hash", "infinity", "doubling", "key_prefix",
            "sig_der", "key_parity", "r_wide", "throws", "outside", "offcurve", "undecodable", "S_n", "S_zero", "noncanon",
            "not_validated", "no_point", "identity", "r_0", "s_0", "r_n", "s_n", "key_identity", "key_small_order"}
    seen = {k for o in DS.OPS() for k in o.faulty}
    assert want <= seen, sorted(want - seen)
    assert all(0 <= i < DS.D for o in DS.OPS() for i in o.faulty.values())


def test_expected_values_are_the_models(env):
    """every operation of the table alone: all items against the model (Expected.get asks), no output all zeros"""
    P, exp = env
    for o in DS.OPS():
        m = exp.size(o.sizes[-1])
        _, want = exp.get(o, m)
        assert DS.check_against_model(o, m, want, everything=True) == m == DS.HOSTSIM_CAP, (o.name, o.curve)


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
