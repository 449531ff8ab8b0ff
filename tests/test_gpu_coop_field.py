"""The lanes-per-item field layers (csrc/coop.h, coop_mont.h, coop_wide.h, coop_ed.h) operation by
operation against Python integers, on the MI355X: field ids 3, 4, 5 and 31..35 of
ellgpu_debug_field_op through the checks of tests/coop_field_checks.py (shared with
tests/test_coop_field_hostsim.py).  This is where the device branch of the row primitives -- DPP
row_shr / row_newbcast, v_readlane, the permlane swaps of pack* / unpack*, the zero tests across a
row -- meets an expected value: a wrong carry across a lane shows here as a wrong field element, not
as a wrong curve point."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import coop_field_checks as CF  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    e = CF.Env(None, hostsim=False)
    yield e
    e.close()


@pytest.mark.parametrize("field", sorted(CF.FIELDS))
def test_operand_lists_cover_every_class_gpu(field):
    c = CF.check_coverage(field)
    assert len(CF.main_pairs(field)) >= 2000 and (field != 4 or len(CF.main_pairs(4)) % 4 == 1), c


@pytest.mark.parametrize("field", sorted(CF.FIELDS))
def test_coop_field_ops_gpu(env, field):
    assert CF.check_ops(env, field) >= 2000 * len(CF.ops_of(field))


@pytest.mark.parametrize("field", [5, 31, 32, 33, 34, 35])
def test_coop_field_inversion_gpu(env, field):
    assert CF.check_inversion(env, field) >= 55


@pytest.mark.parametrize("field", CF.QUAD)
def test_coop_field_four_products_gpu(env, field):
    assert CF.check_quad(env, field) >= 400 * len(CF.quad_ops_of(field))


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_row_per_item_ragged_batches_gpu(env, n):
    assert CF.check_ragged(env, n) == n


def test_row_per_item_neighbour_rows_gpu(env):
    assert CF.check_neighbour_rows(env) > 4 * 100 * len(CF.ops_of(4))


def test_coop_probe_refusals_gpu(env):
    CF.check_refusals(env)
