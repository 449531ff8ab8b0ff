"""The lanes-per-item field layers (csrc/coop.h, coop_mont.h, coop_wide.h, coop_ed.h) operation by
operation against Python integers, on the CPU: the hostsim build of the device headers (a row is an
array of sixteen lanes there) through the checks of tests/coop_field_checks.py.  The same vectors run
on the MI355X in tests/test_gpu_coop_field.py; here they prove the algebra and the vectors themselves
(the bounds checks of ELL_BOUNDS_CHECK included) before either reaches a GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

from elliptic_amd import _lib  # noqa: E402
import coop_field_checks as CF  # noqa: E402


@pytest.fixture(scope="module")
def env():
    hs = _lib.load(build_hostsim(), optional=("ellgpu_probe_valu", "ellgpu_ctx_set_timing",
                                              "ellgpu_ctx_get_timing", "ellgpu_debug_field_op"))
    e = CF.Env(hs, hostsim=True)
    yield e
    e.close()


@pytest.mark.parametrize("field", sorted(CF.FIELDS))
def test_operand_lists_cover_every_class(field):
    c = CF.check_coverage(field)
    assert len(CF.main_pairs(field)) >= 2000 and (field != 4 or len(CF.main_pairs(4)) % 4 == 1), c


@pytest.mark.parametrize("field", sorted(CF.FIELDS))
def test_coop_field_ops(env, field):
    assert CF.check_ops(env, field) >= 2000 * len(CF.ops_of(field))


@pytest.mark.parametrize("field", [5, 31, 32, 33, 34, 35])
def test_coop_field_inversion(env, field):
    assert CF.check_inversion(env, field) >= 55


@pytest.mark.parametrize("field", CF.QUAD)
def test_coop_field_four_products(env, field):
    assert CF.check_quad(env, field) >= 400 * len(CF.quad_ops_of(field))


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_row_per_item_ragged_batches(env, n):
    assert CF.check_ragged(env, n) == n


def test_row_per_item_neighbour_rows(env):
    assert CF.check_neighbour_rows(env) > 4 * 100 * len(CF.ops_of(4))


def test_coop_probe_refusals(env):
    CF.check_refusals(env)
