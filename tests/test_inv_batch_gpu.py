"""The shared-inversion kernels with K > 1 items per inversion on the device: the cases of
tests/inv_batch_checks.py in contexts created under ELLGPU_NORM_K / ELLGPU_PREP_K = (16, 8), the
production maxima, and (3, 3), each against a K = 1 context and against the integer models, on device
tensors, with the refused items placed per thread group.  Per call the kernel timing (set_timing /
get_timing) has to show the one-lane kernel of the case and no lanes-per-item kernel (_c / _r).

Three contexts for the module; their own fixed-base tables are capped at 64 MiB (16-bit combs)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import inv_batch_checks as IB  # noqa: E402

pytestmark = pytest.mark.gpu
COMB_MAX_BYTES = 64 << 20


@pytest.fixture(scope="module")
def contexts():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    made = {}
    mp = pytest.MonkeyPatch()

    def get(ks):
        if ks not in made:
            assert len(made) < 3
            made[ks] = IB.make_context(mp, ks, comb_max_bytes=COMB_MAX_BYTES)
        return made[ks]
    yield get
    for c in made.values():
        c.close()
    mp.undo()


@pytest.mark.parametrize("ks", IB.DEVICE_KS, ids=lambda ks: "K%d_%d" % ks)
@pytest.mark.parametrize("id", IB.CASE_IDS)
def test_case(contexts, id, ks):
    ctx = contexts(ks)

    def launches(fn):
        ctx.set_timing(True)
        try:
            fn()
            return {k: v[0] for k, v in ctx.get_timing().items()}
        finally:
            ctx.set_timing(False)

    ran = IB.check_case(IB.case_of(id), ctx, contexts(IB.REFERENCE_K), "dev_torch", launches)
    assert ran >= len(IB.sizes_of(min(ks)))
