"""The shared-inversion kernels with K > 1 items per inversion on the CPU build (tests/hostsim): the
cases of tests/inv_batch_checks.py in contexts created under ELLGPU_NORM_K / ELLGPU_PREP_K = (16, 8),
(3, 3), (64, 64) and (2, 2), each against a K = 1 context and against the integer models, with the
refused items placed per thread group; the placement helper's own coverage; and the guard that every
device routine with the parameters (t, T, n, K) has a row in the case table.

The CPU build has no timing entry points (ellgpu_ctx_set_timing / _get_timing): which kernels a call
launched is read from the build's own launch counters (hs_launches) instead, by the names the headers
give their kernels."""
import ctypes
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

from elliptic_amd import _lib  # noqa: E402
import inv_batch_checks as IB  # noqa: E402

OPTIONAL = ("ellgpu_probe_valu", "ellgpu_ctx_set_timing", "ellgpu_ctx_get_timing", "ellgpu_debug_field_op")
ROUTINES = ["edcecdsa.h:eq_affine", "edcecdsa.h:sign_norm", "edckey.h:derive_finish", "edckey.h:quotient",
            "edcustom.h:normalize", "edwards.h:normalize", "mont.h:normalize", "montcustom.h:normalize",
            "work.h:ecdsa_prep", "work.h:normalize", "work.h:recover_prep", "work.h:rt_derive_finish",
            "work.h:rt_recover_prep", "work.h:rt_sign_finish", "work.h:sign_finish"]


@pytest.fixture(scope="module")
def hs():
    lib = _lib.load(build_hostsim(), optional=OPTIONAL)
    lib.hs_launches.restype = ctypes.c_int
    lib.hs_launches.argtypes = [ctypes.c_char_p]
    return lib


@pytest.fixture(scope="module")
def contexts(hs):
    """the K = 1 context and one per forced (NORM_K, PREP_K), made on first use"""
    made = {}
    mp = pytest.MonkeyPatch()

    def get(ks):
        if ks not in made:
            made[ks] = IB.make_context(mp, ks, lib_path=hs)
        return made[ks]
    yield get
    for c in made.values():
        c.close()
    mp.undo()


@pytest.fixture(scope="module")
def kernel_names():
    """every kernel name of the headers (NAME = "..." of the launch functors)"""
    names = set()
    for f in os.listdir(IB.CSRC):
        if f.endswith(".h"):
            with open(os.path.join(IB.CSRC, f)) as fh:
                names |= set(re.findall(r'NAME = "(\w+)"', fh.read()))
    assert {"normalize", "ecdsa_prep", "ed_normalize"} <= names
    return sorted(names)


def test_the_overrides_set_K(contexts, hs):
    """37 items of mul_var on p256: one normalize launch, of ceil(37 / K) threads -- told by the answer
    for a batch whose refused items sit at stride T = 3 under K = 16 (and at other strides else)"""
    case = IB.case_of("mul_var-p256")
    for ks in [IB.REFERENCE_K] + IB.HOST_KS:
        ctx = contexts(ks)
        assert ctx.inv_ks == ks
        mask, plan = IB.placement(37, ks[0])
        assert len(plan) == -(-37 // ks[0]) and sum(c for _, c in plan) == 37
        ins, want = IB.compose(case.pool(), mask)
        hs.hs_launches_reset()
        got = case.run(ctx, ins, "dev_np")
        assert hs.hs_launches(b"normalize") == 1
        assert all((g == w).all() for g, w in zip(got, want))
    assert "ELLGPU_NORM_K" not in os.environ and "ELLGPU_COOP_GRID" not in os.environ


@pytest.mark.parametrize("K", sorted({k for ks in IB.HOST_KS for k in ks}))
def test_placement_covers_the_patterns(K):
    """per size: over its rotations every pattern falls on a group; the largest size has groups of the
    tail (cnt < K) with refused items, full groups with every pattern, and both kinds of item"""
    sizes = IB.sizes_of(K)
    assert sizes[-1] == 64 * K + 37 and set(sizes) == {n for n in (1, K - 1, K, K + 1, 2 * K + 1, 64 * K + 37) if n}
    for n in sizes:
        seen, T = set(), -(-n // K)
        for rot in range(IB.rotations_of(n, K)):
            mask, plan = IB.placement(n, K, rot)
            groups = IB.groups_of(n, K)
            assert len(groups) == T and sorted(i for g in groups for i in g) == list(range(n))
            assert all(g == list(range(g[0], n, T))[:K] and len(g) <= K for g in groups)
            for (pat, cnt), g in zip(plan, groups):
                seen.add(pat)
                hit = [int(mask[i]) for i in g]
                if pat == "first":
                    assert hit == [1] + [0] * (cnt - 1)
                elif pat == "last":
                    assert hit == [0] * (cnt - 1) + [1]
                elif pat == "all":
                    assert all(hit)
                elif pat == "none":
                    assert not any(hit)
                elif pat == "all_but_one":
                    assert sum(hit) == cnt - 1
                elif pat == "adjacent" and cnt >= 2:
                    assert sum(hit) == 2 and "11" in "".join(map(str, hit))
                elif pat == "middle" and cnt >= 3:
                    assert sum(hit) == 1 and not hit[0] and not hit[-1]
        assert seen == set(IB.PATTERNS), (K, n, seen)
    n = sizes[-1]
    mask, plan = IB.placement(n, K)
    groups = IB.groups_of(n, K)
    assert {pat for pat, cnt in plan if cnt == K} == set(IB.PATTERNS)
    tail = [(pat, g) for (pat, cnt), g in zip(plan, groups) if cnt < K]
    assert tail and any(mask[g].any() for _, g in tail)
    assert n < K or len({len(g) for g in groups}) == 2                  # an uneven tail
    assert mask.any() and not mask.all()


def test_every_routine_has_a_case():
    """a device routine whose parameters begin (size_t t, size_t T, size_t n, int K) shares an
    inversion: it needs a row in inv_batch_checks.CASES (and a row names no routine that is gone)"""
    found = IB.routines_in_headers()
    assert sorted(found) == ROUTINES, "a shared-inversion routine was added or removed: update CASES and this list"
    missing = set(found) - IB.routines_with_a_row()
    assert not missing, "no case in inv_batch_checks.CASES for %s" % sorted(missing)
    assert IB.routines_with_a_row() <= set(found)
    # ... and the guard bites: without the rows of one routine it is reported
    fewer = [c for c in IB.CASES if "edckey.h:quotient" not in c.routines]
    assert set(found) - IB.routines_with_a_row(fewer) == {"edckey.h:quotient"}


@pytest.mark.parametrize("id", IB.CASE_IDS)
def test_pool(id):
    """the pool of every case holds refused and ordinary items, and a composed batch has a refused
    item exactly where the mask says"""
    pool = IB.case_of(id).pool()
    assert 2 <= pool.refused.sum() and 4 <= (~pool.refused).sum()
    mask, _ = IB.placement(37, 3)
    ins, want = IB.compose(pool, mask)
    assert all(a.shape[0] == 37 for a in ins + want)
    ref = [tuple(a[i].tobytes() for a in pool.ins) for i in range(len(pool.refused)) if pool.refused[i]]
    got = [tuple(a[i].tobytes() for a in ins) for i in range(37)]
    assert all((g in ref) == bool(m) for g, m in zip(got, mask))


@pytest.mark.parametrize("ks", IB.HOST_KS, ids=lambda ks: "K%d_%d" % ks)
@pytest.mark.parametrize("id", IB.CASE_IDS)
def test_case(contexts, hs, kernel_names, id, ks):
    def launches(fn):
        hs.hs_launches_reset()
        fn()
        return {k: c for k, c in ((k, hs.hs_launches(k.encode())) for k in kernel_names) if c}

    ran = IB.check_case(IB.case_of(id), contexts(ks), contexts(IB.REFERENCE_K), "dev_np", launches, whole=True)
    assert ran >= len(IB.sizes_of(min(ks)))
