"""One Engine function serves the host-buffer and the device-pointer form of every batch entry
point.  What each form answers to a call that must not run -- an empty batch, a null buffer, a
zero length, on every kind of curve id -- and which kernels a batch launches, how often, were
recorded from the engine when the two forms were separate functions
(tools/record_entry_forms.py -> tests/golden/entry_forms.json) and are compared here on the CPU
build (tests/hostsim).  No message was changed on purpose: codes and messages are both pinned."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hostsim.build import build as build_hostsim  # noqa: E402

import elliptic_amd  # noqa: E402
import entry_forms_cases as EF  # noqa: E402


@pytest.fixture(scope="module")
def hs():
    return EF.load(build_hostsim())


@pytest.fixture(scope="module")
def golden():
    with open(EF.GOLDEN) as f:
        return json.load(f)


@pytest.fixture()
def ctx(hs):
    c = elliptic_amd.Context(0, lib_path=hs)
    yield c
    c.close()


def test_cases_cover_every_batch_entry_point(hs):
    """every ellgpu_X that has an ellgpu_X_dev is in the table"""
    import re
    with open(os.path.join(os.path.dirname(EF.HERE), "include", "ellgpu.h")) as f:
        dev = set(re.findall(r"ellgpu_(\w+)_dev\(", f.read()))
    assert dev == set(EF.ENTRIES)


def test_codes_and_messages(hs, ctx, golden):
    """n = 0 with null buffers, n = 1 with the first required buffer null, n = 1 with hash_len /
    enc_len / stride / pub_len = 0: (code, message) of both forms on every kind of curve id"""
    hs.hs_launches_reset()
    got = EF.error_table(hs, ctx, EF.define_curves(ctx))
    assert set(got) == set(golden["errors"])
    wrong = {k: (v, golden["errors"][k]) for k, v in got.items() if v != golden["errors"][k]}
    assert not wrong, "%d of %d differ, e.g. %r" % (len(wrong), len(got), sorted(wrong.items())[:5])
    assert not any(hs.hs_launches(k.encode()) for k in EF.kernel_names()), "a refused call launched a kernel"


def test_launch_counts_and_results(hs, ctx, golden):
    """a batch of 20 (several pipeline steps of the host form, a short tail): the kernels each form
    launches and how often, and the two forms' results, byte for byte"""
    counts, results = EF.launch_table(hs, ctx, EF.define_curves(ctx))
    for label, want in golden["launches"].items():
        assert counts[label] == want, label
        assert results[label]["host"] == results[label]["dev"], label
    assert set(counts) == set(golden["launches"])
