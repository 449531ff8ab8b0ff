"""The ctypes prototypes of elliptic_amd/_lib.py against tests/golden/binding_sigs.json, recorded
(tools/record_binding_sigs.py) when every ellgpu_X_dev entry was written out by hand beside its host
entry.  The _dev entries are now derived (host argument list + the stream): each must come out as it
was written, entry for entry and in argument order."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from elliptic_amd import _lib  # noqa: E402
import record_binding_sigs as RB  # noqa: E402


def _golden():
    with open(RB.GOLDEN) as f:
        return json.load(f)


def test_every_prototype_is_the_recorded_one():
    got, want = RB.table(), _golden()
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def test_symbols_are_the_table():
    assert _lib.SYMBOLS == sorted(_golden())


def test_the_fixture_holds_every_dev_form():
    """the recorded table is not a thinned one: every batch entry point of include/ellgpu.h with a
    _dev form has both prototypes in it, the _dev one ending in the stream"""
    import re
    with open(os.path.join(ROOT, "include", "ellgpu.h")) as f:
        dev = set(re.findall(r"(ellgpu_\w+_dev)\(", f.read()))
    want = _golden()
    assert dev and dev <= set(want)
    for name in dev:
        assert want[name]["args"][-1] == "c_void_p" and name[:-4] in want, name
