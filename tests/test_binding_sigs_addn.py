"""The sixth prototype table, elliptic_amd/_lib.py's _SUM_SIGS, pinned the way the first five are
(tests/test_binding_sigs.py .. tests/test_binding_sigs_ext4.py): include/ellgpu_addn.h declares the
entry point added after tests/golden/binding_sigs_ext4.json was recorded, and its functions,
SUM_SYMBOLS and the recorded tests/golden/addn_binding_sigs.json are the same one-element set,
prototype for prototype; the library exports it, the earlier tables hold none of it, ELLGPU_VERSION
is what it was, and the header sits at its sorted place in the list of files the library is built
from."""
import ctypes
import json
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from elliptic_amd import _lib  # noqa: E402
import record_binding_sigs as RB  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "addn_binding_sigs.json")
HEADER = os.path.join(ROOT, "include", "ellgpu_addn.h")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ellgpu_\w+)\s*\(", src)))


def test_every_prototype_is_the_recorded_one():
    got, want = RB.table(_lib._SUM_SIGS), _golden()
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert RB.TABLES["addn"] == ("_SUM_SIGS", GOLDEN)


def test_symbols_are_the_table_and_the_header():
    assert _lib.SUM_SYMBOLS == sorted(_golden()) == _declared() == ["ellgpu_mul_sum"]
    earlier = (set(_lib.SYMBOLS) | set(_lib.EXT_SYMBOLS) | set(_lib.EXT2_SYMBOLS) | set(_lib.EXT3_SYMBOLS)
               | set(_lib.EXT4_SYMBOLS))
    assert not set(_lib.SUM_SYMBOLS) & earlier
    assert not [s for s in _lib.SUM_SYMBOLS if s.endswith("_dev")]
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert '#include "ellgpu_ext4.h"' in code and '#include "ellgpu.h"' not in code and "ELLGPU_VERSION " not in code
    # the call has one form: `mem` and the stream close its list, as in ellgpu_mul_base
    res, args = _lib._SUM_SIGS["ellgpu_mul_sum"]
    assert res is ctypes.c_int and args[-2:] == [ctypes.c_int, ctypes.c_void_p] == _lib._SIGS["ellgpu_mul_base"][1][-2:]
    # ... and takes (ctx, curve, n, m) and ellgpu_mul_var's four buffers between them
    assert args[:4] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t]
    assert args[4:-2] == _lib._SIGS["ellgpu_mul_var"][1][3:] == [_lib.c_u8p] * 4


def test_no_dev_twin_among_the_methods():
    """Context.mul_sum takes both kinds of memory: no method whose name ends in _dev came with it"""
    import elliptic_amd
    assert callable(elliptic_amd.Context.mul_sum)
    assert not [m for m in dir(elliptic_amd.Context) if "sum" in m and m.endswith("_dev")]
    assert not hasattr(elliptic_amd.Context, "mul_sum_dev")


def test_library_exports_it_and_load_applies_the_table():
    from elliptic_amd import build as b
    if not os.path.exists(b.LIB):
        if shutil.which("hipcc") is None and not os.path.exists(b.HIPCC):
            pytest.skip("hipcc not available and libellgpu.so not built")
        b.build(verbose=False)
    raw = ctypes.CDLL(b.LIB)
    for name in _lib.SUM_SYMBOLS:
        assert hasattr(raw, name), "libellgpu.so does not export %s" % name
    lib = _lib.load(b.LIB)
    for name, (res, args) in _lib._SUM_SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ellgpu_version() == 0x000200


def test_header_sits_at_its_sorted_place():
    from elliptic_amd import build as b
    files = b.source_files()[1]
    inc = [f for f in files if f.startswith("include" + os.sep)]
    assert inc == [os.path.join("include", h) for h in ("ellgpu.h", "ellgpu_addn.h", "ellgpu_ext.h", "ellgpu_ext2.h",
                                                        "ellgpu_ext3.h", "ellgpu_ext4.h")]
    assert files[-2:] == inc[-2:] and files[:-1] == sorted(files[:-1])
