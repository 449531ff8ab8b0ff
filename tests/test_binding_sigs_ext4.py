"""The fifth prototype table, elliptic_amd/_lib.py's _EXT4_SIGS, pinned the way the first four are
(tests/test_binding_sigs.py, tests/test_binding_sigs_ext.py, tests/test_binding_sigs_ext2.py,
tests/test_binding_sigs_ext3.py): include/ellgpu_ext4.h declares the entry points added after
tests/golden/binding_sigs_ext3.json was recorded, and its functions, EXT4_SYMBOLS and the recorded
tests/golden/binding_sigs_ext4.json are the same set, prototype for prototype; the library exports
every one of them, the earlier tables hold none of them, and ELLGPU_VERSION is what it was."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "binding_sigs_ext4.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _declared():
    src = open(os.path.join(ROOT, "include", "ellgpu_ext4.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ellgpu_\w+)\s*\(", src)))


def test_every_prototype_is_the_recorded_one():
    got, want = RB.table(_lib._EXT4_SIGS), _golden()
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert RB.TABLES["ext4"] == ("_EXT4_SIGS", GOLDEN)


def test_symbols_are_the_table_and_the_header():
    assert _lib.EXT4_SYMBOLS == sorted(_golden()) == _declared() == ["ellgpu_ecdsa_recid"]
    assert not set(_lib.EXT4_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.EXT_SYMBOLS) | set(_lib.EXT2_SYMBOLS) | set(_lib.EXT3_SYMBOLS))
    assert not [s for s in _lib.EXT4_SYMBOLS if s.endswith("_dev")]
    src = open(os.path.join(ROOT, "include", "ellgpu_ext4.h")).read()
    assert '#include "ellgpu_ext3.h"' in src and '#include "ellgpu.h"' not in src and "ELLGPU_VERSION " not in re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    # the call has one form: `mem` and the stream close its list, as in ellgpu_mul_base
    res, args = _lib._EXT4_SIGS["ellgpu_ecdsa_recid"]
    assert res is ctypes.c_int and args[-2:] == [ctypes.c_int, ctypes.c_void_p] == _lib._SIGS["ellgpu_mul_base"][1][-2:]
    # ... and takes ellgpu_ecdsa_recover's operands with the key in the id's place and a second result
    rec = _lib._SIGS["ellgpu_ecdsa_recover"][1]
    assert args[:-2] == rec[:8] + [_lib.c_u8p, _lib.c_u8p] and len(args) == len(rec) + 2


def test_library_exports_them_and_load_applies_the_table():
    from elliptic_amd import build as b
    if not os.path.exists(b.LIB):
        if shutil.which("hipcc") is None and not os.path.exists(b.HIPCC):
            pytest.skip("hipcc not available and libellgpu.so not built")
        b.build(verbose=False)
    raw = ctypes.CDLL(b.LIB)
    for name in _lib.EXT4_SYMBOLS:
        assert hasattr(raw, name), "libellgpu.so does not export %s" % name
    lib = _lib.load(b.LIB)
    for name, (res, args) in _lib._EXT4_SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ellgpu_version() == 0x000200
    files = b.source_files()[1]
    assert files[-1] == os.path.join("include", "ellgpu_ext4.h") and files[-2] == os.path.join("include", "ellgpu_ext3.h")
