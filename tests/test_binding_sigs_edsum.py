"""The seventh prototype table, elliptic_amd/_lib.py's _EDSUM_SIGS, pinned the way the first six are
(tests/test_binding_sigs.py .. tests/test_binding_sigs_addn.py): elliptic_amd/include/ellgpu_edsum.h
declares the entry point added after tests/golden/addn_binding_sigs.json was recorded, and its
functions, EDSUM_SYMBOLS and the recorded tests/golden/edsum_binding_sigs.json are the same
one-element set, prototype for prototype; the prototype is ellgpu_mul_sum's; the library exports it,
the earlier tables hold none of it, ELLGPU_VERSION is what it was, and the header is one of the files
the library is built from, between the csrc files and include/."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "edsum_binding_sigs.json")
REL = os.path.join("elliptic_amd", "include", "ellgpu_edsum.h")
HEADER = os.path.join(ROOT, REL)


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_every_prototype_is_the_recorded_one():
    got, want = RB.table(_lib._EDSUM_SIGS), _golden()
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert RB.TABLES["edsum"] == ("_EDSUM_SIGS", GOLDEN)
    # (the name keeps the table out of the glob of tests/dev_stream_checks.py)
    assert not os.path.basename(GOLDEN).startswith("binding_sigs")


def test_symbols_are_the_table_and_the_header():
    declared = sorted(set(re.findall(r"\b(ellgpu_\w+)\s*\(", _code())))
    assert _lib.EDSUM_SYMBOLS == sorted(_golden()) == declared == ["ellgpu_ed_mul_sum"]
    earlier = (set(_lib.SYMBOLS) | set(_lib.EXT_SYMBOLS) | set(_lib.EXT2_SYMBOLS) | set(_lib.EXT3_SYMBOLS)
               | set(_lib.EXT4_SYMBOLS) | set(_lib.SUM_SYMBOLS))
    assert not set(_lib.EDSUM_SYMBOLS) & earlier
    assert not [s for s in _lib.EDSUM_SYMBOLS if s.endswith("_dev")]
    code = _code()
    assert '#include "../../include/ellgpu_addn.h"' in code and "ELLGPU_VERSION " not in code
    assert code.count("#include") == 1
    # the prototype is ellgpu_mul_sum's, in the binding table and in the two headers
    assert _lib._EDSUM_SIGS["ellgpu_ed_mul_sum"] == _lib._SUM_SIGS["ellgpu_mul_sum"]
    assert _golden()["ellgpu_ed_mul_sum"] == json.load(open(os.path.join(ROOT, "tests", "golden", "addn_binding_sigs.json")))["ellgpu_mul_sum"]
    proto = lambda src, name: re.sub(r"\s+", " ", re.search(r"int %s\(([^)]*)\)" % name, src).group(1))  # noqa: E731
    addn = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ellgpu_addn.h")).read(), flags=re.S)
    assert proto(code, "ellgpu_ed_mul_sum") == proto(addn, "ellgpu_mul_sum")


def test_the_method_has_no_dev_twin():
    """Context.ed_mul_sum takes both kinds of memory; Context.mul_sum is still there"""
    import elliptic_amd
    assert callable(elliptic_amd.Context.ed_mul_sum) and callable(elliptic_amd.Context.mul_sum)
    assert not hasattr(elliptic_amd.Context, "ed_mul_sum_dev")
    assert not [m for m in dir(elliptic_amd.Context) if "sum" in m and m.endswith("_dev")]


def test_library_exports_it_and_load_applies_the_table():
    from elliptic_amd import build as b
    if not os.path.exists(b.LIB):
        if shutil.which("hipcc") is None and not os.path.exists(b.HIPCC):
            pytest.skip("hipcc not available and libellgpu.so not built")
        b.build(verbose=False)
    raw = ctypes.CDLL(b.LIB)
    for name in _lib.EDSUM_SYMBOLS:
        assert hasattr(raw, name), "libellgpu.so does not export %s" % name
    lib = _lib.load(b.LIB)
    for name, (res, args) in _lib._EDSUM_SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ellgpu_version() == 0x000200 == _lib.ABI_VERSION


def test_header_is_a_source_file_at_its_sorted_place():
    from elliptic_amd import build as b
    files = b.source_files()[1]
    assert files.count(REL) == 1
    assert files[:-1] == sorted(files[:-1])
    i = files.index(REL)
    assert files[i - 1].startswith(os.path.join("elliptic_amd", "csrc") + os.sep)
    assert files[i + 1] == os.path.join("include", "ellgpu.h")
    # the definition is held to the declaration: the C ABI's translation unit includes the header
    capi = open(os.path.join(ROOT, "elliptic_amd", "csrc", "capi_common.h")).read()
    assert '#include "../include/ellgpu_edsum.h"' in capi
