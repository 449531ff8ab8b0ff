#!/usr/bin/env python3
"""Records tests/golden/binding_sigs.json: for every key of elliptic_amd/_lib.py's _SIGS the restype
and the argtypes, by ctypes type name and in argument order, of the tree this is run in.

The fixture pins the prototypes as they stood when every ellgpu_X_dev entry was written out by hand;
tests/test_binding_sigs.py compares the table under test (whose _dev entries are derived from their
host entries) with it.  So run this in a checkout of the commit whose table is to be kept -- or
after a deliberate change of include/ellgpu.h -- never to make a failing test pass.

    python tools/record_binding_sigs.py [--out binding_sigs.json]

--table ext / ext2 / ext3 / ext4 records one of the later tables instead (_EXT_SIGS of include/ellgpu_ext.h
into binding_sigs_ext.json, _EXT2_SIGS of include/ellgpu_ext2.h into binding_sigs_ext2.json,
_EXT3_SIGS of include/ellgpu_ext3.h into binding_sigs_ext3.json, _EXT4_SIGS of include/ellgpu_ext4.h
into binding_sigs_ext4.json; --table addn: _SUM_SIGS of include/ellgpu_addn.h into
addn_binding_sigs.json; --table edsum: _EDSUM_SIGS of elliptic_amd/include/ellgpu_edsum.h into
edsum_binding_sigs.json): once, when the table is introduced.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elliptic_amd import _lib  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "binding_sigs.json")
TABLES = {"sigs": ("_SIGS", GOLDEN), "ext": ("_EXT_SIGS", GOLDEN.replace(".json", "_ext.json")),
          "ext2": ("_EXT2_SIGS", GOLDEN.replace(".json", "_ext2.json")),
          "ext3": ("_EXT3_SIGS", GOLDEN.replace(".json", "_ext3.json")),
          "ext4": ("_EXT4_SIGS", GOLDEN.replace(".json", "_ext4.json")),
          # (addn_binding_sigs.json, not binding_sigs_addn.json: tests/test_dev_streams_hostsim.py takes every
          # binding_sigs*.json for a table whose `mem` calls tests/dev_stream_checks.py schedules; ellgpu_mul_sum
          # is tested in flight in tests/test_mul_sum_gpu.py until that table names it)
          "addn": ("_SUM_SIGS", os.path.join(os.path.dirname(GOLDEN), "addn_binding_sigs.json")),
          # (named like addn's, for the same reason: ellgpu_ed_mul_sum is tested in flight in tests/test_ed_mul_sum_gpu.py)
          "edsum": ("_EDSUM_SIGS", os.path.join(os.path.dirname(GOLDEN), "edsum_binding_sigs.json"))}


def table(sigs=None):
    """{symbol: {"res": type name or None, "args": [type names]}}"""
    sigs = _lib._SIGS if sigs is None else sigs
    return {name: {"res": None if res is None else res.__name__, "args": [a.__name__ for a in args]}
            for name, (res, args) in sigs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--table", choices=sorted(TABLES), default="sigs")
    args = ap.parse_args()
    attr, default_out = TABLES[args.table]
    args.out = args.out or default_out
    data = table(getattr(_lib, attr))
    with open(args.out, "w") as f:
        json.dump(data, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d prototypes" % (args.out, len(data)))


if __name__ == "__main__":
    main()
