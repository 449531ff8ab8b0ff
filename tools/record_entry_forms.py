#!/usr/bin/env python3
"""Records tests/golden/entry_forms.json: the (code, message) of every case of
tests/entry_forms_cases.py and the per-kernel launch counts of its sampled calls, from the CPU
build (tests/hostsim) of the tree this is run in.

The fixture pins what the engine did BEFORE an operation's host and device forms became one
function; tests/test_entry_forms_hostsim.py compares the tree under test with it.  So run this in
a checkout of the commit whose behaviour is to be kept, and copy the file over: never to make a
failing test pass.

    python tools/record_entry_forms.py [--lib libellgpu_hostsim.so] [--out entry_forms.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elliptic_amd  # noqa: E402
import entry_forms_cases as EF  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="a built libellgpu_hostsim.so (default: build this tree's)")
    ap.add_argument("--out", default=EF.GOLDEN)
    args = ap.parse_args()
    if not args.lib:
        from hostsim.build import build
        args.lib = build()
    lib = EF.load(args.lib)
    data = {}
    ctx = elliptic_amd.Context(0, lib_path=lib)
    data["errors"] = EF.error_table(lib, ctx, EF.define_curves(ctx))
    ctx.close()
    ctx = elliptic_amd.Context(0, lib_path=lib)
    data["launches"], _ = EF.launch_table(lib, ctx, EF.define_curves(ctx))
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(data, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d cases, %d sampled calls" % (args.out, len(data["errors"]), len(data["launches"])))


if __name__ == "__main__":
    main()
