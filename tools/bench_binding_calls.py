#!/usr/bin/env python3
"""Per-call cost of the Python binding alone: Context.ecdsa_verify_dev and Context.mul_var at n = 1
against a stub library whose every function returns 0 (no GPU, no libellgpu.so).  The _dev call gets
a stand-in tensor (a shape and an address) and a null stream, as tests/test_binding_forms_hostsim.py
does.  Prints microseconds per call for each repeat; docs/EXPERIMENTS.md records the numbers.

    python tools/bench_binding_calls.py [--calls 100000] [--repeats 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import elliptic_amd  # noqa: E402
from elliptic_amd import _lib  # noqa: E402


class Stub:
    """every ellgpu_* function answers 0"""

    def ellgpu_version(self):
        return _lib.ABI_VERSION

    def __getattr__(self, name):
        if not name.startswith("ellgpu_"):
            raise AttributeError(name)
        fn = lambda *args: 0                                # noqa: E731
        setattr(self, name, fn)
        return fn


class Dev:
    def __init__(self, a):
        self._a = a
        self.shape = a.shape

    def data_ptr(self):
        return self._a.ctypes.data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    ctx = elliptic_amd.Context(0, lib_path=Stub())
    ctx._stream = lambda: None
    z32, z64, z1 = np.zeros((1, 32), np.uint8), np.zeros((1, 64), np.uint8), np.zeros(1, np.uint8)
    d32, d64, d1 = Dev(z32), Dev(z64), Dev(z1)
    out = (np.zeros((1, 64), np.uint8), np.zeros(1, np.uint8))
    runs = {"ecdsa_verify_dev": lambda: ctx.ecdsa_verify_dev("secp256k1", d32, d32, d32, d64, d1),
            "mul_var": lambda: ctx.mul_var("secp256k1", z32, z64, out=out)}
    for name, call in runs.items():
        us = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            us.append((time.perf_counter() - t0) / args.calls * 1e6)
        print("%-18s %s us/call" % (name, "  ".join("%.3f" % v for v in us)))


if __name__ == "__main__":
    main()
