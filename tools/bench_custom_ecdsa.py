#!/usr/bin/env python3
"""ECDSA verify throughput on a user-defined domain (brainpoolP256r1 through
ellgpu_curve_define_short_domain), device-resident buffers, HIP-event timing; beside it, on the
same curve and keys, k*G through the domain's comb and the two-point mul_add2 of a plain
user-defined curve (the comparison point: what a verify cost before the domain existed).
Developer tool (GPU box).

The signatures are drawn at random with 1 <= r, s < n over keys on the curve, so that every item
runs the whole verify (the work does not depend on the verdict).

    [ELLGPU_LIB=variant.so] python tools/bench_custom_ecdsa.py [log2 n ...]   (default: 18 20)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps=5):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(ctx, spec, n):
    import numpy as np
    import torch
    import bench
    import custom_domain_checks as CD
    cid = CD.define(ctx, spec)
    plain = ctx.define_short(*CD.params(spec)[:3])
    nn = CD.I(spec["n"])
    # scalars below n: 256 random bits with the top bit cleared (brainpoolP256r1's n > 2^255)
    def below_n(tag):
        a = bench.xof("custom-ecdsa:" + tag, n * 32).reshape(n, 32).copy()
        a[:, 0] &= 0x7F
        a[:, 31] |= 1
        return a
    d, r, s = below_n("d"), below_n("r"), below_n("s")
    assert int.from_bytes(bytes(d[0]), "big") < nn
    q, inf = ctx.mul_fixed(cid, d)
    assert not inf.any()
    h = bench.xof("custom-ecdsa:h", n * 32).reshape(n, 32).copy()
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dh, dr, ds, dq, dd = t(h), t(r), t(s), t(q), t(d)
    dg = t(np.tile(np.concatenate([CD.b32(CD.I(spec["g"]["x"])), CD.b32(CD.I(spec["g"]["y"]))]), (n, 1)))
    ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    dxy = torch.zeros(n, 64, dtype=torch.uint8, device=dev)
    dinf = torch.zeros(n, dtype=torch.uint8, device=dev)
    out = {"lib": os.path.basename(os.environ.get("ELLGPU_LIB", "libellgpu.so")), "curve": spec["name"], "n": n}
    for name, fn in (("verify", lambda: ctx.ecdsa_verify_dev(cid, dh, dr, ds, dq, ok)),
                     ("mul_add_g", lambda: ctx.mul_add2_dev(cid, dr, None, ds, dq, dxy, dinf)),
                     ("mul_fixed", lambda: ctx.mul_fixed_dev(cid, dd, dxy, dinf)),
                     ("plain_mul_add2", lambda: ctx.mul_add2_dev(plain, dr, dg, ds, dq, dxy, dinf))):
        ms = timed(fn)
        out[name + "_ms"] = round(ms, 3)
        out[name + "_M_per_s"] = round(n / ms / 1e3, 2)
    return out


def main():
    import torch
    import elliptic_amd
    import custom_domain_checks as CD
    spec = next(c for c in CD.curves() if c["name"] == "brainpoolP256r1")
    torch.zeros(1, device="cuda:0")          # the HIP runtime initialised by torch first, as in bench.py
    ctx = elliptic_amd.Context(0)
    try:
        for lg in [int(a) for a in sys.argv[1:]] or [18, 20]:
            print(json.dumps(run(ctx, spec, 1 << lg)), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
