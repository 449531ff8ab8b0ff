#!/usr/bin/env python3
"""Throughput of ellgpu_mul_sum (n sums of m terms k * P) on secp256k1 and p256, device-resident
buffers, HIP-event timing.  Developer tool (GPU box).

2^--log2t terms in all, as (n, m) = (T / 2, 2), (T / 8, 8), (2^10, T / 2^10) and (1, T): random
scalars on random multiples of G.  In one process, on the same terms:
  mul_sum               the new call;
  mul_add2 + point_add  the only way without it: ellgpu_mul_add2_dev over the pairs of neighbouring
                        terms, then ceil(log2(m / 2)) passes of ellgpu_point_add_dev over the halves
                        of the partial sums, each pass with its own normalisation (the partial sums
                        are laid out pair-major so that every pass reads two contiguous halves);
  ... (repeat)          the same baseline again: the difference of the two is the run-to-run spread.
Before anything is timed the outputs of the two are compared at the timed size.  Rows are warmed up,
then timed for at least --seconds of back-to-back calls, --rounds times, alternating inside a round
so that drift is shared; reported: the median round in terms/s and the spread (min .. max).  Last,
the latency of one small call: mul_sum at (1, 2) and (1, 8) against mul_add2_dev at n = 1.  One JSON
line per row, also appended to --out.

    python tools/bench_mul_sum.py [--log2t 20] [--rounds 5] [--seconds 1.0] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fixed_base import measure, write_out  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2t", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--curves", default="secp256k1,p256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import elliptic_amd
    T, B = 1 << a.log2t, 32
    ctx = elliptic_amd.Context(0)
    out = []
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")  # noqa: E731
    for curve in a.curves.split(","):
        rng = np.random.default_rng(13)
        k = rng.integers(0, 256, (T, B), dtype=np.uint8)
        seed = rng.integers(0, 256, (T, B), dtype=np.uint8)
        seed[:, 0] &= 0x7F
        pts, inf = ctx.mul_fixed(curve, seed)
        assert not inf.any()
        dk, dp = torch.from_numpy(k).cuda(), torch.from_numpy(pts).cuda()
        lo = min(10, a.log2t - 1)
        for n, m in ((T // 2, 2), (T // 8, 8), (1 << lo, T >> lo), (1, T)):
            def emit(row, curve=curve, n=n, m=m):
                row.update(curve=curve, n=n, m=m)
                print(json.dumps(row), flush=True)
                out.append(row)

            P = m // 2
            sk, sp = dk.view(n, m, B), dp.view(n, m, 2 * B)
            res = (u8(n, 2 * B), u8(n))
            # the baseline's operands, pair-major: partial sum q of sum j is row q n + j
            pk = dk.view(n, P, 2, B).permute(2, 1, 0, 3).contiguous().view(2, P * n, B)
            pp = dp.view(n, P, 2, 2 * B).permute(2, 1, 0, 3).contiguous().view(2, P * n, 2 * B)
            part = [(u8(P * n, 2 * B), u8(P * n)), (u8(max(P // 2, 1) * n, 2 * B), u8(max(P // 2, 1) * n))]
            last = [None]

            def new():
                ctx.mul_sum(curve, sk, sp, out=res)

            def base():
                ctx.mul_add2_dev(curve, pk[0], pp[0], pk[1], pp[1], part[0][0], part[0][1])
                src, ln = 0, P
                while ln > 1:
                    h = ln // 2
                    xy, f = part[src]
                    oxy, of = part[1 - src]
                    ctx.point_add_dev(curve, xy[:h * n], xy[h * n:2 * h * n], oxy[:h * n], of[:h * n],
                                      inf1=f[:h * n], inf2=f[h * n:2 * h * n])
                    src, ln = 1 - src, h
                last[0] = part[src]

            new(), base()
            torch.cuda.synchronize()
            assert torch.equal(res[0], last[0][0][:n]) and torch.equal(res[1], last[0][1][:n]), (curve, n, m)
            emit({"row": "check", "outputs_equal": True, "at_infinity": int(res[1].sum())})
            measure([("mul_sum", new), ("mul_add2 + point_add", base), ("mul_add2 + point_add (repeat)", base)], n * m, a, emit)
            by = {r_["row"]: r_["items_per_s"] for r_ in out
                  if (r_.get("curve"), r_.get("n"), r_.get("m")) == (curve, n, m) and "items_per_s" in r_}
            b1, b2 = by["mul_add2 + point_add"], by["mul_add2 + point_add (repeat)"]
            emit({"row": "ratios", "mul_sum_over_baseline": round(by["mul_sum"] / b1, 3),
                  "baseline_repeat_over_baseline": round(b2 / b1, 3)})
            del pk, pp, part
        # one small call, synchronised each time: what a caller with one sum waits for
        one = (u8(1, 2 * B), u8(1))
        calls = {"mul_sum (1, 2)": lambda: ctx.mul_sum(curve, dk[:2].view(1, 2, B), dp[:2].view(1, 2, 2 * B), out=one),
                 "mul_sum (1, 8)": lambda: ctx.mul_sum(curve, dk[:8].view(1, 8, B), dp[:8].view(1, 8, 2 * B), out=one),
                 "mul_add2_dev n = 1": lambda: ctx.mul_add2_dev(curve, dk[:1], dp[:1], dk[1:2], dp[1:2], one[0], one[1])}
        for name, fn in calls.items():
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(200):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            ts.sort()
            row = {"row": "latency " + name, "curve": curve, "median_us": round(ts[100] * 1e6, 1), "p10_us": round(ts[20] * 1e6, 1),
                   "p90_us": round(ts[180] * 1e6, 1)}
            print(json.dumps(row), flush=True)
            out.append(row)
    ctx.close()
    write_out(a, out)


if __name__ == "__main__":
    main()
