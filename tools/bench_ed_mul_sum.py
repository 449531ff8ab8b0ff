#!/usr/bin/env python3
"""Throughput of ellgpu_ed_mul_sum (n sums of m terms k * P on an Edwards curve) on ed25519 and
Curve1174 (a user-defined Edwards domain), device-resident buffers, HIP-event timing.  Developer tool
(GPU box); tools/bench_mul_sum.py on the Edwards curves.

2^--log2t terms in all, as (n, m) = (T / 2, 2), (T / 8, 8), (2^10, T / 2^10) and (1, T): random
scalars on random multiples of G.  In one process, on the same terms:
  ed_mul_sum            the new call;
  mul_add2 + point_add  the only way without it: ellgpu_mul_add2_dev over the pairs of neighbouring
                        terms, then ceil(log2(m / 2)) passes of ellgpu_point_add_dev over the halves
                        of the partial sums, each pass with its own normalisation (the partial sums
                        are laid out pair-major so that every pass reads two contiguous halves);
  ... (repeat)          the same baseline again: the difference of the two is the run-to-run spread.
Before anything is timed the outputs of the two are compared at the timed size.  Rows are warmed up,
then timed for at least --seconds of back-to-back calls, --rounds times, alternating inside a round
so that drift is shared; reported: the median round in terms/s and the spread (min .. max).  One JSON
line per row, also appended to --out.

    python tools/bench_ed_mul_sum.py [--log2t 20] [--rounds 5] [--seconds 1.0] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fixed_base import measure, write_out  # noqa: E402

P1174 = 2 ** 251 - 9
CURVES = {
    "ed25519": None,
    "curve1174": dict(p=P1174, a=1, d=P1174 - 1174, n=2 ** 249 - 11332719920821432534773113288178349711,
                      gx=1582619097725911541954547006453739763381091388846394833492296309729998839514,
                      gy=3037538013604154504764115728651437646519513534305223422754827055689195992590),
}
ED25519_G = (15112221349535400772501151409588531511454012693041857206046113283949847762202,
             46316835694926478169428394003475163141307993866256225615783033603165251855960)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2t", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--curves", default="ed25519,curve1174")
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
        c = CURVES[curve]
        cid = curve if c is None else ctx.define_edwards_domain(c["p"], c["a"], c["d"], c["n"], c["gx"], c["gy"])
        g = ED25519_G if c is None else (c["gx"], c["gy"])
        rng = np.random.default_rng(13)
        k = rng.integers(0, 256, (T, B), dtype=np.uint8)
        seed = rng.integers(0, 256, (T, B), dtype=np.uint8)
        seed[:, 0] &= 0x0F
        gxy = np.frombuffer(g[0].to_bytes(B, "big") + g[1].to_bytes(B, "big"), np.uint8)
        pts, inf = ctx.mul_var(cid, seed, np.tile(gxy, (T, 1)))
        assert not (inf == 2).any()
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
                ctx.ed_mul_sum(cid, sk, sp, out=res)

            def base():
                ctx.mul_add2_dev(cid, pk[0], pp[0], pk[1], pp[1], part[0][0], part[0][1])
                src, ln = 0, P
                while ln > 1:
                    h = ln // 2
                    xy, f = part[src]
                    oxy, of = part[1 - src]
                    ctx.point_add_dev(cid, xy[:h * n], xy[h * n:2 * h * n], oxy[:h * n], of[:h * n],
                                      inf1=f[:h * n], inf2=f[h * n:2 * h * n])
                    src, ln = 1 - src, h
                last[0] = part[src]

            new(), base()
            torch.cuda.synchronize()
            assert torch.equal(res[0], last[0][0][:n]) and torch.equal(res[1], last[0][1][:n]), (curve, n, m)
            emit({"row": "check", "outputs_equal": True, "identities": int((res[1] == 1).sum())})
            measure([("ed_mul_sum", new), ("mul_add2 + point_add", base), ("mul_add2 + point_add (repeat)", base)], n * m, a, emit)
            by = {r_["row"]: r_["items_per_s"] for r_ in out
                  if (r_.get("curve"), r_.get("n"), r_.get("m")) == (curve, n, m) and "items_per_s" in r_}
            b1, b2 = by["mul_add2 + point_add"], by["mul_add2 + point_add (repeat)"]
            emit({"row": "ratios", "ed_mul_sum_over_baseline": round(by["ed_mul_sum"] / b1, 3),
                  "baseline_repeat_over_baseline": round(b2 / b1, 3)})
            del pk, pp, part
    ctx.close()
    write_out(a, out)


if __name__ == "__main__":
    main()
