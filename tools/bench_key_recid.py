#!/usr/bin/env python3
"""Throughput of ellgpu_ecdsa_recid (EC#getKeyRecoveryParam in one pass) on secp256k1 and p256,
device-resident buffers, HIP-event timing.  Developer tool (GPU box).

Per curve, 2^--log2n signatures made by the engine's own ecdsa_sign over random 32-byte hashes, keys
and nonces, one item in 16 tampered with (a bit of s).  In one process, on the same items:
  ecdsa_recid                   the new call;
  ecdsa_verify_dev              the same double-scalar product behind EC#verify's front and comparison;
  recover j = 0, j = 1 + compare
                                the only way without the call: ellgpu_ecdsa_recover_dev for j = 0 and
                                for j = 1, each result compared with the key on the device.  (The
                                second candidates j = 2, 3 are left out: they exist for about one r in
                                2^128 on these curves, and the reference's loop asks for them only
                                where both of these fail -- here the tampered sixteenth.)
Before anything is timed the ids of the new call are compared with the ids ecdsa_sign returned and
with what the two recoveries find.  Rows are warmed up, then timed for at least --seconds of
back-to-back calls, --rounds times, alternating inside a round so that drift is shared; reported:
the median round in items/s and the spread (min .. max).  One JSON line per row, also appended to --out.

    python tools/bench_key_recid.py [--log2n 20] [--rounds 5] [--seconds 1.0] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fixed_base import measure, write_out  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--curves", default="secp256k1,p256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import elliptic_amd
    n, B = 1 << a.log2n, 32
    ctx = elliptic_amd.Context(0)
    out = []
    for curve in a.curves.split(","):
        def emit(row, curve=curve):
            row.update(curve=curve, n=n)
            print(json.dumps(row), flush=True)
            out.append(row)

        rng = np.random.default_rng(11)
        draw = lambda: rng.integers(0, 256, (n, B), dtype=np.uint8)  # noqa: E731
        h, priv, nonces = draw(), draw(), draw()
        priv[:, 0] &= 0x7F                                           # below n on both curves
        nonces[:, 0] &= 0x7F
        pub, inf = ctx.mul_fixed(curve, priv)
        r, s, rec, ok = ctx.ecdsa_sign(curve, h, priv, nonces)
        assert not inf.any() and ok.all()
        bad = np.arange(n) % 16 == 7
        s[bad, B - 1] ^= 1
        dh, dr, ds, dpub = (torch.from_numpy(x).cuda() for x in (h, r, s, pub))
        rid, st, vok = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(3))
        j = [torch.full((n,), v, dtype=torch.uint8, device="cuda") for v in (0, 1)]
        xy = [torch.zeros((n, 2 * B), dtype=torch.uint8, device="cuda") for _ in range(2)]
        rst = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(2)]
        found = torch.zeros(n, dtype=torch.uint8, device="cuda")
        c0, c1, c255 = (torch.full((n,), v, dtype=torch.uint8, device="cuda") for v in (0, 1, 255))

        def recid():
            ctx.ecdsa_recid(curve, dh, dr, ds, dpub, out=(rid, st))

        def verify():
            ctx.ecdsa_verify_dev(curve, dh, dr, ds, dpub, vok)

        def two_recoveries():
            for k in (0, 1):
                ctx.ecdsa_recover_dev(curve, dh, dr, ds, j[k], xy[k], rst[k])
            m0 = (xy[0] == dpub).all(dim=1) & (rst[0] == 0)
            m1 = (xy[1] == dpub).all(dim=1) & (rst[1] == 0)
            found.copy_(torch.where(m0, c0, torch.where(m1, c1, c255)))

        recid(), verify(), two_recoveries()
        torch.cuda.synchronize()
        rid_h, st_h, f_h = rid.cpu().numpy(), st.cpu().numpy(), found.cpu().numpy()
        good = ~bad
        assert (st_h[good] == 0).all() and (rid_h[good] == rec[good]).all() and (f_h[good] == rec[good]).all()
        assert (st_h[bad] == 1).all() and (rid_h[bad] == 0).all() and (f_h[bad] == 255).all()
        assert (vok.cpu().numpy() == good).all()
        emit({"row": "check", "ids_equal_ecdsa_sign": True, "tampered": int(bad.sum())})
        measure([("ecdsa_recid", recid), ("ecdsa_verify_dev", verify), ("recover j=0, j=1 + compare", two_recoveries)],
                n, a, emit)
        by = {r_["row"]: r_ for r_ in out if r_.get("curve") == curve and "items_per_s" in r_}
        emit({"row": "ratios", "recid_over_two_recoveries": round(by["ecdsa_recid"]["items_per_s"] / by["recover j=0, j=1 + compare"]["items_per_s"], 3),
              "recid_over_verify": round(by["ecdsa_recid"]["items_per_s"] / by["ecdsa_verify_dev"]["items_per_s"], 3)})
    ctx.close()
    write_out(a, out)


if __name__ == "__main__":
    main()
