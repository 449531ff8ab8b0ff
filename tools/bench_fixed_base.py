#!/usr/bin/env python3
"""Throughput of the fixed-base tables of caller-chosen points (ellgpu_base_define, ellgpu_mul_base,
ellgpu_mul_base2) on one curve, device-resident buffers, HIP-event timing.  Developer tool (GPU box).

In one process, on the same scalars:
  mul_base at each table width (a point H that is not G), and on G by coordinates at the width of
  the curve's own table -- the same kernel over an equally sized table as mul_fixed, so the two
  must agree within their spread;
  mul_var with the point repeated (what a caller paid before), mul_fixed;
  mul_base2(G alias, H) against mul_add2(k1, NULL -> G, k2, H);
  milliseconds per base_define per width (table build, one shot each).
Every row is warmed up, then timed for at least --seconds of back-to-back calls, --rounds times;
the rows alternate inside a round so that drift is shared.  Reported: the median round in items/s
and the spread (min .. max) over the rounds.  One JSON line per row, also appended to --out.

    python tools/bench_fixed_base.py [--curve secp256k1] [--log2n 20] [--rounds 5] [--seconds 1.0] [--out FILE]

--edwards: the Edwards handles of ellgpu_ed_base_define instead, on ed25519 (a caller's point at the
comb's own width) and on Curve1174 as a user-defined domain (8 and 16 bits): mul_base per width beside
mul_var with the point repeated, mul_base2(G, H) beside mul_add2 with both points repeated, and the
milliseconds per define.  mul_var and mul_add2 on these ids are kernels this feature left as they
were, so their rows are the earlier commit's figures on the same device, in the same process.

--verify: ellgpu_ecdsa_verify_base.  On secp256k1 and p256 the key's table at 8, 16 and 22 bits
(G's table as it stands), beside ellgpu_ecdsa_verify on the same items with the key repeated per item
(the baseline: the variable-base ladder) and mul_base2 over the same two tables (the ceiling the two
walks set: no scalar-field prep, but a normalisation); on p384 and brainpoolP256r1 (a user-defined
domain) the one width they have.  The items are random hashes with random r and s below 2^(bits - 1),
so every item is in range and walks both tables; almost every verdict is 0, which costs the x test
its second candidate.  After the timed rows, per curve: the share of ecdsa_prep in the device time of
one more ecdsa_verify_base call (ellgpu_ctx_get_timing).

--eddsa: ellgpu_eddsa_verify_base on ed25519.  Signatures of one signer over 32-byte messages at a
uniform stride (made by the engine's own eddsa_sign), about one item in 16 tampered with; beside
ellgpu_eddsa_verify_dev on the same items with the encoded key repeated per item (the baseline: the
decode of A, the window table and the ladder per item) and ed25519 mul_base2 over the same two tables
(the ceiling the two walks set: no hash, no decode of R, but a normalisation).  The verdicts of the
two verifies are compared before anything is timed.  Then the same two verifies at 200-byte messages:
what the longer hash costs."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curve", default="secp256k1")
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--edwards", action="store_true", help="the Edwards handles (ed25519, Curve1174) instead of --curve")
    ap.add_argument("--verify", action="store_true", help="ellgpu_ecdsa_verify_base beside ecdsa_verify and mul_base2")
    ap.add_argument("--eddsa", action="store_true", help="ellgpu_eddsa_verify_base beside eddsa_verify and ed25519 mul_base2")
    a = ap.parse_args()
    if a.eddsa:
        return main_eddsa(a)
    if a.edwards:
        return main_edwards(a)
    if a.verify:
        return main_verify(a)
    import numpy as np
    import torch
    import elliptic_amd
    import fixed_base_checks as FB
    spec = FB.spec_of(a.curve)
    B, n = spec["B"], 1 << a.log2n
    ctx = elliptic_amd.Context(0)
    G, H = FB.bases_of(spec)[0], FB.bases_of(spec)[3]
    rng = np.random.default_rng(7)
    k1 = torch.from_numpy(rng.integers(0, 256, (n, B), dtype=np.uint8)).cuda()
    k2 = torch.from_numpy(rng.integers(0, 256, (n, B), dtype=np.uint8)).cuda()
    hxy = torch.from_numpy(np.tile(np.frombuffer(FB.xy_bytes(H, B), np.uint8), (n, 1))).cuda()
    xy = torch.zeros((n, 2 * B), dtype=torch.uint8, device="cuda")
    inf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = []

    def emit(row):
        row.update(curve=a.curve, n=n)
        print(json.dumps(row), flush=True)
        out.append(row)

    ctx.mul_fixed_dev(a.curve, k1, xy, inf)                     # the curve's own table
    torch.cuda.synchronize()
    gbits = ctx.comb_bits(a.curve)
    widths = [4, 8, 12, 16, 22] if a.curve in FB.SIGNED else [8]
    bases = {}
    for w in widths:
        t = time.perf_counter()
        bases[w] = ctx.define_base(a.curve, FB.xy_bytes(H, B), w)
        torch.cuda.synchronize()
        emit({"row": "base_define", "width": w, "ms": round((time.perf_counter() - t) * 1e3, 2),
              "table_bytes": ctx.base_info(bases[w])[2]})
    g_coords = ctx.define_base(a.curve, FB.xy_bytes(G, B), gbits)
    alias = ctx.define_base(a.curve)
    dflt = 16 if 16 in bases else widths[0]
    rows = [("mul_base w=%d" % w, lambda w=w: ctx.mul_base(bases[w], k1, out=(xy, inf))) for w in widths]
    rows += [("mul_base G by coordinates w=%d" % gbits, lambda: ctx.mul_base(g_coords, k1, out=(xy, inf))),
             ("mul_fixed (w=%d)" % gbits, lambda: ctx.mul_fixed_dev(a.curve, k1, xy, inf)),
             ("mul_var, point repeated", lambda: ctx.mul_var_dev(a.curve, k1, hxy, xy, inf)),
             ("mul_base2(G alias, H w=%d)" % dflt, lambda: ctx.mul_base2(alias, bases[dflt], k1, k2, out=(xy, inf))),
             ("mul_add2(k1, G, k2, H)", lambda: ctx.mul_add2_dev(a.curve, k1, None, k2, hxy, xy, inf))]
    measure(rows, n, a, emit)
    ctx.close()
    write_out(a, out)


def write_out(a, out):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for row in out:
                f.write(json.dumps(row) + "\n")


def measure(rows, n, a, emit):
    import torch
    reps = {}
    for name, fn in rows:                                       # warm-up, and calls per timed stretch
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        reps[name] = max(3, int(a.seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    rates = {name: [] for name, _ in rows}
    for _ in range(a.rounds):
        for name, fn in rows:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(reps[name]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            rates[name].append(n * reps[name] / (e0.elapsed_time(e1) * 1e-3))
    for name, _ in rows:
        r = sorted(rates[name])
        emit({"row": name, "items_per_s": round(r[len(r) // 2]), "min": round(r[0]), "max": round(r[-1]),
              "rounds": a.rounds, "calls_per_round": reps[name]})


def main_edwards(a):
    import numpy as np
    import torch
    import elliptic_amd
    import fixed_base_checks as FB
    import fixed_base_ed_checks as FE
    n = 1 << a.log2n
    ctx = elliptic_amd.Context(0)
    rng = np.random.default_rng(7)
    k1 = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
    k2 = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
    xy = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    inf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = []
    for name, widths in (("ed25519", [16]), ("curve1174", [8, 16])):
        spec = FE.spec_of(name)
        cid = FE.curve_id(ctx, spec)
        G, H = FE.bases_of(spec)[0], FE.bases_of(spec)[3]

        def emit(row, name=name):
            row.update(curve=name, n=n)
            print(json.dumps(row), flush=True)
            out.append(row)

        gxy = torch.from_numpy(FE.tiled(G, n)).cuda()
        hxy = torch.from_numpy(FE.tiled(H, n)).cuda()
        ctx.mul_var_dev(cid, k1, hxy, xy, inf)                  # (ed25519: the curve's own table, once)
        torch.cuda.synchronize()
        bh, bg = {}, {}
        for w in widths:
            t = time.perf_counter()
            bh[w] = ctx.define_ed_base(cid, FB.xy_bytes(H, 32), w)
            torch.cuda.synchronize()
            emit({"row": "ed_base_define", "width": w, "ms": round((time.perf_counter() - t) * 1e3, 2),
                  "table_bytes": ctx.base_info(bh[w])[2]})
            bg[w] = ctx.define_ed_base(cid, FB.xy_bytes(G, 32), w)
        rows = [("mul_base w=%d" % w, lambda w=w: ctx.mul_base(bh[w], k1, out=(xy, inf))) for w in widths]
        rows += [("mul_var, point repeated", lambda: ctx.mul_var_dev(cid, k1, hxy, xy, inf))]
        rows += [("mul_base2(G, H) w=%d" % w, lambda w=w: ctx.mul_base2(bg[w], bh[w], k1, k2, out=(xy, inf))) for w in widths]
        rows += [("mul_add2(k1, G, k2, H), points repeated", lambda: ctx.mul_add2_dev(cid, k1, gxy, k2, hxy, xy, inf))]
        measure(rows, n, a, emit)
        for h in set(list(bh.values()) + list(bg.values())):
            ctx.release_base(h)
    ctx.close()
    write_out(a, out)


def main_verify(a):
    import numpy as np
    import torch
    import elliptic_amd
    import verify_base_checks as VB
    ctx = elliptic_amd.Context(0)
    rng = np.random.default_rng(11)
    out = []
    for name, widths, log2n in (("secp256k1", [8, 16, 22], a.log2n), ("p256", [8, 16, 22], a.log2n),
                                ("p384", [8], min(a.log2n, 18)), ("brainpoolP256r1", [8], a.log2n)):
        spec = VB.spec_of(name)
        B, n = spec["B"], 1 << log2n
        cid = VB.curve_id(ctx, spec)
        Q = VB.keys_of(spec)[3][1]

        def emit(row, name=name, n=n):
            row.update(curve=name, n=n)
            print(json.dumps(row), flush=True)
            out.append(row)

        def scalars():
            v = rng.integers(0, 256, (n, B), dtype=np.uint8)
            v[:, 0] &= 0x7F                                    # below 2^(8 B - 1) < n: in range
            return torch.from_numpy(v).cuda()

        h = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
        r, s, k1, k2 = scalars(), scalars(), scalars(), scalars()
        pub = torch.from_numpy(np.tile(np.frombuffer(VB.xy_bytes(Q, B), np.uint8), (n, 1))).cuda()
        ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        ok2 = torch.zeros(n, dtype=torch.uint8, device="cuda")
        xy = torch.zeros((n, 2 * B), dtype=torch.uint8, device="cuda")
        inf = torch.zeros(n, dtype=torch.uint8, device="cuda")
        alias = ctx.define_base(cid)
        keys = {w: ctx.define_base(cid, VB.xy_bytes(Q, B), w) for w in widths}
        ctx.ecdsa_verify_dev(cid, h, r, s, pub, ok2)
        for w in widths:                                        # the same verdicts, before anything is timed
            ctx.ecdsa_verify_base(keys[w], h, r, s, out=(ok,))
            torch.cuda.synchronize()
            assert torch.equal(ok, ok2), (name, w)
        gbits = ctx.base_info(alias)[1]
        rows = [("ecdsa_verify_base key w=%d (G w=%d)" % (w, gbits), lambda w=w: ctx.ecdsa_verify_base(keys[w], h, r, s, out=(ok,)))
                for w in widths]
        rows += [("ecdsa_verify, key repeated", lambda: ctx.ecdsa_verify_dev(cid, h, r, s, pub, ok2))]
        rows += [("mul_base2(G alias, key w=%d)" % w, lambda w=w: ctx.mul_base2(alias, keys[w], k1, k2, out=(xy, inf))) for w in widths]
        measure(rows, n, a, emit)
        base = next(x["items_per_s"] for x in out if x["curve"] == name and x["row"].startswith("ecdsa_verify,"))
        for x in out:
            if x["curve"] == name and x["row"].startswith("ecdsa_verify_base"):
                x["ratio_to_ecdsa_verify"] = round(x["items_per_s"] / base, 3)
        dflt = 16 if 16 in keys else widths[0]
        ctx.set_timing(True)
        ctx.ecdsa_verify_base(keys[dflt], h, r, s, out=(ok,))
        torch.cuda.synchronize()
        t = ctx.get_timing()
        ctx.set_timing(False)
        prep, walk = t.get("ecdsa_prep", (0, 0.0))[1], t.get("ecdsa_base", (0, 0.0))[1]
        emit({"row": "kernel times of one ecdsa_verify_base call, key w=%d" % dflt, "ecdsa_prep_ms": round(prep, 4),
              "ecdsa_base_ms": round(walk, 4), "prep_share": round(prep / (prep + walk), 3) if prep + walk else None})
        for hdl in list(keys.values()) + [alias]:
            ctx.release_base(hdl)
    ctx.close()
    write_out(a, out)


def main_eddsa(a):
    import numpy as np
    import torch
    import elliptic_amd
    from oracle import ec_oracle as O
    n = 1 << a.log2n
    ctx = elliptic_amd.Context(0)
    rng = np.random.default_rng(13)
    out = []

    def emit(row):
        row.update(curve="ed25519", n=n)
        print(json.dumps(row), flush=True)
        out.append(row)

    secret = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    A = O.get_curve("ed25519").g.mul(O.eddsa_keypair(O.get_curve("ed25519"), secret)[0])
    x, y = A.normalized()
    enc = O.ed_encode_point(A)
    key = ctx.define_ed_base("ed25519", x.to_bytes(32, "big") + y.to_bytes(32, "big"))
    alias = ctx.define_ed_base("ed25519")
    secrets = torch.from_numpy(np.tile(np.frombuffer(secret, np.uint8), (n, 1))).cuda()
    pubs = torch.from_numpy(np.tile(np.frombuffer(enc, np.uint8), (n, 1))).cuda()
    k1 = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
    k2 = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
    xy = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    inf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ok, err, ok2, err2 = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(4))
    rates = {}
    for mlen in (32, 200):
        msgs = torch.from_numpy(rng.integers(0, 256, (n, mlen), dtype=np.uint8)).cuda()
        sigs = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
        ctx.eddsa_sign_dev(secrets, msgs, mlen, sigs)
        torch.cuda.synchronize()
        sigs[::16, 33] ^= 1                                     # about one item in 16: a bit of S
        ctx.eddsa_verify_dev(msgs, mlen, sigs, pubs, ok2, err2)
        ctx.eddsa_verify_base(key, msgs, sigs, out=(ok, err))
        torch.cuda.synchronize()
        assert torch.equal(ok, ok2) and torch.equal(err, err2), mlen
        accepted = int(ok.sum())
        assert accepted == n - (n + 15) // 16 and not bool(err.any()), (accepted, n)
        rows = [("eddsa_verify_base, %d-byte messages" % mlen, lambda: ctx.eddsa_verify_base(key, msgs, sigs, out=(ok, err))),
                ("eddsa_verify, key repeated, %d-byte messages" % mlen, lambda: ctx.eddsa_verify_dev(msgs, mlen, sigs, pubs, ok2, err2))]
        if mlen == 32:
            rows.append(("mul_base2(G alias, key)", lambda: ctx.mul_base2(alias, key, k1, k2, out=(xy, inf))))
        measure(rows, n, a, emit)
        for x in out:
            rates[x["row"]] = x.get("items_per_s")
    b32, v32 = rates["eddsa_verify_base, 32-byte messages"], rates["eddsa_verify, key repeated, 32-byte messages"]
    b200, v200 = rates["eddsa_verify_base, 200-byte messages"], rates["eddsa_verify, key repeated, 200-byte messages"]
    emit({"row": "ratios", "base_to_verify_32": round(b32 / v32, 3), "base_to_mul_base2_32": round(b32 / rates["mul_base2(G alias, key)"], 3),
          "base_to_verify_200": round(b200 / v200, 3),
          "share_of_the_longer_hash_in_a_200_byte_call": round(1 - b200 / b32, 3)})
    ctx.release_base(key)
    ctx.release_base(alias)
    ctx.close()
    write_out(a, out)


if __name__ == "__main__":
    main()
