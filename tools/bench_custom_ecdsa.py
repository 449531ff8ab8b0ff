#!/usr/bin/env python3
"""ECDSA verify throughput on a user-defined domain (brainpoolP256r1 through
ellgpu_curve_define_short_domain), device-resident buffers, HIP-event timing; beside it, on the
same curve and keys, k*G through the domain's comb and the two-point mul_add2 of a plain
user-defined curve (the comparison point: what a verify cost before the domain existed).
Developer tool (GPU box).

The signatures are drawn at random with 1 <= r, s < n over keys on the curve, so that every item
runs the whole verify (the work does not depend on the verdict).

    [ELLGPU_LIB=variant.so] python tools/bench_custom_ecdsa.py [log2 n ...]   (default: 18 20)

--wire: the same signatures as DER records under compressed SEC1 keys through
custom_verify_wire_dev, next to the raw-form ecdsa_verify_dev over the decoded rows, in one run --
on brainpoolP256r1 (square root: one exponentiation) and secp224k1 (Tonelli-Shanks, p - 1 = q 2^2);
and the key decoding alone (custom_decode_points_dev), which is where the square root is.

    python tools/bench_custom_ecdsa.py --wire [log2 n ...]                     (default: 18)

--recover: public-key recovery (custom_recover_dev) next to the raw-form ecdsa_verify_dev on the
same domain, same r and s, in one run -- on brainpoolP256r1 and secp224k1.  r is the x of a point
k G (so every item has its square root and runs the whole recovery; status 0 is asserted), s is
random, the verify's keys are random points.  Recovery is one square root and one batched
inversion more than a verify; "kernels_ms" are the launches of one recovery call
(ellgpu_ctx_set_timing).

    python tools/bench_custom_ecdsa.py --recover [log2 n ...]                  (default: 16 18)

--sign: signing on the domain (brainpoolP256r1) -- custom_sign_dev over supplied nonces and
custom_sign_det_dev with its own HmacDRBG (SHA-256) nonces -- beside the verify, the recovery and
k*G (mul_fixed_dev) of the same domain in the same run.  k*G is the floor no signature can beat
("sign_over_mul_fixed"); "sign_det_over_sign" is what the DRBG costs.  Every signature is
asserted accepted, the signatures of the deterministic call are then verified and their keys
recovered; "kernels_ms" are the launches of one custom_sign_det call.

    python tools/bench_custom_ecdsa.py --sign [log2 n ...]                     (default: 18 20)

--ecdh: the key side on the domain (brainpoolP256r1), in one run: custom_derive_dev over raw peer
keys, custom_derive_wire_dev over the same keys compressed (02 / 03 || x: the square root on top),
mul_var_dev on the same scalars and points as the yardstick -- the raw derive adds one equation test
in front and drops the y behind ("derive_over_mul_var") -- and custom_validate_dev with the order
test (one n * P per item).  Every item is asserted status 0, the two derives equal to mul_var's x;
"kernels_ms" are the launches of one custom_derive_wire call.

    python tools/bench_custom_ecdsa.py --ecdh [log2 n ...]                     (default: 18 20)

--mont: user-defined Montgomery curves, on curve25519 written out by hand (c25519_user of
tests/golden/custom_mont.json), in one run: custom_mont_ladder_dev and custom_mont_derive_dev beside
the preset's x25519_ladder_dev on the same rows (one-limb a24, special-form prime) and beside
mul_var_dev on w25519_like, the same curve in short Weierstrass form through the run-time field
(the short custom ladder).  Device-resident buffers, HIP-event timing; the four calls alternate
over three rounds and each figure is the median round.  The custom ladder is asserted equal to the
preset's item for item and every derive status 0; "kernels_ms" are the launches of one
custom_mont_derive call.

    python tools/bench_custom_ecdsa.py --mont [log2 n ...]                     (default: 18 20)

--edwards: the key side of user-defined Edwards curves, on Curve1174 and on twisted_a4 (2^255 - 19)
of tests/golden/custom_ed.json, in one run: custom_ed_decompress_dev (pointFromY), custom_ed_validate_dev
without and with the order test, custom_ed_derive_dev and custom_ed_derive_wire_dev (compressed
keys) beside mul_var_dev on the same id and rows.  Device-resident buffers, HIP-event timing; the calls
alternate over three rounds and each figure is the median round.  Every status is asserted 0 and
the two derives equal to mul_var's x; "kernels_ms" are the launches of one custom_ed_derive_wire call.

    python tools/bench_custom_ecdsa.py --edwards [log2 n ...]                  (default: 18 20)

--ed-ecdsa: ECDSA on the Edwards domain over Curve1174 (ellgpu_custom_ed_verify, _sign, _sign_det)
beside mul_add2 (both points given) and mul_var on the plain curve over the same (p, a, d):
verifies/s and signatures/s, and the kernel comparison the shared-table ladder answers to -- the
median of five timed calls (Context.set_timing / get_timing, after two warm-up calls) of edc_ecdsa_ladder against
edc_mul_add2, with the five values of each.

    python tools/bench_custom_ecdsa.py --ed-ecdsa [log2 n ...]                 (default: 16)"""
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


def run_wire(ctx, spec, n):
    import numpy as np
    import torch
    import bench
    import custom_domain_checks as CD
    import custom_wire_checks as CW
    cid = CD.define(ctx, spec)
    nn = CD.I(spec["n"])
    pl = (CD.I(spec["p"]).bit_length() + 7) // 8
    keep = nn.bit_length() - 1                      # scalars below 2^(bitLength(n) - 1) < n
    def below_n(tag):
        a = bench.xof("custom-wire:%s:%s" % (spec["name"], tag), n * 32).reshape(n, 32).copy()
        a[:, :32 - (keep + 7) // 8] = 0
        if keep % 8:
            a[:, 32 - (keep + 7) // 8] &= (1 << (keep % 8)) - 1
        a[:, 31] |= 1
        return a
    d, r, s = below_n("d"), below_n("r"), below_n("s")
    q, inf = ctx.mul_fixed(cid, d)
    assert not inf.any()
    h = bench.xof("custom-wire:h", n * 32).reshape(n, 32).copy()
    keys = np.concatenate([(2 + (q[:, 63] & 1))[:, None], q[:, 32 - pl:32]], axis=1).astype(np.uint8)
    sigs = [CW.der_sig(int.from_bytes(bytes(r[i]), "big"), int.from_bytes(bytes(s[i]), "big")) for i in range(n)]
    der, lens = ctx._pack_records(sigs)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dh, dr, ds, dq, dk, dder = t(h), t(r), t(s), t(q), t(keys), t(der)
    dlens = t(lens.view(np.int32))
    ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    ok2 = torch.zeros(n, dtype=torch.uint8, device=dev)
    err = torch.zeros(n, dtype=torch.uint8, device=dev)
    dxy = torch.zeros(n, 64, dtype=torch.uint8, device=dev)
    dst = torch.zeros(n, dtype=torch.uint8, device=dev)
    out = {"lib": os.path.basename(os.environ.get("ELLGPU_LIB", "libellgpu.so")), "curve": spec["name"], "n": n,
           "p_mod_4": CD.I(spec["p"]) % 4}
    for name, fn in (("raw_verify", lambda: ctx.ecdsa_verify_dev(cid, dh, dr, ds, dq, ok)),
                     ("wire_verify", lambda: ctx.custom_verify_wire_dev(cid, dh, dder, dlens, dk, ok2, out_err=err)),
                     ("decode_keys", lambda: ctx.custom_decode_points_dev(cid, dk, dxy, dst))):
        ms = timed(fn)
        out[name + "_ms"] = round(ms, 3)
        out[name + "_M_per_s"] = round(n / ms / 1e3, 2)
    # the two forms answer alike, no key failed to decode, and the keys came back whole
    assert torch.equal(ok, ok2) and not err.any().item() and not dst.any().item() and torch.equal(dxy, dq)
    out["wire_over_raw"] = round(out["wire_verify_ms"] / out["raw_verify_ms"], 4)
    return out


def run_recover(ctx, spec, n):
    import numpy as np
    import torch
    import bench
    import custom_domain_checks as CD
    cid = CD.define(ctx, spec)
    nn = CD.I(spec["n"])
    keep = nn.bit_length() - 1                      # scalars below 2^(bitLength(n) - 1) < n
    def below_n(tag):
        a = bench.xof("custom-recover:%s:%s" % (spec["name"], tag), n * 32).reshape(n, 32).copy()
        a[:, :32 - (keep + 7) // 8] = 0
        if keep % 8:
            a[:, 32 - (keep + 7) // 8] &= (1 << (keep % 8)) - 1
        a[:, 31] |= 1
        return a
    d, k, s = below_n("d"), below_n("k"), below_n("s")
    q, inf = ctx.mul_fixed(cid, d)
    kg, inf2 = ctx.mul_fixed(cid, k)
    assert not inf.any() and not inf2.any()
    # r = x(k G) where that is below n (else r = 1: counted, and excluded from the status check)
    r = kg[:, :32].copy()
    big = np.array([int.from_bytes(bytes(x), "big") >= nn for x in r])
    r[big] = 0
    r[big, 31] = 1
    recid = (kg[:, 63] & 1).astype(np.uint8)
    h = bench.xof("custom-recover:h", n * 32).reshape(n, 32).copy()
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dh, dr, ds, dq, dj = t(h), t(r), t(s), t(q), t(recid)
    ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    dxy = torch.zeros(n, 64, dtype=torch.uint8, device=dev)
    dst = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    out = {"lib": os.path.basename(os.environ.get("ELLGPU_LIB", "libellgpu.so")), "curve": spec["name"], "n": n,
           "r_not_x": int(big.sum())}
    for name, fn in (("raw_verify", lambda: ctx.ecdsa_verify_dev(cid, dh, dr, ds, dq, ok)),
                     ("recover", lambda: ctx.custom_recover_dev(cid, dh, dr, ds, dj, dxy, dst))):
        ms = timed(fn)
        out[name + "_ms"] = round(ms, 3)
        out[name + "_M_per_s"] = round(n / ms / 1e3, 2)
    st = dst.cpu().numpy()
    assert (st[~big] == 0).all(), np.unique(st, return_counts=True)
    out["recover_over_verify"] = round(out["recover_ms"] / out["raw_verify_ms"], 4)
    ctx.set_timing(True)
    ctx.custom_recover_dev(cid, dh, dr, ds, dj, dxy, dst)
    torch.cuda.synchronize()
    out["kernels_ms"] = {name: round(ms, 4) for name, (cnt, ms) in ctx.get_timing().items()}
    ctx.set_timing(False)
    return out


def run_sign(ctx, spec, n):
    import numpy as np
    import torch
    import bench
    import custom_domain_checks as CD
    cid = CD.define(ctx, spec)
    nn = CD.I(spec["n"])
    keep = nn.bit_length() - 1                      # scalars below 2^(bitLength(n) - 1) < n
    def below_n(tag):
        a = bench.xof("custom-sign:%s:%s" % (spec["name"], tag), n * 32).reshape(n, 32).copy()
        a[:, :32 - (keep + 7) // 8] = 0
        if keep % 8:
            a[:, 32 - (keep + 7) // 8] &= (1 << (keep % 8)) - 1
        a[:, 31] |= 3                               # 1 < k
        return a
    d, k = below_n("d"), below_n("k")
    h = bench.xof("custom-sign:h", n * 32).reshape(n, 32).copy()
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    z = lambda *sh: torch.zeros(*sh, dtype=torch.uint8, device=dev)
    dh, dd, dk = t(h), t(d), t(k)
    r1, s1, j1, ok1 = z(n, 32), z(n, 32), z(n), z(n)
    r2, s2, j2, ok2 = z(n, 32), z(n, 32), z(n), z(n)
    dq, dinf, dxy, dst, ver = z(n, 64), z(n), z(n, 64), z(n), z(n)
    ctx.mul_fixed_dev(cid, dd, dq, dinf)
    out = {"lib": os.path.basename(os.environ.get("ELLGPU_LIB", "libellgpu.so")), "curve": spec["name"], "n": n}
    for name, fn in (("mul_fixed", lambda: ctx.mul_fixed_dev(cid, dd, dxy, dinf)),
                     ("sign", lambda: ctx.custom_sign_dev(cid, dh, dd, dk, r1, s1, j1, ok1, canonical=True)),
                     ("sign_det", lambda: ctx.custom_sign_det_dev(cid, dh, dd, r2, s2, j2, ok2, drbg_hash=0,
                                                                  canonical=True)),
                     ("verify", lambda: ctx.ecdsa_verify_dev(cid, dh, r2, s2, dq, ver)),
                     ("recover", lambda: ctx.custom_recover_dev(cid, dh, r2, s2, j2, dxy, dst))):
        ms = timed(fn)
        out[name + "_ms"] = round(ms, 3)
        out[name + "_M_per_s"] = round(n / ms / 1e3, 2)
    # every item signed; the deterministic signatures verify and give their keys back (32-byte
    # digests on a 256-bit n: recovery sees the digest the signature was made over)
    assert bool((ok1 == 1).all()) and bool((ok2 == 1).all()) and bool((ver == 1).all())
    if nn.bit_length() == 256:
        assert not dst.any().item() and torch.equal(dxy, dq)
    out["sign_over_mul_fixed"] = round(out["sign_ms"] / out["mul_fixed_ms"], 4)
    out["sign_det_over_mul_fixed"] = round(out["sign_det_ms"] / out["mul_fixed_ms"], 4)
    out["sign_det_over_sign"] = round(out["sign_det_ms"] / out["sign_ms"], 4)
    ctx.set_timing(True)
    ctx.custom_sign_det_dev(cid, dh, dd, r2, s2, j2, ok2, drbg_hash=0, canonical=True)
    torch.cuda.synchronize()
    out["kernels_ms"] = {name: round(ms, 4) for name, (cnt, ms) in ctx.get_timing().items()}
    ctx.set_timing(False)
    return out


def run_ecdh(ctx, spec, n):
    import numpy as np
    import torch
    import bench
    import custom_domain_checks as CD
    cid = CD.define(ctx, spec)
    nn = CD.I(spec["n"])
    pl = (CD.I(spec["p"]).bit_length() + 7) // 8
    keep = nn.bit_length() - 1                      # scalars below 2^(bitLength(n) - 1) < n
    def below_n(tag):
        a = bench.xof("custom-ecdh:%s:%s" % (spec["name"], tag), n * 32).reshape(n, 32).copy()
        a[:, :32 - (keep + 7) // 8] = 0
        if keep % 8:
            a[:, 32 - (keep + 7) // 8] &= (1 << (keep % 8)) - 1
        a[:, 31] |= 1
        return a
    d, k = below_n("d"), below_n("k")
    q, inf = ctx.mul_fixed(cid, d)                  # the peers' keys
    assert not inf.any()
    keys = np.concatenate([(2 + (q[:, 63] & 1))[:, None], q[:, 32 - pl:32]], axis=1).astype(np.uint8)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    z = lambda *sh: torch.full(sh, 9, dtype=torch.uint8, device=dev)
    dk, dq, dkeys = t(k), t(q), t(keys)
    x1, st1, x2, st2, err2, vst, mxy, minf = z(n, 32), z(n), z(n, 32), z(n), z(n), z(n), z(n, 64), z(n)
    out = {"lib": os.path.basename(os.environ.get("ELLGPU_LIB", "libellgpu.so")), "curve": spec["name"], "n": n}
    for name, fn in (("mul_var", lambda: ctx.mul_var_dev(cid, dk, dq, mxy, minf)),
                     ("derive", lambda: ctx.custom_derive_dev(cid, dk, dq, x1, st1)),
                     ("derive_wire", lambda: ctx.custom_derive_wire_dev(cid, dk, dkeys, x2, st2, err2)),
                     ("validate_order", lambda: ctx.custom_validate_dev(cid, dq, None, True, vst))):
        ms = timed(fn)
        out[name + "_ms"] = round(ms, 3)
        out[name + "_M_per_s"] = round(n / ms / 1e3, 2)
    assert not st1.any().item() and not st2.any().item() and not err2.any().item() and not vst.any().item()
    assert not minf.any().item() and torch.equal(x1, mxy[:, :32]) and torch.equal(x2, x1)
    out["derive_over_mul_var"] = round(out["derive_ms"] / out["mul_var_ms"], 4)
    out["derive_wire_over_derive"] = round(out["derive_wire_ms"] / out["derive_ms"], 4)
    out["validate_over_mul_var"] = round(out["validate_order_ms"] / out["mul_var_ms"], 4)
    ctx.set_timing(True)
    ctx.custom_derive_wire_dev(cid, dk, dkeys, x2, st2, err2)
    torch.cuda.synchronize()
    out["kernels_ms"] = {name: round(ms, 4) for name, (cnt, ms) in ctx.get_timing().items()}
    ctx.set_timing(False)
    return out


def run_mont(ctx, n):
    import numpy as np
    import torch
    import bench
    import custom_domain_checks as CD
    import custom_ecdh_checks as CE
    import custom_mont_checks as CM
    spec = CM.spec_of("c25519_user")
    cid = CM.define(ctx, spec)
    wspec = CE.spec_of("w25519_like")
    wid = CD.define(ctx, wspec)
    rnd = lambda tag: bench.xof("custom-mont:%s" % tag, n * 32).reshape(n, 32).copy()
    k, d = rnd("k"), rnd("d")
    d[:, 0] &= 0x0F                                  # the peers' keys: below the subgroup order of either form
    d[:, 31] |= 1
    base = np.zeros((n, 32), np.uint8)
    base[:, 31] = 9
    x, inf = ctx.custom_mont_ladder(cid, d, base)    # abscissae of the curve: x(d G)
    assert not inf.any()
    q, qinf = ctx.mul_fixed(wid, d)                  # the same keys on the short form
    assert not qinf.any()
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    z = lambda *sh: torch.full(sh, 9, dtype=torch.uint8, device=dev)
    dk, dx, dq = t(k), t(x), t(q)
    px, pinf, lx, linf, sx, sst, mxy, minf = z(n, 32), z(n), z(n, 32), z(n), z(n, 32), z(n), z(n, 64), z(n)
    calls = (("x25519_ladder", lambda: ctx.x25519_dev(dk, dx, px, pinf)),
             ("custom_mont_ladder", lambda: ctx.custom_mont_ladder_dev(cid, dk, dx, lx, linf)),
             ("custom_mont_derive", lambda: ctx.custom_mont_derive_dev(cid, dk, dx, sx, sst)),
             ("mul_var_w25519_like", lambda: ctx.mul_var_dev(wid, dk, dq, mxy, minf)))
    rounds = {name: [] for name, _ in calls}
    for _ in range(3):
        for name, fn in calls:
            rounds[name].append(timed(fn))
    out = {"lib": os.path.basename(os.environ.get("ELLGPU_LIB", "libellgpu.so")), "curve": spec["name"], "n": n}
    for name, _ in calls:
        ms = sorted(rounds[name])[1]
        out[name + "_ms"] = round(ms, 3)
        out[name + "_ms_rounds"] = [round(v, 3) for v in rounds[name]]
        out[name + "_M_per_s"] = round(n / ms / 1e3, 2)
    assert torch.equal(lx, px) and torch.equal(linf, pinf) and not linf.any().item()
    assert not sst.any().item() and torch.equal(sx, lx) and not minf.any().item()
    out["custom_ladder_over_preset"] = round(out["custom_mont_ladder_ms"] / out["x25519_ladder_ms"], 4)
    out["custom_derive_over_custom_ladder"] = round(out["custom_mont_derive_ms"] / out["custom_mont_ladder_ms"], 4)
    out["short_mul_var_over_custom_ladder"] = round(out["mul_var_w25519_like_ms"] / out["custom_mont_ladder_ms"], 4)
    ctx.set_timing(True)
    ctx.custom_mont_derive_dev(cid, dk, dx, sx, sst)
    torch.cuda.synchronize()
    out["kernels_ms"] = {name: round(ms, 4) for name, (cnt, ms) in ctx.get_timing().items()}
    ctx.set_timing(False)
    return out


def run_edwards(ctx, name, n):
    import numpy as np
    import torch
    import bench
    import custom_ed_checks as CK
    spec = CK.spec_of(name)
    cid = CK.define(ctx, spec)
    m = CK.model_of(spec)
    rnd = lambda tag: bench.xof("custom-ed:%s:%s" % (name, tag), n * 32).reshape(n, 32).copy()
    k, s = rnd("k"), rnd("s")
    y0 = next(y for y in range(2, 1000) if m.from_y(y, 0)[1] == 0 and m.from_y(y, 0)[0][0])
    g, st = ctx.custom_ed_decompress(cid, CK.rows([y0] * n), np.zeros(n, np.uint8), True)
    assert not st.any()
    pub, inf = ctx.mul_var(cid, s, g)                  # the peers' keys: s G
    assert not inf.any()
    enc = ctx.custom_ed_encode_points(cid, pub, True)
    order = (1 << 256) - 1
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    z = lambda *sh: torch.full(sh, 9, dtype=torch.uint8, device=dev)
    dk, dpub, denc, dy, dodd = t(k), t(pub), t(enc), t(pub[:, 32:]), t(pub[:, 31] & 1)
    oxy, ost, v0, v1, dx, dst, wx, wst, mxy, minf = z(n, 64), z(n), z(n), z(n), z(n, 32), z(n), z(n, 32), z(n), z(n, 64), z(n)
    calls = (("mul_var", lambda: ctx.mul_var_dev(cid, dk, dpub, mxy, minf)),
             ("custom_ed_decompress", lambda: ctx.custom_ed_decompress_dev(cid, dy, dodd, True, oxy, ost)),
             ("custom_ed_validate", lambda: ctx.custom_ed_validate_dev(cid, dpub, None, v0)),
             ("custom_ed_validate_order", lambda: ctx.custom_ed_validate_dev(cid, dpub, order, v1)),
             ("custom_ed_derive", lambda: ctx.custom_ed_derive_dev(cid, dk, dpub, dx, dst)),
             ("custom_ed_derive_wire", lambda: ctx.custom_ed_derive_wire_dev(cid, dk, denc, wx, wst)))
    rounds = {nm: [] for nm, _ in calls}
    for _ in range(3):
        for nm, fn in calls:
            rounds[nm].append(timed(fn))
    out = {"lib": os.path.basename(os.environ.get("ELLGPU_LIB", "libellgpu.so")), "curve": name, "n": n}
    for nm, _ in calls:
        ms = sorted(rounds[nm])[1]
        out[nm + "_ms"] = round(ms, 3)
        out[nm + "_ms_rounds"] = [round(v, 3) for v in rounds[nm]]
        out[nm + "_M_per_s"] = round(n / ms / 1e3, 2)
    assert not ost.any().item() and torch.equal(oxy, dpub) and not v0.any().item() and not minf.any().item()
    assert set(v1.unique().tolist()) <= {0, 3}          # an arbitrary scalar as the order: the ladder runs, the answer is its own
    assert not dst.any().item() and not wst.any().item() and torch.equal(dx, mxy[:, :32]) and torch.equal(wx, dx)
    out["derive_over_mul_var_plus_decompress"] = round(
        out["custom_ed_derive_ms"] / (out["mul_var_ms"] + out["custom_ed_decompress_ms"]), 4)
    out["derive_over_mul_var"] = round(out["custom_ed_derive_ms"] / out["mul_var_ms"], 4)
    ctx.set_timing(True)
    ctx.custom_ed_derive_wire_dev(cid, dk, denc, wx, wst)
    torch.cuda.synchronize()
    out["kernels_ms"] = {nm: round(ms, 4) for nm, (cnt, ms) in ctx.get_timing().items()}
    ctx.set_timing(False)
    return out


def run_ed_ecdsa(ctx, n):
    import numpy as np
    import torch
    import bench
    import custom_ed_checks as CK
    import custom_ed_ecdsa_checks as EC
    spec = EC.spec_of("curve1174")
    p, a, d, order, gx, gy = EC.params(spec)
    dom = EC.define(ctx, spec)
    plain = ctx.define_edwards(p, a, d)
    rnd = lambda tag: bench.xof("custom-ed-ecdsa:%s" % tag, n * 32).reshape(n, 32).copy()
    h, priv, k2 = rnd("h"), rnd("d"), rnd("k2")
    priv[:, 0] &= 0x00                                   # below n: the key is the scalar mul_var takes
    g = np.tile(CK.xy_rows([(gx, gy)]), (n, 1))
    pub, inf = ctx.mul_var(plain, priv, g)
    assert not inf.any()
    r, s, rec, ok = ctx.custom_ed_sign_det(dom, h, priv)
    assert ok.all()
    dev = torch.device("cuda", 0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    z = lambda *sh: torch.full(sh, 9, dtype=torch.uint8, device=dev)
    dh, dd, dr, ds, dpub, dg, dk2 = t(h), t(priv), t(r), t(s), t(pub), t(g), t(k2)
    vok, vst, sr, ss, sj, sok, mxy, minf = z(n), z(n), z(n, 32), z(n, 32), z(n), z(n), z(n, 64), z(n)
    calls = (("custom_ed_verify", lambda: ctx.custom_ed_verify_dev(dom, dh, dr, ds, dpub, vok, vst)),
             ("custom_ed_sign_det", lambda: ctx.custom_ed_sign_det_dev(dom, dh, dd, sr, ss, sj, sok)),
             ("custom_ed_sign", lambda: ctx.custom_ed_sign_dev(dom, dh, dd, dk2, sr, ss, sj, sok)),
             ("mul_add2", lambda: ctx.mul_add2_dev(plain, dd, dg, dk2, dpub, mxy, minf)),
             ("mul_var", lambda: ctx.mul_var_dev(plain, dd, dpub, mxy, minf)))
    out = {"lib": os.path.basename(os.environ.get("ELLGPU_LIB", "libellgpu.so")), "curve": "curve1174", "n": n}
    for nm, fn in calls:
        rounds = sorted(timed(fn) for _ in range(3))
        out[nm + "_ms"] = round(rounds[1], 3)
        out[nm + "_M_per_s"] = round(n / rounds[1] / 1e3, 3)
    assert vok.all().item() and not vst.any().item()
    # the kernels: five timed calls each
    ker = {}
    for nm, fn, kern in (("verify", calls[0][1], "edc_ecdsa_ladder"), ("mul_add2", calls[3][1], "edc_mul_add2")):
        vals = []
        for _ in range(2):                               # warm-up: the first calls of a kernel run long
            fn()
        torch.cuda.synchronize()
        for _ in range(5):
            ctx.set_timing(True)                         # (clears what the last call recorded)
            fn()
            torch.cuda.synchronize()
            tm = ctx.get_timing()
            vals.append(round(tm[kern][1] / max(1, tm[kern][0]), 4))
            ker[nm + "_kernels_ms"] = {x: round(ms, 4) for x, (cnt, ms) in tm.items()}
        out[kern + "_ms_five"] = vals
        out[kern + "_ms_median"] = sorted(vals)[2]
    ctx.set_timing(False)
    out.update(ker)
    spread = max(out["edc_mul_add2_ms_five"]) - min(out["edc_mul_add2_ms_five"])
    out["ladder_minus_mul_add2_ms"] = round(out["edc_ecdsa_ladder_ms_median"] - out["edc_mul_add2_ms_median"], 4)
    out["mul_add2_spread_ms"] = round(spread, 4)
    return out


def main():
    import torch
    import elliptic_amd
    import custom_domain_checks as CD
    if sys.argv[1:2] == ["--ed-ecdsa"]:
        torch.zeros(1, device="cuda:0")
        ctx = elliptic_amd.Context(0)
        try:
            for lg in [int(a) for a in sys.argv[2:]] or [16]:
                print(json.dumps(run_ed_ecdsa(ctx, 1 << lg)), flush=True)
        finally:
            ctx.close()
        return
    if sys.argv[1:2] == ["--wire"]:
        torch.zeros(1, device="cuda:0")
        ctx = elliptic_amd.Context(0)
        try:
            for name in ("brainpoolP256r1", "secp224k1"):
                spec = next(c for c in CD.curves() if c["name"] == name)
                for lg in [int(a) for a in sys.argv[2:]] or [18]:
                    print(json.dumps(run_wire(ctx, spec, 1 << lg)), flush=True)
        finally:
            ctx.close()
        return
    if sys.argv[1:2] == ["--sign"]:
        torch.zeros(1, device="cuda:0")
        ctx = elliptic_amd.Context(0)
        try:
            spec = next(c for c in CD.curves() if c["name"] == "brainpoolP256r1")
            for lg in [int(a) for a in sys.argv[2:]] or [18, 20]:
                print(json.dumps(run_sign(ctx, spec, 1 << lg)), flush=True)
        finally:
            ctx.close()
        return
    if sys.argv[1:2] == ["--edwards"]:
        torch.zeros(1, device="cuda:0")
        ctx = elliptic_amd.Context(0)
        try:
            for lg in [int(a) for a in sys.argv[2:]] or [18, 20]:
                for name in ("curve1174", "twisted_a4"):
                    print(json.dumps(run_edwards(ctx, name, 1 << lg)), flush=True)
        finally:
            ctx.close()
        return
    if sys.argv[1:2] == ["--mont"]:
        torch.zeros(1, device="cuda:0")
        ctx = elliptic_amd.Context(0)
        try:
            for lg in [int(a) for a in sys.argv[2:]] or [18, 20]:
                print(json.dumps(run_mont(ctx, 1 << lg)), flush=True)
        finally:
            ctx.close()
        return
    if sys.argv[1:2] == ["--ecdh"]:
        torch.zeros(1, device="cuda:0")
        ctx = elliptic_amd.Context(0)
        try:
            spec = next(c for c in CD.curves() if c["name"] == "brainpoolP256r1")
            for lg in [int(a) for a in sys.argv[2:]] or [18, 20]:
                print(json.dumps(run_ecdh(ctx, spec, 1 << lg)), flush=True)
        finally:
            ctx.close()
        return
    if sys.argv[1:2] == ["--recover"]:
        torch.zeros(1, device="cuda:0")
        ctx = elliptic_amd.Context(0)
        try:
            for name in ("brainpoolP256r1", "secp224k1"):
                spec = next(c for c in CD.curves() if c["name"] == name)
                for lg in [int(a) for a in sys.argv[2:]] or [16, 18]:
                    print(json.dumps(run_recover(ctx, spec, 1 << lg)), flush=True)
        finally:
            ctx.close()
        return
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
