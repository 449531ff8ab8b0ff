"""Checks of ECDSA on user-defined domains (ellgpu_curve_define_short_domain), shared by the CPU
test (tests/test_custom_domain_hostsim.py, the hostsim build of the device code) and the GPU test
(tests/test_custom_domain_gpu.py): the reference's verdicts and points recorded in
tests/golden/custom_ecdsa.json (tools/gen_golden_custom_ecdsa.js), and random batches against
the C oracle."""
import json
import os
import random

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "custom_ecdsa.json")


def I(h):
    return int(h, 16)


def b32(v):
    return np.frombuffer(int(v).to_bytes(32, "big"), np.uint8)


def curves():
    with open(GOLDEN) as f:
        return json.load(f)


def params(spec):
    return [I(spec[k]) for k in ("p", "a", "b", "n")] + [I(spec["g"]["x"]), I(spec["g"]["y"])]


def define(ctx, spec):
    return ctx.define_short_domain(*params(spec))


def _xy(q):
    return np.concatenate([b32(I(q["x"])), b32(I(q["y"]))])


def check_verify_golden(ctx, spec, cid=None):
    """every recorded EC#verify verdict, one call per (digest length, msgBitLength) group;
    returns the number of cases checked"""
    from elliptic_amd import _lib
    cid = define(ctx, spec) if cid is None else cid
    nbits = I(spec["n"]).bit_length()
    groups = {}
    for c in spec["verify"]:
        groups.setdefault((len(c["h"]) // 2, c["bits"]), []).append(c)
    for (hl, bits), cs in sorted(groups.items()):
        h = np.stack([np.frombuffer(bytes.fromhex(c["h"]), np.uint8) for c in cs])
        r = np.stack([b32(I(c["r"]) % (1 << 256)) for c in cs])
        s = np.stack([b32(I(c["s"]) % (1 << 256)) for c in cs])
        q = np.stack([_xy(c["q"]) for c in cs])
        if 8 * hl - max(0, (bits or 8 * hl) - nbits) > 256:
            # a msgBitLength below the digest's width leaves more than 256 bits: outside the C
            # ABI's domain, as on the presets (ELLGPU_E_ARG; the JS layer keeps such calls on the
            # reference)
            with pytest.raises(_lib.EllgpuError) as e:
                ctx.ecdsa_verify(cid, h, r, s, q, msg_bits=bits)
            assert e.value.code == -2
            continue
        ok, st = ctx.ecdsa_verify(cid, h, r, s, q, msg_bits=bits, status=True)
        for i, c in enumerate(cs):
            if c["tag"] == "off_curve":
                # outside the engine's domain: a verdict of 0 with status 2 (the caller runs the
                # reference on such keys), whatever the reference answers
                assert ok[i] == 0 and st[i] == 2, (spec["name"], c)
            else:
                assert ok[i] == c["ok"] and st[i] == 0, (spec["name"], c["tag"], c, int(ok[i]), int(st[i]))
    return len(spec["verify"])


def check_points_golden(ctx, spec, cid=None):
    """k*G (mul_fixed) and k1*G + k2*Q (mul_add2 with p1 = None) against the reference"""
    cid = define(ctx, spec) if cid is None else cid
    k = np.stack([b32(I(c["k"])) for c in spec["mulg"]])
    xy, inf = ctx.mul_fixed(cid, k)
    for i, c in enumerate(spec["mulg"]):
        _same_point(xy[i], inf[i], c["r"], (spec["name"], "k*G", c["k"]))
    k1 = np.stack([b32(I(c["k1"])) for c in spec["muladd"]])
    k2 = np.stack([b32(I(c["k2"])) for c in spec["muladd"]])
    q = np.stack([_xy(c["q"]) for c in spec["muladd"]])
    xy, inf = ctx.mul_add2(cid, k1, None, k2, q)
    for i, c in enumerate(spec["muladd"]):
        _same_point(xy[i], inf[i], c["r"], (spec["name"], "mulAdd", c))
    return len(spec["mulg"]) + len(spec["muladd"])


def _same_point(xy, inf, want, what):
    if want.get("inf"):
        assert inf == 1, what
    else:
        assert inf == 0, what
        assert int.from_bytes(xy[:32].tobytes(), "big") == I(want["x"]), what
        assert int.from_bytes(xy[32:].tobytes(), "big") == I(want["y"]), what


def oracle_name(spec):
    from oracle import c_oracle
    name = "domain_" + spec["name"]
    c_oracle.define_short(name, *params(spec))
    return name


def random_batch(spec, n, seed, ctx=None, cid=None):
    """n verify items over the domain: about half valid signatures (keys, nonces and digests from
    the oracle's k*G), the rest with one of r, s, the digest or the key disturbed.  Returns
    (h, r, s, q, expect) with expect the verdict known by construction (None where it is not:
    the disturbed items)."""
    from oracle import c_oracle
    name = oracle_name(spec)
    p, a, b, nn, gx, gy = params(spec)
    nbits = nn.bit_length()
    rnd = random.Random(seed)
    d = [rnd.randrange(1, nn) for _ in range(n)]
    k = [rnd.randrange(1, nn) for _ in range(n)]
    e = [rnd.getrandbits(256) for _ in range(n)]
    pts = np.stack([b32(v) for v in d + k])
    xy, inf = c_oracle.mul_mt(name, pts, threads=8)
    q = xy[:n].copy()
    rx = [int.from_bytes(xy[n + i, :32].tobytes(), "big") for i in range(n)]
    h = np.stack([b32(v) for v in e])
    r, s, expect = [], [], []
    for i in range(n):
        z = e[i] >> max(0, 256 - nbits)
        if z >= nn:
            z -= nn
        ri = rx[i] % nn
        si = pow(k[i], nn - 2, nn) * (z + ri * d[i]) % nn
        kind = rnd.randrange(8)
        if ri == 0 or si == 0:
            kind = 4
        if kind < 4:
            expect.append(1)
        elif kind == 4:
            si = (si + 1) % nn
            expect.append(None)
        elif kind == 5:
            ri = (ri + 1) % nn
            expect.append(None)
        elif kind == 6:
            h[i, 31] ^= 1
            expect.append(None)
        else:
            q[i] = xy[(i + 1) % n]
            expect.append(None)
        r.append(b32(ri))
        s.append(b32(si))
    return h, np.stack(r), np.stack(s), q, expect


def oracle_verify(spec, h, r, s, q):
    from oracle import c_oracle
    return c_oracle.verify(oracle_name(spec), h, r, s, q, threads=8)
