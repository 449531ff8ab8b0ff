"""Checks of EC#recoverPubKey on user-defined ECDSA domains (ellgpu_custom_recover), shared by the
CPU test (tests/test_custom_recover_hostsim.py, the hostsim build of the device code) and the GPU
test (tests/test_custom_recover_gpu.py):

  * the reference's statuses, points and thrown messages recorded in
    tests/golden/custom_recover.json (tools/gen_golden_custom_recover.js);
  * random batches against a model over Python integers that restates recoverPubKey
    (ec/index.js:231-259) step by step: the range test, the second-candidate test against
    p mod n, x = (r + [j >> 1] n) mod p as toRed leaves it, Euler's criterion and the root with
    its parity, s1 = (n - e) / r, s2 = s / r, and s1 G + s2 R.

The model's last step is done twice: by the C oracle's mulAdd for every item, and by affine
additions over Python integers for a sample of them (the first SAMPLE_HEAD items and every
SAMPLE_STEP-th after), which must agree -- the whole batch over integers alone would take a
minute at the largest size.  A smaller sample also goes through oracle.ec_oracle.ecdsa_recover.

Every call is run in one of three forms: "host" (host buffers), "dev_np" (the _dev entry point on
the hostsim build, where device memory is host memory) and "dev_torch" (the _dev entry point on
torch tensors).  Result arrays are pre-filled with 0xA5, so a byte the call leaves unwritten shows."""
import json
import os
import random

import numpy as np

import custom_domain_checks as CD
import custom_wire_checks as CW

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "custom_recover.json")
FILL = CW.FILL
THROWN = {"Unable to find sencond key candinate", "invalid point", "Assertion failed",
          "The recovery param is more than two bits"}
SAMPLE_HEAD, SAMPLE_STEP, SAMPLE_ORACLE = 48, 37, 12

I = CD.I
b32 = CD.b32
_cache = {}


def curves():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
    return _cache["golden"]


def spec_of(name):
    return next(c for c in curves() if c["name"] == name)


def define(ctx, spec):
    return CD.define(ctx, spec)


# ---- the three forms of the call ----------------------------------------------------------

def run_recover(ctx, cid, h, r, s, j, form="host"):
    h, r, s, j = (np.ascontiguousarray(a, np.uint8) for a in (h, r, s, j))
    n, hl = h.shape
    xy, st = np.full((n, 64), FILL, np.uint8), np.full((n,), FILL, np.uint8)
    if form == "host":
        ctx.custom_recover(cid, h, r, s, j, out=(xy, st))
    elif form == "dev_np":
        P = lambda a: a.ctypes.data
        CW._raw(ctx, ctx._lib.ellgpu_custom_recover_dev(ctx._ctx, cid, n, P(h), hl, P(r), P(s), P(j), P(xy), P(st),
                                                        None))
    else:
        xy, st = CW._torch_call(lambda i, o: ctx.custom_recover_dev(cid, i[0], i[1], i[2], i[3], o[0], o[1]),
                                [h, r, s, j], [xy, st])
    return xy, st


# ---- the reference's recorded answers -----------------------------------------------------

def check_golden(ctx, spec, form="host", cid=None):
    """every recorded case, one call per digest length; a thrown message is status 2; returns the
    set of statuses seen"""
    cid = define(ctx, spec) if cid is None else cid
    assert I(spec["p_mod_n"]) == I(spec["p"]) % I(spec["n"])
    groups = {}
    for c in spec["recover"]:
        groups.setdefault(len(c["h"]) // 2, []).append(c)
    seen, msgs = set(), set()
    for hl, cs in sorted(groups.items()):
        h = np.stack([np.frombuffer(bytes.fromhex(c["h"]), np.uint8) for c in cs])
        r = np.stack([b32(I(c["r"])) for c in cs])
        s = np.stack([b32(I(c["s"])) for c in cs])
        j = np.array([c["j"] for c in cs], np.uint8)
        xy, st = run_recover(ctx, cid, h, r, s, j, form)
        for i, c in enumerate(cs):
            what = (spec["name"], c["tag"], c, int(st[i]))
            assert ("msg" in c) == (c["st"] == 2) and c.get("msg", next(iter(THROWN))) in THROWN, what
            assert st[i] == c["st"], what
            want = b32(I(c["x"])).tobytes() + b32(I(c["y"])).tobytes() if c["st"] == 0 else bytes(64)
            assert xy[i].tobytes() == want, what
            seen.add(c["st"])
            msgs.add(c.get("msg"))
    assert seen == {0, 1, 2, 3}, seen
    no_root = "invalid point" if I(spec["p"]) % 4 == 3 else "Assertion failed"
    assert {"Unable to find sencond key candinate", "The recovery param is more than two bits", no_root} <= msgs
    return seen


# ---- recoverPubKey over Python integers -----------------------------------------------------

def sqrt_mod(a, p):
    """a root of the quadratic residue a mod the odd prime p (Tonelli-Shanks)"""
    if a == 0:
        return 0
    if p % 4 == 3:
        return pow(a, (p + 1) // 4, p)
    s, q = 0, p - 1
    while q % 2 == 0:
        s, q = s + 1, q // 2
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, x = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, u = 0, t
        while u != 1:
            u, i = u * u % p, i + 1
        bb = pow(c, 1 << (m - i - 1), p)
        m, c, t, x = i, bb * bb % p, t * bb * bb % p, x * bb % p
    return x


def pt_add(p, a, P, Q):
    """affine addition on y^2 = x^3 + a x + b over integers; None is the point at infinity"""
    if P is None:
        return Q
    if Q is None:
        return P
    (x1, y1), (x2, y2) = P, Q
    if x1 == x2:
        if (y1 + y2) % p == 0:
            return None
        lam = (3 * x1 * x1 + a) * pow(2 * y1, -1, p) % p
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return x3, (lam * (x1 - x3) - y1) % p


def pt_mul_add(p, a, k1, P1, k2, P2):
    """k1 P1 + k2 P2, one joint double-and-add"""
    both = pt_add(p, a, P1, P2)
    acc = None
    for i in range(max(k1.bit_length(), k2.bit_length()) - 1, -1, -1):
        acc = pt_add(p, a, acc, acc)
        sel = ((k1 >> i) & 1) | (((k2 >> i) & 1) << 1)
        if sel:
            acc = pt_add(p, a, acc, (P1, P2, both)[sel - 1])
    return acc


def model_front(spec, h, r, s, j):
    """recoverPubKey up to the double-scalar multiplication: (status, R, s1, s2) with status 0 =
    go on, 2 = thrown, 3 = r out of the engine's range (tested first)"""
    p, a, b, n, gx, gy = CD.params(spec)
    if r == 0 or r >= n:
        return 3, None, 0, 0
    if j > 3:
        return 2, None, 0, 0                                  # 'The recovery param is more than two bits'
    second = j >> 1
    if second and r >= p % n:
        return 2, None, 0, 0                                  # 'Unable to find sencond key candinate'
    x = (r + n if second else r) % p                          # pointFromX: toRed reduces mod p
    rhs = (x * x * x + a * x + b) % p
    if rhs != 0 and pow(rhs, (p - 1) // 2, p) != 1:
        return 2, None, 0, 0                                  # 'invalid point' / 'Assertion failed'
    y = sqrt_mod(rhs, p)
    assert y * y % p == rhs
    if (y & 1) != (j & 1):
        y = (p - y) % p
    e = int.from_bytes(h, "big")
    rinv = pow(r, -1, n)
    return 0, (x, y), (n - e) * rinv % n, s * rinv % n


def model(spec, h, r, s, j):
    """-> (st (n,), xy (n, 64)) for byte rows h, r, s and recids j"""
    from oracle import c_oracle, ec_oracle
    p, a, b, n, gx, gy = CD.params(spec)
    name = CD.oracle_name(spec)
    cnt = len(j)
    ri = [int.from_bytes(x.tobytes(), "big") for x in r]
    si = [int.from_bytes(x.tobytes(), "big") for x in s]
    front = [model_front(spec, h[i].tobytes(), ri[i], si[i], int(j[i])) for i in range(cnt)]
    live = [i for i in range(cnt) if front[i][0] == 0]
    st = np.array([f[0] for f in front], np.uint8)
    xy = np.zeros((cnt, 64), np.uint8)
    if live:
        k1 = np.stack([b32(front[i][2]) for i in live])
        k2 = np.stack([b32(front[i][3]) for i in live])
        R = np.stack([np.concatenate([b32(front[i][1][0]), b32(front[i][1][1])]) for i in live])
        q, inf = c_oracle.mul_add(name, k1, None, k2, R)
        for m, i in enumerate(live):
            if inf[m]:
                st[i] = 1
            else:
                xy[i] = q[m]
    # the same over integers alone, on a sample
    sample = [i for i in live if i < SAMPLE_HEAD or i % SAMPLE_STEP == 0]
    for i in sample:
        Q = pt_mul_add(p, a, front[i][2], (gx, gy), front[i][3], front[i][1])
        got = None if st[i] == 1 else (int.from_bytes(xy[i, :32].tobytes(), "big"), int.from_bytes(xy[i, 32:].tobytes(), "big"))
        assert Q == got, (spec["name"], i, Q, got)
    cur = ec_oracle.ShortCurve(spec["name"], p, a, b, n, gx, gy)
    for i in list(range(min(cnt, SAMPLE_ORACLE))):
        if st[i] == 3:
            continue
        try:
            Q = ec_oracle.ecdsa_recover(cur, int.from_bytes(h[i].tobytes(), "big"), ri[i], si[i], int(j[i]))
            want = (1, bytes(64)) if Q.inf else (0, b32(Q.x).tobytes() + b32(Q.y).tobytes())
        except ValueError as e:
            assert str(e) in THROWN
            want = (2, bytes(64))
        assert (int(st[i]), xy[i].tobytes()) == want, (spec["name"], i)
    return st, xy


def random_batch(spec, n, seed, hash_len=32):
    """n items with digests of hash_len bytes:
      60 %  signatures made here by integer ECDSA (key d, nonce k, e = the digest mod n, which is
            what recovery sees whatever the digest's length), with the recovery parameter of k G
      25 %  random r, s below n, j in 0..5
      15 %  constructed: r below and around p mod n with j = 2, 3; r around p and n - 1 where
            n > p; r = 0, n, n + 1; s = 0 and s >= n; j = 4, 5
    -> dict h, r, s, j (byte rows), signer (n, 64: the signer's key, zeros where there is none),
    signed (bool rows), st, xy (the model's answers)"""
    key = (spec["name"], n, seed, hash_len)
    if key in _cache:
        return _cache[key]
    from oracle import c_oracle
    p, a, b, nn, gx, gy = CD.params(spec)
    name = CD.oracle_name(spec)
    pmn = p % nn
    rnd = random.Random(seed)
    d = [rnd.randrange(1, nn) for _ in range(n)]
    k = [rnd.randrange(1, nn) for _ in range(n)]
    pts, _ = c_oracle.mul_mt(name, np.stack([b32(v) for v in d + k]), threads=8)
    h = np.frombuffer(bytes(rnd.getrandbits(8) for _ in range(n * hash_len)), np.uint8).reshape(n, hash_len).copy()
    top = 1 << 256
    edges = [lambda: (rnd.randrange(1, max(2, min(pmn, nn))), rnd.randrange(1, nn), 2 + rnd.randrange(2)),
             lambda: ((pmn - 1) % top, rnd.randrange(1, nn), rnd.randrange(4)),
             lambda: (pmn, rnd.randrange(1, nn), rnd.randrange(4)),
             lambda: (pmn + 1, rnd.randrange(1, nn), rnd.randrange(4)),
             lambda: (0, rnd.randrange(1, nn), rnd.randrange(6)),
             lambda: (nn, rnd.randrange(1, nn), rnd.randrange(4)),
             lambda: ((nn + 1) % top, rnd.randrange(1, nn), rnd.randrange(4)),
             lambda: (rnd.randrange(1, nn), 0, rnd.randrange(4)),
             lambda: (rnd.randrange(1, nn), rnd.randrange(nn, top), rnd.randrange(4)),
             lambda: (rnd.randrange(1, nn), rnd.randrange(1, nn), 4 + rnd.randrange(2))]
    if nn > p:
        edges += [lambda: (p - 1, rnd.randrange(1, nn), rnd.randrange(4)),
                  lambda: (p, rnd.randrange(1, nn), rnd.randrange(4)),
                  lambda: (p + 2, rnd.randrange(1, nn), rnd.randrange(4)),
                  lambda: (nn - 1, rnd.randrange(1, nn), rnd.randrange(4))]
    r, s, j = [], [], np.zeros(n, np.uint8)
    signer = np.zeros((n, 64), np.uint8)
    signed = np.zeros(n, bool)
    nedge = 0
    for i in range(n):
        kind = i % 20                                        # 12 signed, 5 random, 3 constructed of every 20
        if kind < 12:
            rx = int.from_bytes(pts[n + i, :32].tobytes(), "big")
            ry = int.from_bytes(pts[n + i, 32:].tobytes(), "big")
            ri = rx % nn
            e = int.from_bytes(h[i].tobytes(), "big") % nn
            si = pow(k[i], -1, nn) * (e + ri * d[i]) % nn
            if ri == 0 or si == 0:
                kind = 12
            else:
                ji = (ry & 1) | (2 if rx != ri else 0)
                signer[i] = pts[i]
                signed[i] = True
        if 12 <= kind < 17:
            ri, si, ji = rnd.randrange(1, nn), rnd.randrange(1, nn), rnd.randrange(6)
        elif kind >= 17:
            ri, si, ji = edges[nedge % len(edges)]()
            nedge += 1
        r.append(b32(ri))
        s.append(b32(si))
        j[i] = ji
    out = {"h": h, "r": np.stack(r), "s": np.stack(s), "j": j, "signer": signer, "signed": signed}
    out["st"], out["xy"] = model(spec, h, out["r"], out["s"], j)
    for v in out.values():
        v.setflags(write=False)
    _cache[key] = out
    return out


def check_batch(ctx, spec, bt, n, form="host", cid=None):
    """the first n items of a random batch, item by item against the model; returns the engine's
    (xy, st)"""
    cid = define(ctx, spec) if cid is None else cid
    xy, st = run_recover(ctx, cid, bt["h"][:n], bt["r"][:n], bt["s"][:n], bt["j"][:n], form)
    bad = np.nonzero(st != bt["st"][:n])[0]
    assert bad.size == 0, (spec["name"], n, form, bad[:10], st[bad[:10]], bt["st"][bad[:10]])
    bad = np.nonzero((xy != bt["xy"][:n]).any(axis=1))[0]
    assert bad.size == 0, (spec["name"], n, form, bad[:10])
    if n >= 257:
        # conditions, so that the test cannot pass on a batch of error rows
        seen = set(int(v) for v in st)
        assert {0, 2, 3} <= seen, seen
        if spec["name"] in ("brainpoolP256r1", "secp224k1"):
            back = (st == 0) & bt["signed"][:n] & (xy == bt["signer"][:n]).all(axis=1)
            assert back.sum() >= 0.55 * n, (int(back.sum()), n)
    return xy, st


def check_random(ctx, spec, n, seed, form="host", hash_len=32, cid=None):
    """a random batch of n items against the model; returns the engine's (xy, st)"""
    return check_batch(ctx, spec, random_batch(spec, n, seed, hash_len), n, form, cid)
