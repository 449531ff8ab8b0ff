"""ECDSA verification against a fixed-base table of the signer's key (ellgpu_ecdsa_verify_base): the
reference's recorded verdicts (tests/golden/verify_base.json, tools/gen_golden_verify_base.js), a
Python-integer model of EC#verify and the helpers the hostsim, device and N-API tests share.

The model is EC#verify (ec/index.js:188-229) over Python integers: the range tests of r and s,
_truncateToN, u1 = e / s and u2 = r / s mod n, R = u1 G + u2 Q by the affine group law of
tests/fixed_base_checks.py, and the comparison -- JPoint#eqXToP's candidates r mod p, r + n, r + 2 n,
... below p where the curve has _maxwellTrick (floor(p / n) <= 100, n > p included), else x mod n
== r.  test_model_is_pinned_to_the_fixture holds it to every recorded verdict before anything else
relies on it.

Every call is run with one of three memory kinds: "host" (ELLGPU_MEM_HOST), "dev_np"
(ELLGPU_MEM_DEVICE on the hostsim build, where device memory is host memory) and "dev_torch"
(ELLGPU_MEM_DEVICE on device tensors, the current stream)."""
import json
import os
import random

import numpy as np

import fixed_base_checks as FB

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "verify_base.json")
FILL = 0xA5
PRESETS = FB.PRESETS
SIGNED = FB.SIGNED
DOMAINS = ["brainpoolP256r1", "secp192k1", "secp224k1", "cof_p10007"]
NAMES = PRESETS + DOMAINS
TAGS = ["valid20", "valid32", "valid64", "msgbits", "high_s", "flip_r", "flip_s", "flip_h", "r_zero", "s_zero",
        "r_n", "s_n", "r_nm1", "u1_zero", "sum_inf"]
I = FB.I
rows = FB.rows
xy_bytes = FB.xy_bytes
_cache = {}


def curves():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
    return _cache["golden"]


def spec_of(name):
    return next(c for c in curves() if c["name"] == name)


# ---- the model ------------------------------------------------------------------------------

class Domain:
    """the curve, G and n of a fixture entry, with EC#verify over Python integers"""

    def __init__(self, spec):
        self.B = spec["B"]
        self.n = I(spec["n"])
        if "p" in spec:
            self.m = FB.Model(I(spec["p"]), I(spec["a"]), I(spec["b"]))
            self.G = (I(spec["g"][0]), I(spec["g"][1]))
        else:
            from oracle import ec_oracle as O
            c = O.get_curve(spec["name"], precompute=False)
            self.m = FB.Model(c.p, c.a, c.b)
            self.G = (c.g.x, c.g.y)
            assert c.n == self.n
        self.p = self.m.p
        self.maxwell = self.p // self.n <= 100           # BaseCurve's _maxwellTrick (base.js:33-40)
        self.bits = 8 * self.B

    def truncate(self, h, msg_bits=0):
        """_truncateToN (ec/index.js:81-108) without its one subtraction of n: every use is mod n"""
        delta = (msg_bits or 8 * len(h)) - self.n.bit_length()
        e = int.from_bytes(h, "big")
        return e >> delta if delta > 0 else e

    def x_matches(self, x, r):
        if not self.maxwell:
            return x % self.n == r
        if x == r % self.p:
            return True
        c = r + self.n
        while c < self.p:                                # JPoint#eqXToP (short.js:908-925)
            if x == c:
                return True
            c += self.n
        return False

    def scalars(self, h, msg_bits, r, s):
        """(u1, u2), or None where r or s is out of range"""
        n = self.n
        if not (1 <= r < n and 1 <= s < n):
            return None
        w = pow(s, -1, n)
        return self.truncate(h, msg_bits) * w % n, r * w % n

    def verify(self, h, msg_bits, r, s, Q):
        u = self.scalars(h, msg_bits, r, s)
        if u is None:
            return 0
        R = self.m.mul2(u[0], self.G, u[1], Q)
        return 1 if R is not None and self.x_matches(R[0], r) else 0

    def verify_many(self, hs, msg_bits, rs, ss, Q):
        """the same for a batch on one key, through Model.mul_many (held to `verify` by check_model_pinned)"""
        us = [self.scalars(h, msg_bits, r, s) for h, r, s in zip(hs, rs, ss)]
        live = [i for i, u in enumerate(us) if u is not None]
        Rs = self.m.mul_many([us[i][1] for i in live], Q, self.bits,
                             self.m.mul_many([us[i][0] for i in live], self.G, self.bits))
        out = [0] * len(us)
        for i, R in zip(live, Rs):
            out[i] = 1 if R is not None and self.x_matches(R[0], rs[i]) else 0
        return out

    def sign(self, d, h, msg_bits, k, R=None):
        """EC#sign's equations with the nonce k (R = k G if the caller has it) -> (r, s, R)"""
        R = self.m.mul(k, self.G) if R is None else R
        r = R[0] % self.n
        return r, pow(k, -1, self.n) * (self.truncate(h, msg_bits) + r * d) % self.n, R

    def hash_of(self, e):
        """a hash of B bytes that _truncateToN brings to e exactly"""
        return (e << (self.bits - self.n.bit_length())).to_bytes(self.B, "big")


def domain_of(spec):
    key = ("domain", spec["name"])
    if key not in _cache:
        _cache[key] = Domain(spec)
    return _cache[key]


def keys_of(spec):
    return [(I(d), (I(x), I(y))) for d, x, y in spec["keys"]]


def check_fixture_shape(spec):
    """five keys d G with d = 1, n - 1, 2 and two more; every category and both verdicts per key"""
    D = domain_of(spec)
    keys = keys_of(spec)
    assert len(keys) == 5 and [d for d, _ in keys[:3]] == [1, D.n - 1, 2]
    assert keys[0][1] == D.G and keys[1][1] == D.m.neg(D.G)
    for d, Q in keys:
        assert D.m.on_curve(Q) and D.m.mul(d, D.G) == Q
    want = set(TAGS) | ({"x_ge_n"} if spec["name"] == "cof_p10007" else set()) | ({"r_ge_p"} if D.n > D.p else set())
    for ki, cs in enumerate(spec["cases"]):
        assert {c[0] for c in cs} == want == set(spec["tags"]), (spec["name"], ki)
        assert {c[5] for c in cs} == {0, 1}
        by = {c[0]: c for c in cs}
        assert [len(by[t][1]) // 2 for t in ("valid20", "valid32", "valid64")] == [20, 32, 64] and by["msgbits"][2] > 0
        assert all(by[t][5] == 1 for t in ("valid20", "valid32", "valid64", "msgbits", "high_s", "u1_zero"))
        assert all(by[t][5] == 0 for t in ("r_zero", "s_zero", "r_n", "s_n", "sum_inf"))
        assert D.truncate(bytes.fromhex(by["u1_zero"][1])) % D.n == 0
        si = by["sum_inf"]
        assert (D.truncate(bytes.fromhex(si[1])) + I(si[3]) * keys[ki][0]) % D.n == 0
        if "x_ge_n" in want:
            c = by["x_ge_n"]
            u = D.scalars(bytes.fromhex(c[1]), c[2], I(c[3]), I(c[4]))
            assert c[5] == 1 and D.m.mul2(u[0], D.G, u[1], keys[ki][1])[0] >= D.n
        if "r_ge_p" in want:
            assert D.p <= I(by["r_ge_p"][3]) < D.n


def check_model_pinned(spec):
    D = domain_of(spec)
    for (d, Q), cs in zip(keys_of(spec), spec["cases"]):
        got = [D.verify(bytes.fromhex(c[1]), c[2], I(c[3]), I(c[4]), Q) for c in cs]
        assert got == [c[5] for c in cs], (spec["name"], d)
        for bits in sorted({(c[2], len(c[1])) for c in cs}):
            idx = [j for j, c in enumerate(cs) if (c[2], len(c[1])) == bits]
            fast = D.verify_many([bytes.fromhex(cs[j][1]) for j in idx], bits[0], [I(cs[j][3]) for j in idx],
                                 [I(cs[j][4]) for j in idx], Q)
            assert fast == [got[j] for j in idx]


# ---- the engine's side ----------------------------------------------------------------------

def curve_id(ctx, spec):
    """the preset's name, or the id of the user-defined domain"""
    if "p" not in spec:
        return spec["name"]
    return ctx.define_short_domain(I(spec["p"]), I(spec["a"]), I(spec["b"]), I(spec["n"]), I(spec["g"][0]), I(spec["g"][1]))


def define_keys(ctx, spec, width=0, cid=None):
    """-> (curve id, the handles of the five keys at one table width)"""
    cid = curve_id(ctx, spec) if cid is None else cid
    return cid, [ctx.define_base(cid, xy_bytes(Q, spec["B"]), width) for _, Q in keys_of(spec)]


def _raw(ctx, rc):
    from elliptic_amd import _lib
    if rc != 0:
        raise _lib.EllgpuError(rc, ctx._lib.ellgpu_last_error().decode())


def _P(a):
    return a.ctypes.data if a is not None else None


def run_verify(ctx, base, h, r, s, msg_bits=0, mem="host"):
    """ellgpu_ecdsa_verify_base on (n, hash_len), (n, B), (n, B) uint8 arrays -> ok (n,) uint8, written into a
    buffer that was filled with 0xA5"""
    h, r, s = (np.ascontiguousarray(a, np.uint8) for a in (h, r, s))
    n = h.shape[0]
    if mem == "dev_torch":
        import torch
        dh, dr, ds = (torch.from_numpy(a).cuda() for a in (h, r, s))
        ok = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
        ctx.ecdsa_verify_base(base, dh, dr, ds, msg_bits, out=(ok,))
        torch.cuda.synchronize()
        return ok.cpu().numpy()
    ok = np.full(n, FILL, np.uint8)
    if mem == "host":
        got = ctx.ecdsa_verify_base(base, h, r, s, msg_bits, out=(ok,))
        assert got is ok
    else:
        _raw(ctx, ctx._lib.ellgpu_ecdsa_verify_base(ctx._ctx, base, n, _P(h), h.shape[1], msg_bits, _P(r), _P(s), _P(ok), 1, None))
    return ok


def case_groups(cs):
    """the recorded cases of one key, grouped by (hash_len, msg_bits): one call each"""
    out = {}
    for j, c in enumerate(cs):
        out.setdefault((len(c[1]) // 2, c[2]), []).append(j)
    return sorted(out.items())


def check_golden(ctx, spec, hs, mem):
    """every recorded case of every key through one memory kind; -> the bytes the engine wrote"""
    B, got = spec["B"], []
    for h, cs in zip(hs, spec["cases"]):
        for (hl, bits), idx in case_groups(cs):
            hh = np.stack([np.frombuffer(bytes.fromhex(cs[j][1]), np.uint8) for j in idx])
            ok = run_verify(ctx, h, hh, rows([I(cs[j][3]) for j in idx], B), rows([I(cs[j][4]) for j in idx], B), bits, mem)
            assert ok.tolist() == [cs[j][5] for j in idx], (spec["name"], mem, h, hl, bits, [cs[j][0] for j in idx])
            got.append(ok)
    return got


# ---- random batches -------------------------------------------------------------------------

def random_batch(spec, n, seed, key=3, model=True):
    """n signatures by key `key` over hashes of B bytes, made by the model with the nonces k0 + i dk
    (R advances by one affine addition per item).  Every third item is tampered with, cycling
    through r, s and the hash.  The first rows are there by construction: row 0 a valid signature
    over a hash with e = n (u1 = 0), row 1 e = -r d (R = O, false), row 2 r = n (out of range).
    model: the model's verdicts for all n items (`want`); otherwise for the first 64 alone."""
    rng = random.Random("verify-base:%s:%d" % (spec["name"], seed))
    D = domain_of(spec)
    B, nn = D.B, D.n
    d, Q = keys_of(spec)[key]
    k, dk = rng.randrange(1, nn), rng.randrange(1, nn)
    R, S = D.m.mul(k, D.G), D.m.mul(dk, D.G)
    hs, rs, ss, kinds = [], [], [], []
    for i in range(n):
        while R is None or R[0] % nn == 0:
            k, R = (k + dk) % nn, D.m.add(R, S)
        h = D.hash_of(nn) if i == 0 else bytes(rng.getrandbits(8) for _ in range(B))
        r, s, _ = D.sign(d, h, 0, k, R)
        kind = "valid"
        if i == 1:
            r, s, kind = rng.randrange(1, nn), rng.randrange(1, nn), "sum_inf"
            h = D.hash_of(-r * d % nn)
        elif i == 2:
            r, kind = nn, "r_range"
        elif i >= 3 and i % 3 == 0:
            kind = ("r", "s", "hash")[(i // 3) % 3]
            bit = 1 << rng.randrange(nn.bit_length() - 1)
            if kind == "r":
                r ^= bit
            elif kind == "s":
                s ^= bit
            else:
                h = bytes([h[0] ^ (0x80 >> rng.randrange(8))]) + h[1:]
        if s == 0:                                       # (a tiny n: keep s in range so that the row says what its kind says)
            s = 1
        hs.append(h); rs.append(r); ss.append(s); kinds.append(kind)
        k, R = (k + dk) % nn, D.m.add(R, S)
    m = n if model else min(n, 64)
    return {"h": np.stack([np.frombuffer(h, np.uint8) for h in hs]), "r": rows(rs, B), "s": rows(ss, B), "kinds": kinds,
            "want": np.array(D.verify_many(hs[:m], 0, rs[:m], ss[:m], Q), np.uint8), "key": key,
            "pub": np.frombuffer(xy_bytes(Q, B), np.uint8), "ints": (hs, rs, ss)}


def batch_meets_conditions(spec, bt):
    """both verdicts, the three constructed rows and all three kinds of tampering -- asserted on the
    model, before any engine runs"""
    D = domain_of(spec)
    d, Q = keys_of(spec)[bt["key"]]
    hs, rs, ss = bt["ints"]
    w = bt["want"]
    u0, u1 = D.scalars(hs[0], 0, rs[0], ss[0]), D.scalars(hs[1], 0, rs[1], ss[1])
    return (set(w.tolist()) == {0, 1} and u0[0] == 0 and w[0] == 1 and D.m.mul2(u1[0], D.G, u1[1], Q) is None and w[1] == 0
            and rs[2] == D.n and w[2] == 0 and bt["kinds"][:3] == ["valid", "sum_inf", "r_range"]
            and {"r", "s", "hash", "valid"} <= set(bt["kinds"]))


def tiled_verify(ctx, cid, bt, n):
    """ellgpu_ecdsa_verify on the first n items with the key repeated in pub_xy (host memory)"""
    pub = np.ascontiguousarray(np.broadcast_to(bt["pub"], (n, bt["pub"].shape[0])))
    return np.asarray(ctx.ecdsa_verify(cid, bt["h"][:n], bt["r"][:n], bt["s"][:n], pub), np.uint8)
