"""ECDSA on user-defined Edwards domains (ellgpu_curve_define_edwards_domain, ellgpu_custom_ed_verify,
_custom_ed_sign, _custom_ed_sign_det): lib/elliptic/ec/index.js:81-229 restated over Python integers
on the AFFINE complete addition law of a x^2 + y^2 = 1 + d x^2 y^2, the reference's recorded answers
(tests/golden/custom_ed_ecdsa.json, tools/gen_golden_custom_ed_ecdsa.js) and the helpers the hostsim,
device and N-API tests share.

The model knows nothing of the engine's ladder: points are affine pairs, P + Q is
((x1 y2 + y1 x2) / (1 + t), (y1 y2 - a x1 x2) / (1 - t)) with t = d x1 x2 y1 y2 -- defined for every
pair of points where a is a square and d is not, which holds on all four domains -- scalar
multiplication is double-and-add, u1 G + u2 Q is two of them and a sum.  EC#verify is the range test,
u1 = msg / s, u2 = r / s, false for the identity (0, 1), then x mod n == r; with _maxwellTrick
(floor(p / n) <= 100) the reference compares X == (r + j n) Z for the j with r + j n < p, which is
the same predicate on the affine x (asserted where the model meets the fixture).  EC#sign's scalar
half -- _truncateToN, HmacDRBG, the rejections, the canonical form -- is tests/custom_sign_checks.py's.

Every call is run in one of three forms: "host" (host buffers), "dev_np" (the _dev entry point on
the hostsim build, where device memory is host memory) and "dev_torch" (the _dev entry point on
device tensors), through the runners' conventions of tests/custom_ed_checks.py: result arrays are
pre-filled with 0xA5, so a byte the call leaves unwritten shows."""
import json
import os
import random

import numpy as np

import custom_ed_checks as CK
import custom_sign_checks as CS
import custom_wire_checks as CW

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "custom_ed_ecdsa.json")
DOMAINS = ["curve1174", "e222", "ed25519_by_hand", "toy_p65521"]
BIG = DOMAINS[:3]
FILL = CW.FILL
I = CK.I
rows = CK.rows
xy_rows = CK.xy_rows
ints = CK.ints
_P = CK._P
_cache = {}


def domains():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
    return _cache["golden"]


def spec_of(name):
    return next(c for c in domains() if c["name"] == name)


def params(spec):
    """p, a, d, n, gx, gy"""
    return tuple(I(spec[k]) for k in ("p", "a", "d", "n", "gx", "gy"))


def define(ctx, spec):
    return ctx.define_edwards_domain(*params(spec))


# ---- the group over the integers: the affine complete law ---------------------------------------

class Group:
    def __init__(self, spec):
        self.p, self.a, self.d, self.n, gx, gy = params(spec)
        self.g = (gx, gy)
        self.maxwell = self.p // self.n <= 100
        self.memo = {}

    def on_curve(self, P):
        p = self.p
        x, y = P[0] % p, P[1] % p
        return (self.a * x * x + y * y - 1 - self.d * x * x * y * y) % p == 0

    def add(self, P, Q):
        p = self.p
        (x1, y1), (x2, y2) = P, Q
        t = self.d * x1 * x2 % p * y1 * y2 % p
        i = pow((1 - t * t) % p, -1, p)                  # 1 / ((1 + t)(1 - t)): never 0 on a complete curve
        return ((x1 * y2 + y1 * x2) * (1 - t) % p * i % p, (y1 * y2 - self.a * x1 * x2) * (1 + t) % p * i % p)

    def mul(self, k, P):
        key = (k, P)
        if key not in self.memo:
            acc, Q = (0, 1), P
            while k:
                if k & 1:
                    acc = self.add(acc, Q)
                Q = self.add(Q, Q)
                k >>= 1
            self.memo[key] = acc
        return self.memo[key]

    def verify(self, h, bits, r, s, Q):
        """EC#verify -> (ok, status): status 2 for a key off the curve with r and s in range
        (the engine's convention; the reference computes with such a key)"""
        n, p = self.n, self.p
        if not (1 <= r < n and 1 <= s < n):
            return 0, 0
        Q = (Q[0] % p, Q[1] % p)
        if not self.on_curve(Q):
            return 0, 2
        msg = CS.truncate_msg(n, h, bits)
        w = pow(s, -1, n)
        P = self.add(self.mul(msg * w % n, self.g), self.mul(r * w % n, Q))
        if P == (0, 1):
            return 0, 0
        if self.maxwell:                                 # eqXToP: x == r + j n for a j with r + j n < p
            return (1 if any(P[0] == (r % p + j * n) % p and r + j * n < p for j in range(p // n + 1)) else 0), 0
        return (1 if P[0] % n == r else 0), 0

    def finish(self, msg, priv, k, R, canonical):
        """EC#sign's loop body behind the range test of k -> (r, s, j) or None"""
        n = self.n
        if R == (0, 1):
            return None
        r = R[0] % n
        if r == 0:
            return None
        s = pow(k, -1, n) * (r * (priv % n) + msg) % n
        if s == 0:
            return None
        j = (R[1] & 1) | (2 if R[0] != r else 0)
        if canonical and s > n >> 1:
            s, j = n - s, j ^ 1
        return r, s, j

    def sign_pass(self, h, bits, d, v, canonical):
        """one pass for the supplied nonce v"""
        k = CS.truncate_nonce(self.n, v)
        if not CS.nonce_in_range(self.n, k):
            return None
        return self.finish(CS.truncate_msg(self.n, h, bits), d, k, self.mul(k, self.g), canonical)

    def candidates(self, hname, h, bits, d):
        """-> (draws, v, k) of the first candidate in range (v None beyond MAX_DRAWS)"""
        n = self.n
        nb = (n.bit_length() + 7) // 8
        if nb < 24:
            raise ValueError(CS.ENTROPY)
        g = CS.HmacDrbg(hname, (d % n).to_bytes(nb, "big"), CS.truncate_msg(n, h, bits).to_bytes(nb, "big"))
        for it in range(CS.MAX_DRAWS):
            v = int.from_bytes(g.generate(nb), "big")
            k = CS.truncate_nonce(n, v)
            if CS.nonce_in_range(n, k):
                return it + 1, v, k
        return CS.MAX_DRAWS, None, None

    def sign_det(self, hname, h, bits, d, canonical):
        """-> ((r, s, j) or None, draws, x(k G) >= n)"""
        draws, v, k = self.candidates(hname, h, bits, d)
        if v is None:
            return None, draws, False
        R = self.mul(k, self.g)
        got = self.finish(CS.truncate_msg(self.n, h, bits), d, k, R, canonical)
        assert got is not None
        return got, draws, R[0] >= self.n


def group_of(spec):
    if ("group", spec["name"]) not in _cache:
        _cache[("group", spec["name"])] = Group(spec)
    return _cache[("group", spec["name"])]


# ---- the forms of the calls -----------------------------------------------------------------

def run_verify(ctx, cid, h, r, s, q, bits=0, form="host", want_status=True):
    """-> (ok, status); status is None with want_status=False (out_status = NULL)"""
    h, r, s, q = (np.ascontiguousarray(a, np.uint8) for a in (h, r, s, q))
    n, hl = h.shape
    ok, st = np.full(n, FILL, np.uint8), np.full(n, FILL, np.uint8)
    if form == "host":
        ctx.custom_ed_verify(cid, h, r, s, q, msg_bits=bits, status=want_status, out=(ok, st) if want_status else (ok,))
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_ed_verify_dev(ctx._ctx, cid, n, _P(h), hl, bits, _P(r), _P(s), _P(q), _P(ok),
                                                          _P(st) if want_status else None, None))
    else:
        ok, st = CW._torch_call(lambda i, o: ctx.custom_ed_verify_dev(cid, i[0], i[1], i[2], i[3], o[0], o[1], msg_bits=bits),
                                [h, r, s, q], [ok, st if want_status else None])
    return ok, (st if want_status else None)


def _filled(n):
    return [np.full(sh, FILL, np.uint8) for sh in ((n, 32), (n, 32), (n,), (n,))]


def run_sign(ctx, cid, h, d, k, canonical=0, bits=0, form="host"):
    h, d, k = (np.ascontiguousarray(a, np.uint8) for a in (h, d, k))
    n, hl = h.shape
    out = _filled(n)
    if form == "host":
        ctx.custom_ed_sign(cid, h, d, k, canonical=canonical, msg_bits=bits, out=out)
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_ed_sign_dev(ctx._ctx, cid, n, _P(h), hl, bits, _P(d), _P(k), canonical,
                                                        *[_P(o) for o in out], None))
    else:
        out = CW._torch_call(lambda i, o: ctx.custom_ed_sign_dev(cid, i[0], i[1], i[2], o[0], o[1], o[2], o[3],
                                                                 canonical=canonical, msg_bits=bits), [h, d, k], out)
    return out


def run_sign_det(ctx, cid, h, d, drbg_hash, canonical=0, bits=0, form="host"):
    h, d = (np.ascontiguousarray(a, np.uint8) for a in (h, d))
    n, hl = h.shape
    out = _filled(n)
    if form == "host":
        ctx.custom_ed_sign_det(cid, h, d, drbg_hash=drbg_hash, canonical=canonical, msg_bits=bits, out=out)
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_ed_sign_det_dev(ctx._ctx, cid, n, _P(h), hl, bits, _P(d), drbg_hash, canonical,
                                                            *[_P(o) for o in out], None))
    else:
        out = CW._torch_call(lambda i, o: ctx.custom_ed_sign_det_dev(cid, i[0], i[1], o[0], o[1], o[2], o[3],
                                                                     drbg_hash=drbg_hash, canonical=canonical,
                                                                     msg_bits=bits), [h, d], out)
    return out


# ---- the reference's recorded answers ----------------------------------------------------------

def _q(c):
    return I(c["q"][:64]), I(c["q"][64:])


def _off_curve(c):
    return c["tag"].startswith("off_curve")


def check_model_against_golden(spec):
    """the model alone against the fixture, so that a model error cannot hide behind agreement with
    the kernel; -> the tags seen"""
    G = group_of(spec)
    assert bool(spec["maxwell"]) == G.maxwell and int(spec["p_div_n"]) == G.p // G.n
    assert G.on_curve(G.g) and G.mul(G.n, G.g) == (0, 1)
    assert pow(G.a, (G.p - 1) // 2, G.p) == 1 and pow(G.d, (G.p - 1) // 2, G.p) == G.p - 1
    for c in spec["verify"]:
        ok, st = G.verify(bytes.fromhex(c["h"]), c["bits"], I(c["r"]), I(c["s"]), _q(c))
        if _off_curve(c):
            assert "ok" not in c and (ok, st) == (0, 2 if c["tag"] != "off_curve_r_0" else 0), (spec["name"], c["tag"])
        else:
            assert (ok, st) == (c["ok"], 0), (spec["name"], c["tag"])
    for c in spec["det"]:
        h, d = bytes.fromhex(c["h"]), I(c["d"])
        if "msg" in c:
            try:
                G.sign_det(c["hash"], h, c["bits"], d, c["c"])
            except ValueError as e:
                assert str(e) == c["msg"] == CS.ENTROPY
            else:
                raise AssertionError((spec["name"], c["tag"]))
            continue
        assert G.sign_det(c["hash"], h, c["bits"], d, c["c"])[0] == (I(c["r"]), I(c["s"]), c["j"]), (spec["name"], c["tag"], c["hash"])
    for c in spec["sup"]:
        got = G.sign_pass(bytes.fromhex(c["h"]), c["bits"], I(c["d"]), I(c["k"]), c["c"])
        assert (got is not None) == bool(c["ok"]), (spec["name"], c["tag"])
        if got:
            assert got == (I(c["r"]), I(c["s"]), c["j"]), (spec["name"], c["tag"])
    return {c["tag"] for c in spec["verify"]} | {c["tag"] for c in spec["det"]} | {c["tag"] for c in spec["sup"]}


def _hrows(cs):
    return np.stack([np.frombuffer(bytes.fromhex(c["h"]), np.uint8) for c in cs])


def check_golden(ctx, spec, form="host", cid=None):
    """every recorded case through the three calls, one call per (digest length, msgBitLength[, ...])
    group; a 'throws' record expects ELLGPU_E_UNSUPPORTED.  -> the number of cases checked"""
    from elliptic_amd import _lib
    cid = define(ctx, spec) if cid is None else cid
    done = 0
    groups = {}
    for c in spec["verify"]:
        groups.setdefault((len(c["h"]) // 2, c["bits"]), []).append(c)
    for (hl, bits), cs in sorted(groups.items()):
        args = (_hrows(cs), rows([I(c["r"]) for c in cs]), rows([I(c["s"]) for c in cs]), xy_rows([_q(c) for c in cs]))
        ok, st = run_verify(ctx, cid, *args, bits, form)
        ok2, _ = run_verify(ctx, cid, *args, bits, form, want_status=False)
        assert (ok == ok2).all()
        for i, c in enumerate(cs):
            want = (0, 0 if c["tag"] == "off_curve_r_0" else 2) if _off_curve(c) else (c["ok"], 0)
            assert (int(ok[i]), int(st[i])) == want, (spec["name"], "verify", c["tag"], form)
        done += len(cs)
    groups = {}
    for c in spec["det"]:
        groups.setdefault((len(c["h"]) // 2, c["bits"], c["c"], c["hash"], "msg" in c), []).append(c)
    for (hl, bits, can, hname, throws), cs in sorted(groups.items()):
        h, d = _hrows(cs), rows([I(c["d"]) for c in cs])
        if throws:
            try:
                run_sign_det(ctx, cid, h, d, CS.HASH_ID[hname], can, bits, form)
            except _lib.EllgpuError as e:
                assert e.code == -5, e
            else:
                raise AssertionError("custom_ed_sign_det on %s did not refuse" % spec["name"])
        else:
            out = run_sign_det(ctx, cid, h, d, CS.HASH_ID[hname], can, bits, form)
            for i, c in enumerate(cs):
                CS._same(out, i, c, (spec["name"], "det", c["tag"], hname, form))
        done += len(cs)
    groups = {}
    for c in spec["sup"]:
        groups.setdefault((len(c["h"]) // 2, c["bits"], c["c"]), []).append(c)
    for (hl, bits, can), cs in sorted(groups.items()):
        out = run_sign(ctx, cid, _hrows(cs), rows([I(c["d"]) for c in cs]), rows([I(c["k"]) for c in cs]), can, bits, form)
        for i, c in enumerate(cs):
            CS._same(out, i, c, (spec["name"], "sup", c["tag"], form))
        done += len(cs)
    assert done == len(spec["verify"]) + len(spec["det"]) + len(spec["sup"])
    return done


# ---- random batches ---------------------------------------------------------------------------

VALID = "valid"
FAILURES = ["r_flipped", "s_flipped", "digest_flipped", "other_key", "r_0", "s_0", "r_n", "s_n", "p_is_identity",
            "key_identity", "key_small_order", "off_curve"]
_PLAN = [VALID] * 9 + ["r_flipped", "s_flipped", "digest_flipped", "other_key", "range", "special_key", "off_curve"]


def verify_batch(spec, n, seed, distinct=288, hash_len=32):
    """n EC#verify items and the model's answers: a seeded permutation of `distinct` modelled tuples
    (the model takes milliseconds per item).  Nine of sixteen tuples are valid signatures, made from
    random nonces with a pool of eight keys; the others carry one failure class each.  -> dict h, r,
    s, q (byte rows), ok, st, kind (labels), wrapped (valid items with x(k G) >= n)"""
    key = ("verify", spec["name"], n, seed, distinct, hash_len)
    if key in _cache:
        return _cache[key]
    G = group_of(spec)
    p, nn = G.p, G.n
    rng = random.Random("custom-ed-ecdsa:%s:%d" % (spec["name"], seed))
    keys = []
    for _ in range(8):
        d = rng.randrange(1, nn)
        keys.append((d, G.mul(d, G.g)))
    tuples = []
    for i in range(distinct):
        kind = _PLAN[i % len(_PLAN)]
        d, Q = keys[rng.randrange(8)]
        h = rng.randbytes(hash_len)
        while True:
            k = rng.randrange(2, nn - 1)
            R = G.mul(k, G.g)
            sg = G.finish(CS.truncate_msg(nn, h, 0), d, k, R, 0)    # not canonical: -(x, y) = (-x, y), so (r, n - s) does not verify
            if sg:
                break
        r, s = sg[0], sg[1]
        wrapped = R[0] >= nn
        if kind == "r_flipped":
            r ^= 1 << rng.randrange(nn.bit_length() - 1)
        elif kind == "s_flipped":
            s ^= 1 << rng.randrange(nn.bit_length() - 1)
        elif kind == "digest_flipped":
            h = bytes([h[0] ^ 0x80]) + h[1:]
        elif kind == "other_key":
            Q = next(q for _, q in keys if q != Q)
        elif kind == "range":
            kind = ("r_0", "s_0", "r_n", "s_n", "r_n_minus_1")[(i // len(_PLAN)) % 5]
            r, s = {"r_0": (0, s), "s_0": (r, 0), "r_n": (nn, s), "s_n": (r, nn), "r_n_minus_1": (nn - 1, s)}[kind]
        elif kind == "special_key":
            kind = ("p_is_identity", "key_identity", "key_small_order")[(i // len(_PLAN)) % 3]
            if kind == "p_is_identity":
                w = pow(s, -1, nn)
                u1, u2 = CS.truncate_msg(nn, h, 0) * w % nn, r * w % nn
                Q = G.mul(-u1 * pow(u2, -1, nn) % nn, G.g)
            else:
                Q = (0, 1) if kind == "key_identity" else (0, p - 1)
        elif kind == "off_curve":
            Q = (Q[0], (Q[1] + 1 + rng.randrange(p - 2)) % p)
            if G.on_curve(Q):
                Q = (Q[0], (Q[1] + 1) % p)
            if (i // len(_PLAN)) % 4 == 3:
                r = 0                                     # out of range first: status 0
        if kind == VALID and Q[0] + p < CK.TOP and Q[1] + p < CK.TOP and rng.random() < 0.1:
            Q = (Q[0] + p, Q[1] + p)                      # reduced mod p on input, as toRed does
        ok, st = G.verify(h, 0, r, s, Q)
        tuples.append((h, r, s, Q, ok, st, kind, wrapped and kind == VALID))
    order = [j % distinct for j in range(n)]
    random.Random(seed).shuffle(order)
    t = [tuples[j] for j in order]
    out = {"h": np.stack([np.frombuffer(x[0], np.uint8) for x in t]), "r": rows([x[1] for x in t]),
           "s": rows([x[2] for x in t]), "q": xy_rows([x[3] for x in t]), "ok": np.array([x[4] for x in t], np.uint8),
           "st": np.array([x[5] for x in t], np.uint8), "kind": np.array([x[6] for x in t]),
           "wrapped": np.array([x[7] for x in t]), "distinct": tuples}
    _cache[key] = out
    return out


def verify_batch_meets_conditions(spec, bt):
    """on the model alone: at least 40 % valid signatures, every failure class present and refused,
    status 2 present; on the cofactor-4 and cofactor-8 domains at least a quarter of the valid items
    with x(k G) >= n"""
    kinds, ok, st = bt["kind"], bt["ok"], bt["st"]
    valid = kinds == VALID
    good = ok[valid].all() and valid.mean() >= 0.4 and set(FAILURES) <= set(kinds.tolist())
    good = good and not ok[np.isin(kinds, FAILURES)].any() and (st == 2).any() and set(st.tolist()) == {0, 2}
    good = good and ((kinds == "off_curve") & (st == 0)).any()
    if spec["name"] in ("curve1174", "ed25519_by_hand"):
        good = good and bt["wrapped"][valid].mean() >= 0.25
    return bool(good)


def check_verify_batch(ctx, spec, bt, n, form="host", cid=None):
    cid = define(ctx, spec) if cid is None else cid
    ok, st = run_verify(ctx, cid, bt["h"][:n], bt["r"][:n], bt["s"][:n], bt["q"][:n], 0, form)
    bad = np.nonzero((ok != bt["ok"][:n]) | (st != bt["st"][:n]))[0]
    assert bad.size == 0, (spec["name"], n, form, bad[:10].tolist(), bt["kind"][bad[:10]].tolist())
    return ok, st


def _pack(res):
    return CS._pack(res)


def _tile(n, distinct, seed):
    order = [j % distinct for j in range(n)]
    random.Random(seed).shuffle(order)
    return order


def det_batch(spec, n, seed, hname, hash_len, canonical, bits=0, distinct=96):
    """n EC#sign items (a permutation of `distinct` modelled ones): random digests, keys that are any
    32-byte value for one item in four.  -> h, d, r, s, j, ok, draws, wrapped, pub"""
    key = ("det", spec["name"], n, seed, hname, hash_len, canonical, bits, distinct)
    if key in _cache:
        return _cache[key]
    G = group_of(spec)
    rng = random.Random("custom-ed-ecdsa-det:%s:%d" % (spec["name"], seed))
    hs = [rng.randbytes(hash_len) for _ in range(distinct)]
    ds = [rng.getrandbits(256) if i % 4 == 3 else rng.randrange(1, G.n) for i in range(distinct)]
    res = [G.sign_det(hname, hs[i], bits, ds[i], canonical) for i in range(distinct)]
    pubs = [G.mul(d % G.n, G.g) for d in ds]
    o = _tile(n, distinct, seed)
    out = dict(zip(("r", "s", "j", "ok"), _pack([res[j][0] for j in o])))
    out.update(h=np.stack([np.frombuffer(hs[j], np.uint8) for j in o]), d=rows([ds[j] for j in o]),
               draws=np.array([res[j][1] for j in o]), wrapped=np.array([res[j][2] for j in o]),
               pub=xy_rows([pubs[j] for j in o]))
    _cache[key] = out
    return out


def sup_batch(spec, n, seed, hash_len, canonical, bits=0, distinct=96):
    """n items for the supplied-nonce call, the classes of tests/custom_sign_checks.py sup_batch: of
    every eight, item 0 has k <= 1, item 1 a value whose truncation is >= n - 1, item 2 a key chosen so
    that s = 0; the others are candidates as a DRBG would draw them, with a zero top byte (item 3) or
    wider than n.byteLength() where that fits into 32 bytes (item 4)"""
    key = ("sup", spec["name"], n, seed, hash_len, canonical, bits, distinct)
    if key in _cache:
        return _cache[key]
    G = group_of(spec)
    nn = G.n
    nb = (nn.bit_length() + 7) // 8
    full_shift = 8 * nb - nn.bit_length()
    rng = random.Random("custom-ed-ecdsa-sup:%s:%d" % (spec["name"], seed))
    hs = [rng.randbytes(hash_len) for _ in range(distinct)]
    ds = [rng.getrandbits(256) if i % 16 == 5 else rng.randrange(1, nn) for i in range(distinct)]
    vs = []
    for i in range(distinct):
        kind = i % 8
        if kind == 0:
            vs.append(rng.randrange(2))
        elif kind == 1:
            hi = min(nn - 1 + rng.randrange(3), (1 << (8 * nb - full_shift)) - 1)
            vs.append((hi << full_shift) | rng.getrandbits(full_shift) if full_shift else hi)
        elif kind == 3:
            vs.append(rng.getrandbits(8 * nb - 8))
        elif kind == 4 and nb < 32:
            vs.append(rng.getrandbits(256) | (1 << 255))
        else:
            vs.append(int.from_bytes(rng.randbytes(nb), "big"))
    forced = 0
    for i in range(distinct):
        k = CS.truncate_nonce(nn, vs[i])
        if i % 8 == 2 and CS.nonce_in_range(nn, k):
            r = G.mul(k, G.g)[0] % nn
            if r:
                ds[i] = (nn - CS.truncate_msg(nn, hs[i], bits)) * pow(r, -1, nn) % nn
                forced += 1
    res = [G.sign_pass(hs[i], bits, ds[i], vs[i], canonical) for i in range(distinct)]
    assert forced >= distinct // 20 and not any(res[i] for i in range(distinct) if i % 8 in (0, 1, 2))
    o = _tile(n, distinct, seed)
    out = dict(zip(("r", "s", "j", "ok"), _pack([res[j] for j in o])))
    out.update(h=np.stack([np.frombuffer(hs[j], np.uint8) for j in o]), d=rows([ds[j] for j in o]), k=rows([vs[j] for j in o]))
    _cache[key] = out
    return out


def check_det_batch(ctx, spec, bt, n, hname, canonical, bits=0, form="host", cid=None):
    cid = define(ctx, spec) if cid is None else cid
    got = run_sign_det(ctx, cid, bt["h"][:n], bt["d"][:n], CS.HASH_ID[hname], canonical, bits, form)
    assert (got[3] == 1).all(), (spec["name"], n, form, np.nonzero(got[3] != 1)[0][:10])
    CS._compare(got, bt, n, (spec["name"], "det", n, form))
    return got


def check_sup_batch(ctx, spec, bt, n, canonical, bits=0, form="host", cid=None):
    cid = define(ctx, spec) if cid is None else cid
    got = run_sign(ctx, cid, bt["h"][:n], bt["d"][:n], bt["k"][:n], canonical, bits, form)
    assert set(np.unique(got[3]).tolist()) <= {0, 1}
    CS._compare(got, bt, n, (spec["name"], "sup", n, form))
    return got
