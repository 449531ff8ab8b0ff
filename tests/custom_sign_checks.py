"""Checks of EC#sign on user-defined ECDSA domains (ellgpu_custom_sign, ellgpu_custom_sign_det),
shared by the CPU test (tests/test_custom_sign_hostsim.py, the hostsim build of the device code)
and the GPU test (tests/test_custom_sign_gpu.py):

  * the reference's own signatures, acceptances and thrown messages recorded in
    tests/golden/custom_sign.json (tools/gen_golden_custom_sign.js);
  * random batches against a model over Python integers that restates EC#sign
    (ec/index.js:110-186) step by step with stdlib hmac and hashlib: msg = _truncateToN(hash, false,
    bits) with its one subtraction, priv mod n, HmacDRBG (hmac-drbg 1.0.1) seeded with both as
    n.byteLength() bytes, k = _truncateToN(candidate, true) whose shift depends on the candidate's
    own byte length, the rejections (k <= 1, k >= n - 1, k G = O, r = 0, s = 0), r = x mod n as a
    general reduction, recoveryParam = (y odd) | (x != r ? 2 : 0), s = k^-1 (msg + r priv) and the
    canonical form -- with at most MAX_DRAWS candidates per item, and the draw count reported.

k G is computed by the C oracle for a batch and over Python integers alone (affine additions) for
the fixture's cases and a sample of every batch, which must agree.

Every call is run in one of three forms: "host" (host buffers), "dev_np" (the _dev entry point on
the hostsim build, where device memory is host memory) and "dev_torch" (the _dev entry point on
torch tensors).  Result arrays are pre-filled with 0xA5, so a byte the call leaves unwritten shows."""
import hashlib
import hmac
import json
import os
import random

import numpy as np

import custom_domain_checks as CD
import custom_recover_checks as CR
import custom_wire_checks as CW

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "custom_sign.json")
FILL = CW.FILL
MAX_DRAWS = 64                                   # ELLGPU_CUSTOM_SIGN_MAX_DRAWS
HASH_ID = {"sha256": 0, "sha384": 1, "sha512": 2}
ENTROPY = "Not enough entropy. Minimum is: 192 bits"
SAMPLE_HEAD, SAMPLE_STEP = 8, 331

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


def rows(vals):
    return np.stack([b32(v) for v in vals]) if len(vals) else np.zeros((0, 32), np.uint8)


def ints(a):
    return [int.from_bytes(x.tobytes(), "big") for x in a]


# ---- the forms of the two calls --------------------------------------------------------------

def _filled(n):
    return [np.full(sh, FILL, np.uint8) for sh in ((n, 32), (n, 32), (n,), (n,))]


def run_sign(ctx, cid, h, d, k, canonical=0, bits=0, form="host"):
    h, d, k = (np.ascontiguousarray(a, np.uint8) for a in (h, d, k))
    n, hl = h.shape
    out = _filled(n)
    if form == "host":
        ctx.custom_sign(cid, h, d, k, canonical=canonical, msg_bits=bits, out=out)
    elif form == "dev_np":
        P = lambda a: a.ctypes.data
        CW._raw(ctx, ctx._lib.ellgpu_custom_sign_dev(ctx._ctx, cid, n, P(h), hl, bits, P(d), P(k), canonical,
                                                     *[P(o) for o in out], None))
    else:
        out = CW._torch_call(lambda i, o: ctx.custom_sign_dev(cid, i[0], i[1], i[2], o[0], o[1], o[2], o[3],
                                                              canonical=canonical, msg_bits=bits), [h, d, k], out)
    return out


def run_sign_det(ctx, cid, h, d, drbg_hash, canonical=0, bits=0, form="host"):
    h, d = (np.ascontiguousarray(a, np.uint8) for a in (h, d))
    n, hl = h.shape
    out = _filled(n)
    if form == "host":
        ctx.custom_sign_det(cid, h, d, drbg_hash=drbg_hash, canonical=canonical, msg_bits=bits, out=out)
    elif form == "dev_np":
        P = lambda a: a.ctypes.data
        CW._raw(ctx, ctx._lib.ellgpu_custom_sign_det_dev(ctx._ctx, cid, n, P(h), hl, bits, P(d), drbg_hash, canonical,
                                                         *[P(o) for o in out], None))
    else:
        out = CW._torch_call(lambda i, o: ctx.custom_sign_det_dev(cid, i[0], i[1], o[0], o[1], o[2], o[3],
                                                                  drbg_hash=drbg_hash, canonical=canonical,
                                                                  msg_bits=bits), [h, d], out)
    return out


# ---- EC#sign over Python integers --------------------------------------------------------------

def truncate_msg(n, h, bits=0):
    """_truncateToN(h, false, bits) of a byte string: the shift, then ONE subtraction of n"""
    m = int.from_bytes(h, "big")
    delta = (bits or 8 * len(h)) - n.bit_length()
    if delta > 0:
        m >>= delta
    return m - n if m >= n else m


def truncate_nonce(n, v):
    """_truncateToN(v, true) of a BN: the shift comes from the VALUE's byte length"""
    delta = 8 * ((v.bit_length() + 7) // 8) - n.bit_length()
    return v >> delta if delta > 0 else v


def nonce_in_range(n, k):
    return 1 < k < n - 1


class HmacDrbg:
    """hmac-drbg 1.0.1 (lib/hmac-drbg.js) without pers or additional input"""

    def __init__(self, hname, entropy, nonce):
        self.h = getattr(hashlib, hname)
        size = self.h().digest_size
        self.K, self.V = bytes(size), b"\x01" * size
        self._update(entropy + nonce)

    def _mac(self, data):
        return hmac.new(self.K, data, self.h).digest()

    def _update(self, seed=b""):
        self.K = self._mac(self.V + b"\x00" + seed)
        self.V = self._mac(self.V)
        if seed:
            self.K = self._mac(self.V + b"\x01" + seed)
            self.V = self._mac(self.V)

    def generate(self, length):
        out = b""
        while len(out) < length:
            self.V = self._mac(self.V)
            out += self.V
        self._update()
        return out[:length]


def finish(spec, msg, priv, k, R, canonical):
    """the loop's body behind the range test, R = k G as (x, y) or None -> (r, s, j) or None"""
    n = CD.params(spec)[3]
    if R is None:
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


def mul_g(spec, k):
    p, a, b, n, gx, gy = CD.params(spec)
    return CR.pt_mul_add(p, a, k, (gx, gy), 0, None)


def model_pass(spec, h, bits, d, v, canonical, R=False):
    """one pass of the loop for the supplied nonce v -> (r, s, j) or None; R: k G where the caller
    has it (else computed here over integers)"""
    n = CD.params(spec)[3]
    k = truncate_nonce(n, v)
    if not nonce_in_range(n, k):
        return None
    return finish(spec, truncate_msg(n, h, bits), d, k, mul_g(spec, k) if R is False else R, canonical)


def det_candidates(spec, hname, h, bits, d):
    """-> (draws, v, k): the first candidate in range, the number of generate() calls it took
    (None, None beyond MAX_DRAWS)"""
    n = CD.params(spec)[3]
    nb = (n.bit_length() + 7) // 8
    if nb < 24:
        raise ValueError(ENTROPY)
    g = HmacDrbg(hname, (d % n).to_bytes(nb, "big"), truncate_msg(n, h, bits).to_bytes(nb, "big"))
    for it in range(MAX_DRAWS):
        v = int.from_bytes(g.generate(nb), "big")
        k = truncate_nonce(n, v)
        if nonce_in_range(n, k):
            return it + 1, v, k
    return MAX_DRAWS, None, None


def model_det(spec, hname, h, bits, d, canonical):
    """EC#sign for one item over integers alone -> ((r, s, j) or None, draws)"""
    draws, v, k = det_candidates(spec, hname, h, bits, d)
    if v is None:
        return None, draws
    got = finish(spec, truncate_msg(CD.params(spec)[3], h, bits), d, k, mul_g(spec, k), canonical)
    assert got is not None          # k G = O, r = 0 or s = 0: the reference would draw again; as likely as guessing a key
    return got, draws


# ---- the reference's recorded answers ------------------------------------------------------------

def check_model_against_golden(spec):
    """the model alone against the fixture, so that a model error cannot hide behind agreement with
    the kernel; returns the largest draw count seen"""
    most = 0
    for c in spec["det"]:
        h, d = bytes.fromhex(c["h"]), I(c["d"])
        if "msg" in c:
            assert c["msg"] == ENTROPY
            try:
                model_det(spec, c["hash"], h, c["bits"], d, c["c"])
            except ValueError as e:
                assert str(e) == ENTROPY
            else:
                raise AssertionError((spec["name"], c["tag"]))
            continue
        got, draws = model_det(spec, c["hash"], h, c["bits"], d, c["c"])
        assert got == (I(c["r"]), I(c["s"]), c["j"]), (spec["name"], c["tag"], c["hash"])
        most = max(most, draws)
    for c in spec["sup"]:
        got = model_pass(spec, bytes.fromhex(c["h"]), c["bits"], I(c["d"]), I(c["k"]), c["c"])
        assert (got is not None) == bool(c["ok"]), (spec["name"], c["tag"])
        if got:
            assert got == (I(c["r"]), I(c["s"]), c["j"]), (spec["name"], c["tag"])
    return most


def _want(c):
    if c.get("ok", 1) and "r" in c:
        return b32(I(c["r"])).tobytes(), b32(I(c["s"])).tobytes(), c["j"], 1
    return bytes(32), bytes(32), 0, 0


def _same(out, i, c, what):
    r, s, j, ok = out
    assert (r[i].tobytes(), s[i].tobytes(), int(j[i]), int(ok[i])) == _want(c), what


def check_golden(ctx, spec, form="host", cid=None):
    """every recorded case through the two calls, one call per (digest length, msgBitLength,
    canonical[, hash]) group; a 'throws' record expects ELLGPU_E_UNSUPPORTED.  Returns the number
    of cases checked"""
    from elliptic_amd import _lib
    cid = define(ctx, spec) if cid is None else cid
    done = 0
    groups = {}
    for c in spec["det"]:
        groups.setdefault((len(c["h"]) // 2, c["bits"], c["c"], c["hash"], "msg" in c), []).append(c)
    for (hl, bits, can, hname, throws), cs in sorted(groups.items()):
        h = np.stack([np.frombuffer(bytes.fromhex(c["h"]), np.uint8) for c in cs])
        d = rows([I(c["d"]) for c in cs])
        if throws:
            try:
                run_sign_det(ctx, cid, h, d, HASH_ID[hname], can, bits, form)
            except _lib.EllgpuError as e:
                assert e.code == -5, e
            else:
                raise AssertionError("custom_sign_det on %s did not refuse" % spec["name"])
        else:
            out = run_sign_det(ctx, cid, h, d, HASH_ID[hname], can, bits, form)
            for i, c in enumerate(cs):
                _same(out, i, c, (spec["name"], "det", c["tag"], hname, form))
        done += len(cs)
    groups = {}
    for c in spec["sup"]:
        groups.setdefault((len(c["h"]) // 2, c["bits"], c["c"]), []).append(c)
    for (hl, bits, can), cs in sorted(groups.items()):
        h = np.stack([np.frombuffer(bytes.fromhex(c["h"]), np.uint8) for c in cs])
        out = run_sign(ctx, cid, h, rows([I(c["d"]) for c in cs]), rows([I(c["k"]) for c in cs]), can, bits, form)
        for i, c in enumerate(cs):
            _same(out, i, c, (spec["name"], "sup", c["tag"], form))
        done += len(cs)
    assert done == len(spec["det"]) + len(spec["sup"])
    return done


# ---- random batches ---------------------------------------------------------------------------

def _mul_g_batch(spec, ks):
    """k G for every k (all in range) by the C oracle, a sample again over integers"""
    from oracle import c_oracle
    pts, inf = c_oracle.mul_mt(CD.oracle_name(spec), rows(ks), threads=8)
    assert not inf.any()
    out = [(int.from_bytes(q[:32].tobytes(), "big"), int.from_bytes(q[32:].tobytes(), "big")) for q in pts]
    for i in range(len(ks)):
        if i < SAMPLE_HEAD or i % SAMPLE_STEP == 0:
            assert out[i] == mul_g(spec, ks[i]), (spec["name"], i)
    return out


def _pack(res):
    cnt = len(res)
    r, s = np.zeros((cnt, 32), np.uint8), np.zeros((cnt, 32), np.uint8)
    j, ok = np.zeros(cnt, np.uint8), np.zeros(cnt, np.uint8)
    for i, g in enumerate(res):
        if g is not None:
            r[i], s[i], j[i], ok[i] = b32(g[0]), b32(g[1]), g[2], 1
    return r, s, j, ok


def det_batch(spec, cnt, seed, hname, hash_len, canonical, bits=0):
    """cnt EC#sign items: random digests, keys that are any 32-byte value for one item in four.
    -> dict h, d (byte rows), r, s, j, ok (the model's answers), draws, pub (priv mod n times G)"""
    key = ("det", spec["name"], cnt, seed, hname, hash_len, canonical, bits)
    if key in _cache:
        return _cache[key]
    n = CD.params(spec)[3]
    rnd = random.Random(seed)
    h = np.frombuffer(rnd.randbytes(cnt * hash_len), np.uint8).reshape(cnt, hash_len).copy()
    d = [rnd.getrandbits(256) if i % 4 == 3 else rnd.randrange(1, n) for i in range(cnt)]
    cand = [det_candidates(spec, hname, h[i].tobytes(), bits, d[i]) for i in range(cnt)]
    assert all(c[1] is not None for c in cand)
    pts = _mul_g_batch(spec, [c[2] for c in cand] + [x % n for x in d])
    res = [finish(spec, truncate_msg(n, h[i].tobytes(), bits), d[i], cand[i][2], pts[i], canonical) for i in range(cnt)]
    assert all(g is not None for g in res)
    out = dict(zip(("r", "s", "j", "ok"), _pack(res)))
    out.update(h=h, d=rows(d), draws=np.array([c[0] for c in cand]),
               pub=np.stack([np.concatenate([b32(q[0]), b32(q[1])]) for q in pts[cnt:]]))
    for v in out.values():
        v.setflags(write=False)
    _cache[key] = out
    return out


def sup_batch(spec, cnt, seed, hash_len, canonical, bits=0):
    """cnt items for the supplied-nonce call.  Of every eight: item 0 has k <= 1, item 1 a value
    whose truncation is >= n - 1, item 2 a key chosen so that s = 0 (priv = -msg / r); the others
    are candidates as a DRBG would draw them (n.byteLength() random bytes: where n lies just above
    a power of two about half of them are out of range), with a zero top byte (item 3) or wider
    than n.byteLength() where that fits into 32 bytes (item 4).  The two remaining classes cannot be
    built on these domains: k G = O needs k = 0 (mod n), and r = 0 a point whose x is a multiple of n."""
    key = ("sup", spec["name"], cnt, seed, hash_len, canonical, bits)
    if key in _cache:
        return _cache[key]
    n = CD.params(spec)[3]
    nb = (n.bit_length() + 7) // 8
    full_shift = 8 * nb - n.bit_length()
    rnd = random.Random(seed)
    h = np.frombuffer(rnd.randbytes(cnt * hash_len), np.uint8).reshape(cnt, hash_len).copy()
    d = [rnd.getrandbits(256) if i % 16 == 5 else rnd.randrange(1, n) for i in range(cnt)]
    v = []
    for i in range(cnt):
        kind = i % 8
        if kind == 0:
            v.append(rnd.randrange(2))
        elif kind == 1:
            hi = min(n - 1 + rnd.randrange(3), (1 << (8 * nb - full_shift)) - 1)
            v.append((hi << full_shift) | rnd.getrandbits(full_shift) if full_shift else hi)
        elif kind == 3:
            v.append(rnd.getrandbits(8 * nb - 8))
        elif kind == 4 and nb < 32:
            v.append(rnd.getrandbits(256) | (1 << 255))
        else:
            v.append(int.from_bytes(rnd.randbytes(nb), "big"))
    ks = [truncate_nonce(n, x) for x in v]
    live = [nonce_in_range(n, k) for k in ks]
    pts = _mul_g_batch(spec, [k if ok else 2 for k, ok in zip(ks, live)])
    forced = 0
    for i in range(cnt):
        if i % 8 == 2 and live[i]:
            r = pts[i][0] % n
            d[i] = (n - truncate_msg(n, h[i].tobytes(), bits)) * pow(r, -1, n) % n
            forced += 1
    res = [finish(spec, truncate_msg(n, h[i].tobytes(), bits), d[i], ks[i], pts[i], canonical) if live[i] else None
           for i in range(cnt)]
    out = dict(zip(("r", "s", "j", "ok"), _pack(res)))
    out.update(h=h, d=rows(d), k=rows(v), live=np.array(live))
    if cnt >= 64:
        assert forced >= cnt // 20 and not any(out["ok"][i] for i in range(cnt) if i % 8 in (0, 1))
    for x in out.values():
        x.setflags(write=False)
    _cache[key] = out
    return out


def _compare(got, bt, cnt, what):
    for name, g in zip(("ok", "r", "s", "j"), (got[3], got[0], got[1], got[2])):
        w = bt[name][:cnt]
        bad = np.nonzero((g != w).reshape(cnt, -1).any(axis=1))[0]
        assert bad.size == 0, what + (name, bad[:10].tolist())


def check_det_batch(ctx, spec, bt, cnt, hname, canonical, bits=0, form="host", cid=None):
    cid = define(ctx, spec) if cid is None else cid
    got = run_sign_det(ctx, cid, bt["h"][:cnt], bt["d"][:cnt], HASH_ID[hname], canonical, bits, form)
    assert (got[3] == 1).all(), (spec["name"], cnt, form, np.nonzero(got[3] != 1)[0][:10])
    _compare(got, bt, cnt, (spec["name"], "det", cnt, form))
    return got


def check_sup_batch(ctx, spec, bt, cnt, canonical, bits=0, form="host", cid=None):
    cid = define(ctx, spec) if cid is None else cid
    got = run_sign(ctx, cid, bt["h"][:cnt], bt["d"][:cnt], bt["k"][:cnt], canonical, bits, form)
    assert set(np.unique(got[3]).tolist()) <= {0, 1}
    _compare(got, bt, cnt, (spec["name"], "sup", cnt, form))
    return got


# ---- the round trip, with calls that were there before -------------------------------------------

def check_round_trip(ctx, spec, bt, cnt, got, bits=0, cid=None):
    """Q = mul_fixed(priv mod n) is the expected key: every signature verifies on the domain, and
    ellgpu_custom_recover(the digest truncated by the caller, r, s, recid) returns Q on a
    cofactor-1 domain; on a cofactor curve it answers what the recovery model does (x = r also
    belongs to points outside the subgroup, in the reference too)"""
    cid = define(ctx, spec) if cid is None else cid
    p, a, b, n = CD.params(spec)[:4]
    r, s, j, ok = got
    dm = rows([x % n for x in ints(bt["d"][:cnt])])
    q, inf = ctx.mul_fixed(cid, dm)
    assert not inf.any()
    if "pub" in bt:
        assert (q == bt["pub"][:cnt]).all()
    acc = np.nonzero(ok)[0]
    ver = ctx.ecdsa_verify(cid, bt["h"][:cnt][acc], r[acc], s[acc], q[acc], msg_bits=bits)
    assert (ver == 1).all(), (spec["name"], acc[np.nonzero(ver != 1)[0][:10]])
    e = rows([truncate_msg(n, bt["h"][i].tobytes(), bits) for i in acc])
    xy, st = ctx.custom_recover(cid, e, r[acc], s[acc], j[acc])
    if p // n <= 1:                    # cofactor 1 (Hasse: n is within 2 sqrt(p) of p + 1)
        assert (st == 0).all() and (xy == q[acc]).all(), spec["name"]
    else:
        wst, wxy = CR.model(spec, e, r[acc], s[acc], j[acc])
        assert (st == wst).all() and (xy == wxy).all(), spec["name"]
    return len(acc)
