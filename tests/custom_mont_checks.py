"""User-defined Montgomery curves (ellgpu_curve_define_mont, ellgpu_custom_mont_ladder / _validate /
_derive): lib/elliptic/curve/mont.js restated over Python integers, the reference's recorded answers
(tests/golden/custom_mont.json, tools/gen_golden_custom_mont.js) and the helpers the hostsim, device
and N-API tests share.

The model is the reference's own shape: Point#mul walks k's exact bit length MSB first with dbl
(dbl-1987-m-3) and diffAdd (dadd-1987-m-3) in projective (X : Z), getX is X / Z with redInvm(0) = 0,
validate is rhs = x^3 + a x^2 + x followed by a square root that answers false on a non-residue where
p = 3 (mod 4) and throws 'Assertion failed' where p = 1 (mod 4), derive is validate, mul, getX.  The
engine walks 256 fixed bits and tests by Euler's criterion; the two must agree item for item.

Every call is run in one of three forms: "host" (host buffers), "dev_np" (the _dev entry point on
the hostsim build, where device memory is host memory) and "dev_torch" (the _dev entry point on
device tensors)."""
import json
import os
import random

import numpy as np

import custom_wire_checks as CW

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "custom_mont.json")
FILL = CW.FILL
TOP = 1 << 256
BIG = ["c25519_user", "m221", "bp256_mont", "top256_mont"]
_cache = {}


def I(s):
    return int(s, 16)


def b32(v):
    return np.frombuffer(int(v).to_bytes(32, "big"), np.uint8)


def rows(vals):
    return np.stack([b32(v) for v in vals]) if len(vals) else np.zeros((0, 32), np.uint8)


def ints(arr):
    return [int.from_bytes(r.tobytes(), "big") for r in arr]


def curves():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
        for c in _cache["golden"]:
            if "rows" in c:
                c["cases"] = [case for r in c["rows"] for case in _row_cases(r)]
    return _cache["golden"]


def _row_cases(r):
    """a row of the toy curve (one x, lists over k = 0, 1, ...) -> cases of the common shape"""
    for k, (z0, gx) in enumerate(zip(r["z0"], r["getx"])):
        c = {"tag": "exhaustive", "k": "%x" % k, "x": "%x" % r["x"], "z0": z0, "getx": "%x" % gx}
        c.update({f: r[f] for f in ("valid", "vmsg", "dmsg") if f in r})
        if "derive" in r:
            c["derive"] = "%x" % r["derive"][k]
        yield c


def spec_of(name):
    return next(c for c in curves() if c["name"] == name)


def params(spec):
    return I(spec["p"]), I(spec["a"])


def define(ctx, spec):
    return ctx.define_mont(*params(spec))


def statuses_of(spec):
    """what derive can answer on the curve"""
    return {0, 3, 2} if I(spec["p"]) % 4 == 1 else {0, 1, 2}


# ---- mont.js over the integers --------------------------------------------------------------

class Model:
    def __init__(self, p, a):
        self.p, self.a = p, a % p
        self.a24 = (self.a + 2) * pow(4, -1, p) % p

    def mul(self, k, x):
        """Point#mul(k) of (x : 1) -> (X, Z), mont.js:130-153 with dbl (:82-101) and diffAdd (:107-128)
        written out in the loop (thousands of items go through here): A, B are the reference's a, b;
        S = A + B by diffAdd, D the double of the one the bit selects"""
        p, a24 = self.p, self.a24
        x %= p
        AX, AZ, BX, BZ = x, 1, 1, 0
        for bit in bin(k)[2:] if k else "":
            da = (BX - BZ) * (AX + AZ)
            cb = (BX + BZ) * (AX - AZ)
            SX, SZ = (da + cb) ** 2 % p, x * ((da - cb) ** 2 % p) % p
            TX, TZ = (AX, AZ) if bit == "1" else (BX, BZ)
            aa = (TX + TZ) ** 2 % p
            bb = (TX - TZ) ** 2 % p
            c = aa - bb
            DX, DZ = aa * bb % p, c * (bb + a24 * c) % p
            if bit == "1":
                AX, AZ, BX, BZ = DX, DZ, SX, SZ
            else:
                AX, AZ, BX, BZ = SX, SZ, DX, DZ
        return BX, BZ

    def ladder(self, k, x):
        """-> (getX(), [Z == 0]); getX is 0 where Z == 0 (redInvm of 0 is 0)"""
        X, Z = self.mul(k, x)
        if Z % self.p == 0:
            return 0, 1
        return X * pow(Z, -1, self.p) % self.p, 0

    def is_square(self, x):
        p = self.p
        x %= p
        rhs = (x * x * x + self.a * x * x + x) % p
        return rhs == 0 or pow(rhs, (p - 1) // 2, p) == 1

    def validate(self, x):
        """0 true, 1 false, 3 'Assertion failed'"""
        if self.is_square(x):
            return 0
        return 3 if self.p % 4 == 1 else 1

    def derive(self, k, x):
        """-> (x, status): validation first, then 2 where Z == 0"""
        v = self.validate(x)
        if v:
            return 0, v
        gx, inf = self.ladder(k, x)
        return (0, 2) if inf else (gx, 0)


def model_of(spec):
    return Model(*params(spec))


# ---- the three forms of the calls -----------------------------------------------------------

def _P(a):
    return a.ctypes.data if a is not None else None


def _filled(*shapes):
    return [np.full(s, FILL, np.uint8) for s in shapes]


def run_ladder(ctx, cid, k, x, form="host"):
    k, x = (np.ascontiguousarray(a, np.uint8).reshape(-1, 32) for a in (k, x))
    n = k.shape[0]
    ox, inf = _filled((n, 32), (n,))
    if form == "host":
        ctx.custom_mont_ladder(cid, k, x, out=(ox, inf))
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_mont_ladder_dev(ctx._ctx, cid, n, _P(k), _P(x), _P(ox), _P(inf), None))
    else:
        ox, inf = CW._torch_call(lambda i, o: ctx.custom_mont_ladder_dev(cid, i[0], i[1], o[0], o[1]), [k, x], [ox, inf])
    return ox, inf


def run_validate(ctx, cid, x, form="host"):
    x = np.ascontiguousarray(x, np.uint8).reshape(-1, 32)
    n = x.shape[0]
    st, = _filled((n,))
    if form == "host":
        ctx.custom_mont_validate(cid, x, out=(st,))
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_mont_validate_dev(ctx._ctx, cid, n, _P(x), _P(st), None))
    else:
        st, = CW._torch_call(lambda i, o: ctx.custom_mont_validate_dev(cid, i[0], o[0]), [x], [st])
    return st


def run_derive(ctx, cid, k, x, form="host"):
    k, x = (np.ascontiguousarray(a, np.uint8).reshape(-1, 32) for a in (k, x))
    n = k.shape[0]
    ox, st = _filled((n, 32), (n,))
    if form == "host":
        ctx.custom_mont_derive(cid, k, x, out=(ox, st))
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_mont_derive_dev(ctx._ctx, cid, n, _P(k), _P(x), _P(ox), _P(st), None))
    else:
        ox, st = CW._torch_call(lambda i, o: ctx.custom_mont_derive_dev(cid, i[0], i[1], o[0], o[1]), [k, x], [ox, st])
    return ox, st


# ---- the recorded cases ---------------------------------------------------------------------

VMSG = {"Assertion failed": 3}
DMSG = {"public point not validated": 1, "Assertion failed": 3}


def expected(c):
    """a recorded case -> (ladder x, inf, validate status, derive x, derive status) as the engine
    answers: where Z == 0 the reference's getX() and derive return 0, the engine flags the item"""
    vst = 1 - c["valid"] if "valid" in c else VMSG[c["vmsg"]]
    if "derive" in c:
        assert vst == 0 and c["derive"] == c["getx"]
        dx, dst = (0, 2) if c["z0"] else (I(c["derive"]), 0)
    else:
        dx, dst = 0, DMSG[c["dmsg"]]
        assert dst == vst
    if c["z0"]:
        assert I(c["getx"]) == 0
    return I(c["getx"]), c["z0"], vst, dx, dst


def check_golden(ctx, spec, form="host", cid=None):
    """every recorded case through the three calls, and through the model; -> the derive statuses seen"""
    cid = define(ctx, spec) if cid is None else cid
    cs = spec["cases"]
    m = model_of(spec)
    assert I(spec["a24"]) == m.a24 and spec["pmod4"] == m.p % 4
    want = [expected(c) for c in cs]
    k, x = rows([I(c["k"]) for c in cs]), rows([I(c["x"]) for c in cs])
    for c, w in zip(cs, want):
        kk, xx = I(c["k"]), I(c["x"])
        assert m.ladder(kk, xx) == w[:2] and m.validate(xx) == w[2] and m.derive(kk, xx) == w[3:], c["tag"]
    ox, inf = run_ladder(ctx, cid, k, x, form)
    vst = run_validate(ctx, cid, x, form)
    dx, dst = run_derive(ctx, cid, k, x, form)
    got = list(zip(ints(ox), inf.tolist(), vst.tolist(), ints(dx), dst.tolist()))
    for c, w, g in zip(cs, want, got):
        assert g == w, (spec["name"], c["tag"], c["k"], c["x"], g, w)
    return set(dst.tolist())


# ---- random batches -------------------------------------------------------------------------

def random_batch(spec, n, seed):
    """n items and the model's answers.  About 70 % abscissae of the curve (chosen by Euler's
    criterion here), about 20 % non-residues, the rest k = 0 and x = 0 in turn; the first four items
    are one of each kind, so that every status shows in any prefix of four or more.  A third of the
    scalars have a random bit length below 256 (the leading-zero rounds), the others are 256-bit
    draws; a tenth of the abscissae that fit are given as x + p."""
    rng = random.Random("custom-mont:%s:%d" % (spec["name"], seed))
    m = model_of(spec)
    p = m.p
    ks, xs, kinds = [], [], []
    for i in range(n):
        r = rng.random()
        kind = i if i < 4 else (0 if r < 0.70 else 1 if r < 0.90 else 2 + (i & 1))
        k = rng.getrandbits(256) if rng.random() < 0.65 else rng.getrandbits(rng.randrange(1, 256)) | 1
        if kind != 3:
            while True:
                x = rng.randrange(1, p)
                if m.is_square(x) == (kind != 1):
                    break
            if x + p < TOP and rng.random() < 0.1:
                x += p
            if kind == 2:
                k = 0                                    # on an abscissa of the curve: status 2, not the non-residue's
        else:
            x = 0
        ks.append(k)
        xs.append(x)
        kinds.append(kind)
    lad = [m.ladder(k, x) for k, x in zip(ks, xs)]
    vst = [m.validate(x) for x in xs]
    der = [(0, v) if v else ((0, 2) if l[1] else (l[0], 0)) for v, l in zip(vst, lad)]
    return {"k": rows(ks), "x": rows(xs), "ks": ks, "xs": xs, "kind": np.array(kinds),
            "ox": rows([l[0] for l in lad]), "inf": np.array([l[1] for l in lad], np.uint8),
            "vst": np.array(vst, np.uint8), "dx": rows([d[0] for d in der]),
            "dst": np.array([d[1] for d in der], np.uint8), "statuses": statuses_of(spec)}


def model_meets_conditions(bt, n):
    """every status the curve can give occurs within the first 257 items, and at least 60 % of the
    n items are shared secrets"""
    head = set(bt["dst"][:min(n, 257)].tolist())
    return head == bt["statuses"] and (bt["dst"][:n] == 0).sum() >= 0.6 * n


def check_batch(ctx, spec, bt, n, form="host", cid=None):
    """the first n items of a batch through the three calls"""
    cid = define(ctx, spec) if cid is None else cid
    ox, inf = run_ladder(ctx, cid, bt["k"][:n], bt["x"][:n], form)
    assert (inf == bt["inf"][:n]).all() and (ox == bt["ox"][:n]).all(), (spec["name"], n, form)
    vst = run_validate(ctx, cid, bt["x"][:n], form)
    assert (vst == bt["vst"][:n]).all(), (spec["name"], n, form)
    dx, dst = run_derive(ctx, cid, bt["k"][:n], bt["x"][:n], form)
    assert (dst == bt["dst"][:n]).all() and (dx == bt["dx"][:n]).all(), (spec["name"], n, form)
    return ox, inf, vst, dx, dst


def base_point(spec):
    """G = (9 : 1) on curve25519 written out by hand, elsewhere the least abscissa >= 2 of the curve"""
    if spec["name"] == "c25519_user":
        return 9
    m = model_of(spec)
    return next(x for x in range(2, 1000) if m.is_square(x))


def check_symmetry(ctx, spec, n, seed, form="host", cid=None):
    """derive(a, x(b G)) = derive(b, x(a G)) through the engine alone"""
    cid = define(ctx, spec) if cid is None else cid
    rng = random.Random("custom-mont-ecdh:%s:%d" % (spec["name"], seed))
    a = rows([rng.getrandbits(256) for _ in range(n)])
    b = rows([rng.getrandbits(256) for _ in range(n)])
    g = rows([base_point(spec)] * n)
    xa, ia = run_ladder(ctx, cid, a, g, form)
    xb, ib = run_ladder(ctx, cid, b, g, form)
    assert not ia.any() and not ib.any()
    s1, st1 = run_derive(ctx, cid, a, xb, form)
    s2, st2 = run_derive(ctx, cid, b, xa, form)
    assert not st1.any() and not st2.any() and (s1 == s2).all() and s1.any(axis=1).all()
