"""Fixed-base tables of caller-chosen points on Edwards curves (ellgpu_ed_base_define, then
ellgpu_mul_base / ellgpu_mul_base2 on its handles): the reference's recorded answers
(tests/golden/fixed_base_ed.json, tools/gen_golden_fixed_base_ed.js), a Python-integer model of the
affine Edwards law and the helpers the hostsim, device and N-API tests share.

The model is the affine law a x^2 + y^2 = 1 + d x^2 y^2 (complete on every curve of the fixture: a is
a square, d is not) under plain double-and-add.  The fixture records a digest per answer -- the first
8 bytes of SHA-256(inf || x || y), the identity as inf = 1 beside (0, 1) -- and check_model_pinned
holds the model to every one of them before anything else relies on it.

What the engine writes: x || y, and inf = 1 at the identity on ed25519 (Point#isInfinity), inf = 0
always on a user-defined id -- what ellgpu_mul_var writes on the same id (`answer`).

The memory kinds "host", "dev_np" and "dev_torch" are those of tests/fixed_base_checks.py, whose
callers (run_mul, run_mul2) take these handles unchanged."""
import json
import os
import random

import numpy as np

import fixed_base_checks as FB
from fixed_base_checks import I, rows, xy_bytes, run_mul, run_mul2, digest  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fixed_base_ed.json")
NAMES = ["ed25519", "curve1174", "e222", "ed25519_by_hand"]
USER = NAMES[1:]
B = 32
_cache = {}


def curves():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
    return _cache["golden"]


def spec_of(name):
    return next(c for c in curves() if c["name"] == name)


class Model:
    """a x^2 + y^2 = 1 + d x^2 y^2 over p; points are (x, y) tuples, the identity is (0, 1)"""
    ID = (0, 1)

    def __init__(self, p, a, d):
        self.p, self.a, self.d = p, a % p, d % p

    def on_curve(self, P):
        x2, y2 = P[0] * P[0], P[1] * P[1]
        return (self.a * x2 + y2 - 1 - self.d * x2 * y2) % self.p == 0

    def add(self, P, Q):
        p = self.p
        t = self.d * P[0] * Q[0] * P[1] * Q[1] % p
        x = (P[0] * Q[1] + P[1] * Q[0]) * pow(1 + t, -1, p) % p
        y = (P[1] * Q[1] - self.a * P[0] * Q[0]) * pow(1 - t, -1, p) % p
        return x, y

    def neg(self, P):
        return -P[0] % self.p, P[1]

    def mul(self, k, P):
        R = self.ID
        for bit in bin(k)[2:] if k else "":
            R = self.add(R, R)
            if bit == "1":
                R = self.add(R, P)
        return R

    def mul2(self, k1, P1, k2, P2):
        return self.add(self.mul(k1, P1), self.mul(k2, P2))


def model_of(spec):
    return Model(I(spec["p"]), I(spec["a"]), I(spec["d"]))


def bases_of(spec):
    return [(I(x), I(y)) for x, y in spec["bases"]]


def answer(spec, P):
    """a model point -> (x || y row, inf) as the engine writes it on this curve"""
    return np.frombuffer(xy_bytes(P, B), np.uint8), 1 if spec["kind"] == "preset" and P == Model.ID else 0


def golden_answers(spec):
    """the model's answers for every recorded case, computed once per curve:
    -> (mul: per base (xy (n, 64), inf (n,)), pairs: (xy, inf))"""
    key = ("answers", spec["name"])
    if key not in _cache:
        m, pts = model_of(spec), bases_of(spec)
        ks = [I(k) for k in spec["k"]]
        mul = []
        for P in pts:
            a = [answer(spec, m.mul(k, P)) for k in ks]
            mul.append((np.stack([x for x, _ in a]), np.array([f for _, f in a], np.uint8)))
        a = [answer(spec, m.mul2(I(k1), pts[i1], I(k2), pts[i2])) for i1, i2, k1, k2, _ in spec["pairs"]]
        _cache[key] = (mul, (np.stack([x for x, _ in a]), np.array([f for _, f in a], np.uint8)))
    return _cache[key]


def _is_id(xy_row):
    return not xy_row[:63].any() and xy_row[63] == 1


def check_model_pinned(spec):
    """every digest of the fixture from the model's coordinates (the digest's inf byte is
    Point#isInfinity on every curve, whatever the engine writes there)"""
    mul, pairs = golden_answers(spec)
    dg = lambda row: digest(row, 1 if _is_id(row) else 0)
    for bi, (xy, _) in enumerate(mul):
        assert [dg(xy[j]) for j in range(len(xy))] == spec["mul"][bi], (spec["name"], bi)
    assert [dg(pairs[0][j]) for j in range(len(pairs[0]))] == [q[4] for q in spec["pairs"]], spec["name"]


# ---- the engine's side ----------------------------------------------------------------------

def curve_id(ctx, spec):
    """the preset's name, or the id of the user-defined Edwards curve (a domain where the fixture says so)"""
    if spec["kind"] == "preset":
        return spec["name"]
    p, a, d = I(spec["p"]), I(spec["a"]), I(spec["d"])
    if spec["kind"] == "domain":
        return ctx.define_edwards_domain(p, a, d, I(spec["n"]), I(spec["g"][0]), I(spec["g"][1]))
    return ctx.define_edwards(p, a, d)


def define_bases(ctx, spec, width=0, cid=None, which=None):
    """-> (curve id, {index: handle}) for the fixture's bases `which` (default: all)"""
    cid = curve_id(ctx, spec) if cid is None else cid
    pts = bases_of(spec)
    return cid, {i: ctx.define_ed_base(cid, xy_bytes(pts[i], B), width) for i in (range(len(pts)) if which is None else which)}


def release(ctx, hs):
    for h in set(hs.values() if isinstance(hs, dict) else hs):
        ctx.release_base(h)


def check_golden(ctx, spec, hs, mem):
    """every recorded case over the handles hs (define_bases) through one memory kind; -> the bytes
    the engine wrote"""
    mul, pairs = golden_answers(spec)
    k = rows([I(v) for v in spec["k"]], B)
    got = []
    for bi in sorted(hs):
        xy, inf = run_mul(ctx, hs[bi], k, B, mem)
        assert (inf == mul[bi][1]).all() and (xy == mul[bi][0]).all(), (spec["name"], mem, bi)
        got.append((xy, inf))
    for i1, i2 in sorted({(q[0], q[1]) for q in spec["pairs"]}):
        idx = [j for j, q in enumerate(spec["pairs"]) if (q[0], q[1]) == (i1, i2)]
        k1 = rows([I(spec["pairs"][j][2]) for j in idx], B)
        k2 = rows([I(spec["pairs"][j][3]) for j in idx], B)
        xy, inf = run_mul2(ctx, hs[i1], hs[i2], k1, k2, B, mem)
        assert (inf == pairs[1][idx]).all() and (xy == pairs[0][idx]).all(), (spec["name"], mem, i1, i2)
        got.append((xy, inf))
    return got


# ---- random batches, checked against the engine's own variable-base calls ---------------------

def random_batch(spec, n, seed):
    """n scalars for mul_base on bases[3] and n pairs for mul_base2 on (bases[0], bases[2]) = (G, -G).
    A third of the scalars have a random bit length below the full width.  The first rows are there
    by construction.  Single batch: k = 0 and k = n (both the identity), then k = 1.  Pair batch:
    (5, 5), 5 G - 5 G = the identity; (n - 5, 5), where the second walk finds the accumulator -5 G equal
    to the entry 5 (-G) it adds (B1 = B2 as points: the law doubles); (7, 7 + 3 2^16), where the
    accumulator is the identity after the second walk's first window; then random pairs."""
    rng = random.Random("fixed-base-ed:%s:%d" % (spec["name"], seed))
    order = I(spec["n"])

    def draw():
        return rng.getrandbits(256) if rng.random() < 0.65 else rng.getrandbits(rng.randrange(1, 256)) | 1

    ks = [0, order, 1] + [draw() for _ in range(n - 3)]
    k1 = [5, order - 5, 7] + [draw() for _ in range(n - 3)]
    k2 = [5, 5, 7 + (3 << 16)] + [draw() for _ in range(n - 3)]
    return {"k": rows(ks, B), "k1": rows(k1, B), "k2": rows(k2, B), "ints": (ks, k1, k2)}


def model_meets_conditions(spec, bt):
    """the first four rows hold an identity answer in both batches, and the pair batch a row whose two
    products are the same point -- asserted on the model, before any device runs"""
    m, pts = model_of(spec), bases_of(spec)
    ks, k1, k2 = bt["ints"]
    one = [m.mul(k, pts[3]) for k in ks[:4]]
    two = [(m.mul(a, pts[0]), m.mul(b, pts[2])) for a, b in zip(k1[:4], k2[:4])]
    same = [u == v and u != Model.ID for u, v in two]
    return Model.ID in one and any(m.add(u, v) == Model.ID for u, v in two) and any(same) and one[2] == pts[3]


def tiled(P, n):
    return np.tile(np.frombuffer(xy_bytes(P, B), np.uint8), (n, 1))


def variable_base_answers(ctx, cid, spec, bt):
    """the whole batch through ellgpu_mul_var (bases[3] tiled) and ellgpu_mul_add2 ((G, -G) tiled),
    host memory: what mul_base and mul_base2 must give byte for byte.  Computed once per curve."""
    pts, n = bases_of(spec), bt["k"].shape[0]
    xy, inf = ctx.mul_var(cid, bt["k"], tiled(pts[3], n))
    xy2, inf2 = ctx.mul_add2(cid, bt["k1"], tiled(pts[0], n), bt["k2"], tiled(pts[2], n))
    for a in (xy, inf, xy2, inf2):
        a.setflags(write=False)
    return {"xy": xy, "inf": inf, "xy2": xy2, "inf2": inf2}


def check_batch(ctx, spec, bt, want, n, hs, mem):
    """the first n items: mul_base on hs[3] against mul_var, mul_base2 on (hs[0], hs[2]) against mul_add2"""
    xy, inf = run_mul(ctx, hs[3], bt["k"][:n], B, mem)
    assert (inf == want["inf"][:n]).all() and (xy == want["xy"][:n]).all(), (spec["name"], n, mem)
    xy2, inf2 = run_mul2(ctx, hs[0], hs[2], bt["k1"][:n], bt["k2"][:n], B, mem)
    assert (inf2 == want["inf2"][:n]).all() and (xy2 == want["xy2"][:n]).all(), (spec["name"], n, mem)
    return xy, inf, xy2, inf2
