"""Sums of many k * P terms (ellgpu_mul_sum): the reference's recorded answers
(tests/golden/mul_sum.json, tools/gen_golden_mul_sum.js), a Python-integer model and the helpers the
hostsim and device tests share.

The model is the definition over Python integers (the affine group law of
tests/fixed_base_checks.py): every coordinate reduced mod p; status 2 where a term's point is not on
the curve; else the products k * P, the scalar as it stands, added in order; status 1 with a zeroed
result where the sum is O.  check_model_pinned holds it to every recorded digest of the reference --
its own points.map(mul).reduce(add) -- before anything relies on it.

Batches of any shape (n, m) draw their terms from ONE pool of terms per curve whose products the
model computes once (term_pool): a batch's expected bytes then cost one affine addition per term.

Memory kinds as in tests/verify_base_checks.py: "host", "dev_np" (ELLGPU_MEM_DEVICE on the hostsim
build, where device memory is host memory) and "dev_torch" (device tensors, the current stream)."""
import json
import os
import random

import numpy as np

import fixed_base_checks as FB

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "mul_sum.json")
FILL = 0xA5
PRESETS = FB.PRESETS
USER = ["brainpoolP256r1", "secp192k1"]
NAMES = PRESETS + USER
I = FB.I
OPTIONAL = ("ellgpu_probe_valu", "ellgpu_ctx_set_timing", "ellgpu_ctx_get_timing", "ellgpu_debug_field_op")
POOL = 256                      # terms in a curve's pool
_cache = {}


def curves():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
    return _cache["golden"]


def spec_of(name):
    return next(c for c in curves() if c["name"] == name)


def curve_id(ctx, name):
    """the preset's name, or the id of the user-defined curve (a domain where the fixture says so)"""
    return FB.curve_id(ctx, spec_of(name))


# ---- the model ------------------------------------------------------------------------------

class Curve:
    def __init__(self, spec):
        self.name, self.B = spec["name"], spec["B"]
        self.m = FB.model_of(spec)
        self.p, self.n = self.m.p, I(spec["n"])
        self.pts = [(I(x), I(y)) for x, y in spec["pts"]]

    def point(self, P):
        """the point with its coordinates reduced, or None where that is no curve point"""
        P = (P[0] % self.p, P[1] % self.p)
        return P if self.m.on_curve(P) else None

    def total(self, products):
        """products: affine points, O as None, or "off" for a term that is not on the curve -> (point, status)"""
        if any(isinstance(R, str) for R in products):
            return None, 2
        S = None
        for R in products:
            S = self.m.add(S, R)
        return S, 1 if S is None else 0

    def sum_of(self, terms):
        """terms: [(k, (x, y))], the slow way: Model.mul per term"""
        prods = []
        for k, P in terms:
            Q = self.point(P)
            prods.append("off" if Q is None else self.m.mul(k, Q))
        return self.total(prods)

    def products(self, terms):
        """the same products through Model.mul_many, grouped by point (held to `sum_of` by check_model_pinned)"""
        out = [None] * len(terms)
        by_pt = {}
        for i, (k, P) in enumerate(terms):
            by_pt.setdefault(P, []).append(i)
        for P, idx in by_pt.items():
            Q = self.point(P)
            if Q is None:
                for i in idx:
                    out[i] = "off"
                continue
            for i, R in zip(idx, self.m.mul_many([terms[i][0] for i in idx], Q, 8 * self.B)):
                out[i] = R
        return out


def curve_of(name):
    key = ("curve", name)
    if key not in _cache:
        _cache[key] = Curve(spec_of(name))
    return _cache[key]


def answer_bytes(C, S, st):
    """(point, status) -> (x || y row, status) as the engine writes it"""
    if st:
        return np.zeros(2 * C.B, np.uint8), st
    return np.frombuffer(FB.xy_bytes(S, C.B), np.uint8), 0


def row_terms(C, row):
    return [(I(k), C.pts[pi]) for k, pi in row[1]]


def check_fixture_shape(spec):
    """the rows the generator promises are there"""
    tags = [r[0] for r in spec["rows"]]
    for m in (1, 2, 3, 4, 5, 7, 8, 16, 33):
        assert len(spec["rows"][tags.index("m%d" % m)][1]) == m
    for t in ["edge%d" % i for i in range(6)] + ["zeros", "twice_pair", "twice_fold", "cancel_pair", "cancel_fold",
                                                  "total_o"]:
        assert t in tags, (spec["name"], t)
    assert ("wide" in tags) == (spec["name"] in ("p521", "brainpoolP256r1", "secp192k1"))
    C = curve_of(spec["name"])
    n, top = C.n, (1 << (8 * C.B)) - 1
    for i, k in enumerate((0, 1, n - 1, n, n + 1, top)):
        assert [I(t[0]) for t in spec["rows"][tags.index("edge%d" % i)][1]] == [k] * 3
    o = FB.digest(np.zeros(2 * C.B, np.uint8), 1)
    for t in ("zeros", "total_o", "cancel_pair_alone", "edge0"):
        assert spec["rows"][tags.index(t)][2] == o, (spec["name"], t)
    assert [r[0] for r in spec["off"]][:3] == ["first", "last", "lone"]
    for tag, terms in spec["off"]:
        on = [C.point(C.pts[pi]) is not None for _, pi in terms]
        assert on.count(False) == 1, (spec["name"], tag)
    offs = {r[0]: [C.point(C.pts[pi]) is None for _, pi in r[1]] for r in spec["off"]}
    assert offs["first"][0] and offs["last"][-1] and offs["lone"][-1] and len(offs["lone"]) % 2 == 1
    if "wide" in tags:
        assert any(C.pts[pi][0] >= C.p or C.pts[pi][1] >= C.p for _, pi in spec["rows"][tags.index("wide")][1])


def check_model_pinned(spec):
    C = curve_of(spec["name"])
    for row in spec["rows"]:
        terms = row_terms(C, row)
        S, st = C.total(C.products(terms))
        xy, inf = answer_bytes(C, S, st)
        assert FB.digest(xy, inf) == row[2], (spec["name"], row[0])
    for row in spec["rows"][:3] + spec["rows"][-2:]:        # the fast products are the plain ones
        terms = row_terms(C, row)
        assert C.sum_of(terms) == C.total(C.products(terms)), (spec["name"], row[0])
    for row in spec["off"]:
        assert C.total(C.products(row_terms(C, row)))[1] == 2


# ---- batches ----------------------------------------------------------------------------------

class Batch:
    """n sums of m terms: k (n, m, B), xy (n, m, 2B) and the expected xy (n, 2B) / inf (n,)"""

    def __init__(self, k, xy, want_xy, want_inf, tags=None):
        self.k, self.xy, self.want_xy, self.want_inf, self.tags = k, xy, want_xy, want_inf, tags
        self.n, self.m = k.shape[0], k.shape[1]

    def take(self, idx):
        idx = np.asarray(idx)
        return Batch(np.ascontiguousarray(self.k[idx]), np.ascontiguousarray(self.xy[idx]), self.want_xy[idx],
                     self.want_inf[idx], [self.tags[i] for i in idx] if self.tags else None)

    def first(self, n):
        return self.take(np.arange(n))


def _term_arrays(C, terms):
    k = FB.rows([t[0] for t in terms], C.B)
    xy = np.stack([np.frombuffer(FB.xy_bytes(t[1], C.B), np.uint8) for t in terms])
    return k, xy


def _batch_of(C, sums, answers, tags=None):
    m = len(sums[0])
    ks, xys = zip(*[_term_arrays(C, s) for s in sums])
    a = [answer_bytes(C, S, st) for S, st in answers]
    return Batch(np.stack(ks).reshape(len(sums), m, C.B), np.stack(xys).reshape(len(sums), m, 2 * C.B),
                 np.stack([x for x, _ in a]), np.array([f for _, f in a], np.uint8), tags)


def fixture_batches(name, shuffled=False):
    """the recorded rows, and the off-curve rows (expected: status 2), as one batch per m, in fixture
    order or shuffled"""
    key = ("fixture", name, shuffled)
    if key not in _cache:
        spec, C = spec_of(name), curve_of(name)
        by_m = {}
        for row in spec["rows"] + [r + [None] for r in spec["off"]]:
            by_m.setdefault(len(row[1]), []).append(row)
        out = []
        for m in sorted(by_m):
            rws = by_m[m]
            if shuffled:
                random.Random(m).shuffle(rws)
            sums = [row_terms(C, r) for r in rws]
            answers = [C.total(C.products(s)) for s in sums]
            bt = _batch_of(C, sums, answers, [r[0] for r in rws])
            for j, r in enumerate(rws):
                assert (r[2] is None and bt.want_inf[j] == 2) or FB.digest(bt.want_xy[j], bt.want_inf[j]) == r[2]
            out.append(bt)
        _cache[key] = out
    return _cache[key]


def term_pool(name):
    """POOL terms (k, P) with their products, computed once per curve.  Points: the first eight of the
    fixture's pool (four points and their negatives).  Scalars: random ones, each also on the
    negative of its point now and then (so that partial sums cancel), and 0, 1, 2, n - 1, n, n + 1,
    2^(8B) - 1, small and short ones."""
    key = ("pool", name)
    if key not in _cache:
        C = curve_of(name)
        rnd = random.Random("mul-sum-pool:" + name)
        top = (1 << (8 * C.B)) - 1
        special = [0, 1, 2, C.n - 1, C.n, C.n + 1, top, 5, 0xFFFF, 1 << 64, (1 << (4 * C.B)) - 1, top - 1]
        terms = []
        while len(terms) < POOL:
            j = len(terms)
            k = special[j // 2 % len(special)] if j % 8 < 2 else rnd.randrange(top + 1)
            pi = rnd.randrange(8)
            terms.append((k, C.pts[pi]))
            if j % 5 == 0:
                terms.append((k, C.pts[pi ^ 1]))
        terms = terms[:POOL]
        _cache[key] = (terms, C.products(terms))
    return _cache[key]


def pool_batch(name, n, m, seed=1):
    """n sums of m terms drawn from the pool; every eleventh sum repeats its first term's pool
    neighbour so that equal and opposite partial sums meet"""
    key = ("batch", name, n, m, seed)
    if key not in _cache:
        C = curve_of(name)
        terms, prods = term_pool(name)
        rnd = random.Random("mul-sum-batch:%s:%d:%d:%d" % (name, n, m, seed))
        idx = np.array([[rnd.randrange(POOL) for _ in range(m)] for _ in range(n)])
        for j in range(0, n, 11):
            if m >= 4:
                idx[j, 2:4] = idx[j, 0:2]                       # two equal pairs: the fold's doubling branch
        pk, pxy = _term_arrays(C, terms)
        a = [answer_bytes(C, *C.total([prods[i] for i in row])) for row in idx]
        _cache[key] = Batch(np.ascontiguousarray(pk[idx]), np.ascontiguousarray(pxy[idx]),
                            np.stack([x for x, _ in a]), np.array([f for _, f in a], np.uint8))
    return _cache[key]


def with_off_curve(name, bt, places):
    """a copy of the batch in which the term (j, i) of every place has a point that is not on the
    curve: those sums expect status 2 and zeroed bytes, every other sum what it expected before"""
    C = curve_of(name)
    off = np.frombuffer(FB.xy_bytes(C.pts[[i for i, P in enumerate(C.pts) if C.point(P) is None][0]], C.B), np.uint8)
    xy, want_xy, want_inf = bt.xy.copy(), bt.want_xy.copy(), bt.want_inf.copy()
    for j, i in places:
        xy[j, i] = off
        want_xy[j] = 0
        want_inf[j] = 2
    return Batch(bt.k, xy, want_xy, want_inf)


# ---- the engine's side ----------------------------------------------------------------------

def _raw(ctx, rc):
    from elliptic_amd import _lib
    if rc != 0:
        raise _lib.EllgpuError(rc, ctx._lib.ellgpu_last_error().decode())


def run(ctx, curve, bt, mem="host"):
    """ellgpu_mul_sum on a Batch -> (xy, inf), written into buffers that were filled with 0xA5"""
    n, B2 = bt.n, bt.want_xy.shape[1]
    if mem == "dev_torch":
        import torch
        k, xy = torch.from_numpy(bt.k).cuda(), torch.from_numpy(bt.xy).cuda()
        out = (torch.full((n, B2), FILL, dtype=torch.uint8, device="cuda"),
               torch.full((n,), FILL, dtype=torch.uint8, device="cuda"))
        got = ctx.mul_sum(curve, k, xy, out=out)
        torch.cuda.synchronize()
        assert got[0] is out[0] and got[1] is out[1]
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    oxy, inf = np.full((n, B2), FILL, np.uint8), np.full(n, FILL, np.uint8)
    if mem == "host":
        got = ctx.mul_sum(curve, bt.k, bt.xy, out=(oxy, inf))
        assert got[0] is oxy and got[1] is inf
    else:
        P = lambda a: a.ctypes.data  # noqa: E731
        _raw(ctx, ctx._lib.ellgpu_mul_sum(ctx._ctx, ctx._cid(curve), n, bt.m, P(bt.k), P(bt.xy), P(oxy), P(inf), 1, None))
    return oxy, inf


def check(ctx, curve, bt, mem="host"):
    """the engine's bytes are the expected ones; -> them"""
    oxy, inf = run(ctx, curve, bt, mem)
    bad = np.nonzero((inf != bt.want_inf) | (oxy != bt.want_xy).any(axis=1))[0]
    assert bad.size == 0, (curve, mem, bt.n, bt.m, [(int(i), bt.tags[i] if bt.tags else None, int(inf[i]),
                                                     int(bt.want_inf[i])) for i in bad[:8]])
    return oxy, inf
