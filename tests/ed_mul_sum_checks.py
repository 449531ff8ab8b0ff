"""Sums of many k * P terms on Edwards curves (ellgpu_ed_mul_sum): the reference's recorded answers
(tests/golden/ed_mul_sum.json, tools/gen_golden_ed_mul_sum.js), the Python-integer Edwards model of
tests/fixed_base_ed_checks.py and the helpers the hostsim and device tests share.

The model is the affine law a x^2 + y^2 = 1 + d x^2 y^2 (complete on every curve of the fixture):
every coordinate reduced mod p; status 2 and zeroed bytes where a term's point is not on the curve;
else the products k * P, the scalar as it stands, added in order.  The identity is (0, 1) with
out_inf = 1 on ed25519 and out_inf = 0 on a user-defined id (fixed_base_ed_checks.answer): what the
curve's ellgpu_mul_add2 writes.  check_model_pinned holds the model to every recorded digest of the
reference -- its own points.map(mul).reduce(add) -- before anything relies on it.

Batches of any shape (n, m) draw their terms from ONE pool of terms per curve whose products the
model computes once (term_pool): a batch's expected bytes then cost one affine addition per term.

Memory kinds as in tests/mul_sum_checks.py: "host", "dev_np" (ELLGPU_MEM_DEVICE on the hostsim build,
where device memory is host memory) and "dev_torch" (device tensors, the current stream)."""
import json
import os
import random

import numpy as np

import fixed_base_ed_checks as FBE
from fixed_base_ed_checks import I, rows, xy_bytes, digest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ed_mul_sum.json")
FILL = 0xA5
NAMES = FBE.NAMES
B = 32
TOP = (1 << 256) - 1
OPTIONAL = ("ellgpu_probe_valu", "ellgpu_ctx_set_timing", "ellgpu_ctx_get_timing", "ellgpu_debug_field_op")
POOL = 256                      # terms in a curve's pool
MS = (1, 2, 3, 4, 5, 7, 8, 16, 33)
_cache = {}


def curves():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
    return _cache["golden"]


def spec_of(name):
    return next(c for c in curves() if c["name"] == name)


def curve_id(ctx, name):
    """the preset's name, or the id of the user-defined Edwards curve (a domain where the fixture says so)"""
    return FBE.curve_id(ctx, spec_of(name))


# ---- the model ------------------------------------------------------------------------------

class Curve:
    def __init__(self, spec):
        self.spec, self.name = spec, spec["name"]
        self.m = FBE.model_of(spec)
        self.p, self.n = self.m.p, I(spec["n"])
        self.pts = [(I(x), I(y)) for x, y in spec["pts"]]

    def point(self, P):
        """the point with its coordinates reduced, or None where that is no curve point"""
        P = (P[0] % self.p, P[1] % self.p)
        return P if self.m.on_curve(P) else None

    def total(self, products):
        """products: affine points, or "off" for a term that is not on the curve -> (point, status)"""
        if any(isinstance(R, str) for R in products):
            return None, 2
        S = FBE.Model.ID
        for R in products:
            S = self.m.add(S, R)
        return S, 0

    def sum_of(self, terms):
        """terms: [(k, (x, y))], the slow way: Model.mul per term"""
        prods = []
        for k, P in terms:
            Q = self.point(P)
            prods.append("off" if Q is None else self.m.mul(k, Q))
        return self.total(prods)

    def products(self, terms):
        """the same products over the doublings 2^i P of every distinct point, shared by its terms
        (held to `sum_of` by check_model_pinned)"""
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
            dbl = [Q]
            for _ in range(max(terms[i][0] for i in idx).bit_length()):
                dbl.append(self.m.add(dbl[-1], dbl[-1]))
            for i in idx:
                R, k, b = FBE.Model.ID, terms[i][0], 0
                while k:
                    if k & 1:
                        R = self.m.add(R, dbl[b])
                    k >>= 1
                    b += 1
                out[i] = R
        return out

    def answer(self, S, st):
        """(point, status) -> (x || y row, out_inf) as the engine writes it on this curve"""
        if st:
            return np.zeros(2 * B, np.uint8), st
        return FBE.answer(self.spec, S)


def curve_of(name):
    key = ("curve", name)
    if key not in _cache:
        _cache[key] = Curve(spec_of(name))
    return _cache[key]


def row_terms(C, row):
    return [(I(k), C.pts[pi]) for k, pi in row[1]]


def check_fixture_shape(spec):
    """the rows the generator promises are there"""
    C = curve_of(spec["name"])
    assert spec["B"] == B and spec["kind"] == FBE.spec_of(spec["name"])["kind"]
    for f in ("p", "a", "d", "n", "g"):
        assert spec[f] == FBE.spec_of(spec["name"])[f], (spec["name"], f)
    tags = [r[0] for r in spec["rows"]]
    at = lambda t: spec["rows"][tags.index(t)]  # noqa: E731
    for m in MS:
        assert len(at("m%d" % m)[1]) == m
    for t in ["edge%d" % i for i in range(6)] + ["zeros", "twice_pair", "twice_fold", "cancel_pair", "cancel_fold",
                                                  "total_id", "identity_term", "wide"]:
        assert t in tags, (spec["name"], t)
    assert ("torsion" in tags) == (spec["name"] in ("ed25519", "ed25519_by_hand"))
    for i, k in enumerate((0, 1, C.n - 1, C.n, C.n + 1, TOP)):
        assert [I(t[0]) for t in at("edge%d" % i)[1]] == [k] * 3
    ident = digest(*C.answer(FBE.Model.ID, 0))
    assert ident == digest(np.frombuffer(xy_bytes((0, 1), B), np.uint8), 1 if spec["kind"] == "preset" else 0)
    for t in ("zeros", "total_id", "cancel_pair_alone", "edge0"):
        assert at(t)[2] == ident, (spec["name"], t)
    assert len(at("total_id")[1]) == 7
    assert any(C.pts[pi] == (0, 1) for _, pi in at("identity_term")[1])
    if "torsion" in tags:
        order = lambda P: next(o for o in (1, 2, 4, 8, 0) if o == 0 or C.m.mul(o, P) == FBE.Model.ID)  # noqa: E731
        on8 = [I(k) % 8 for k, pi in at("torsion")[1] if order(C.pts[pi]) == 8]
        assert sorted(on8) == [1, 2, 3, 4, 5, 6, 7]
        assert any(C.pts[pi] == (0, C.p - 1) for _, pi in at("torsion")[1])
    assert all(C.pts[pi][0] >= C.p or C.pts[pi][1] >= C.p for _, pi in at("wide")[1][:-1])
    assert [r[0] for r in spec["off"]][:3] == ["first", "last", "lone"]
    for tag, terms in spec["off"]:
        on = [C.point(C.pts[pi]) is not None for _, pi in terms]
        assert on.count(False) == 1, (spec["name"], tag)
    offs = {r[0]: [C.point(C.pts[pi]) is None for _, pi in r[1]] for r in spec["off"]}
    assert offs["first"][0] and offs["last"][-1] and offs["lone"][-1] and len(offs["lone"]) % 2 == 1


def check_model_pinned(spec):
    C = curve_of(spec["name"])
    for row in spec["rows"]:
        terms = row_terms(C, row)
        assert digest(*C.answer(*C.total(C.products(terms)))) == row[2], (spec["name"], row[0])
    for row in spec["rows"][:3] + spec["rows"][-2:]:        # the shared doublings give the plain products
        terms = row_terms(C, row)
        assert C.sum_of(terms) == C.total(C.products(terms)), (spec["name"], row[0])
    for row in spec["off"]:
        assert C.total(C.products(row_terms(C, row)))[1] == 2


# ---- batches ----------------------------------------------------------------------------------

class Batch:
    """n sums of m terms: k (n, m, 32), xy (n, m, 64) and the expected xy (n, 64) / inf (n,)"""

    def __init__(self, k, xy, want_xy, want_inf, tags=None):
        self.k, self.xy, self.want_xy, self.want_inf, self.tags = k, xy, want_xy, want_inf, tags
        self.n, self.m = k.shape[0], k.shape[1]


def _term_arrays(terms):
    k = rows([t[0] for t in terms], B)
    xy = np.stack([np.frombuffer(xy_bytes(t[1], B), np.uint8) for t in terms])
    return k, xy


def _batch_of(C, sums, answers, tags=None):
    m = len(sums[0])
    ks, xys = zip(*[_term_arrays(s) for s in sums])
    a = [C.answer(S, st) for S, st in answers]
    return Batch(np.stack(ks).reshape(len(sums), m, B), np.stack(xys).reshape(len(sums), m, 2 * B),
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
            rws = list(by_m[m])
            if shuffled:
                random.Random(m).shuffle(rws)
            sums = [row_terms(C, r) for r in rws]
            answers = [C.total(C.products(s)) for s in sums]
            bt = _batch_of(C, sums, answers, [r[0] for r in rws])
            for j, r in enumerate(rws):
                assert (r[2] is None and bt.want_inf[j] == 2) or digest(bt.want_xy[j], bt.want_inf[j]) == r[2]
            out.append(bt)
        _cache[key] = out
    return _cache[key]


def term_pool(name):
    """POOL terms (k, P) with their products, computed once per curve.  Points: the first eight of the
    fixture's pool (four points and their negatives).  Scalars: random ones, each also on the
    negative of its point now and then (so that partial sums cancel), and 0, 1, 2, n - 1, n, n + 1,
    2^256 - 1, small and short ones."""
    key = ("pool", name)
    if key not in _cache:
        C = curve_of(name)
        rnd = random.Random("ed-mul-sum-pool:" + name)
        special = [0, 1, 2, C.n - 1, C.n, C.n + 1, TOP, 5, 0xFFFF, 1 << 64, (1 << 128) - 1, TOP - 1]
        terms = []
        while len(terms) < POOL:
            j = len(terms)
            k = special[j // 2 % len(special)] if j % 8 < 2 else rnd.randrange(TOP + 1)
            pi = rnd.randrange(8)
            terms.append((k, C.pts[pi]))
            if j % 5 == 0:
                terms.append((k, C.pts[pi ^ 1]))
        terms = terms[:POOL]
        _cache[key] = (terms, C.products(terms), _term_arrays(terms))
    return _cache[key]


def pool_batch(name, n, m, seed=1):
    """n sums of m terms drawn from the pool; every eleventh sum repeats its first pair so that equal
    partial sums meet"""
    key = ("batch", name, n, m, seed)
    if key not in _cache:
        C = curve_of(name)
        terms, prods, (pk, pxy) = term_pool(name)
        rnd = random.Random("ed-mul-sum-batch:%s:%d:%d:%d" % (name, n, m, seed))
        idx = np.array([[rnd.randrange(POOL) for _ in range(m)] for _ in range(n)])
        for j in range(0, n, 11):
            if m >= 4:
                idx[j, 2:4] = idx[j, 0:2]                       # two equal pairs: the fold adds a partial to itself
        a = [C.answer(*C.total([prods[i] for i in row])) for row in idx]
        _cache[key] = Batch(np.ascontiguousarray(pk[idx]), np.ascontiguousarray(pxy[idx]),
                            np.stack([x for x, _ in a]), np.array([f for _, f in a], np.uint8))
    return _cache[key]


def with_off_curve(name, bt, places):
    """a copy of the batch in which the term (j, i) of every place has a point that is not on the
    curve: those sums expect status 2 and zeroed bytes, every other sum what it expected before"""
    C = curve_of(name)
    off = np.frombuffer(xy_bytes(next(P for P in C.pts if C.point(P) is None), B), np.uint8)
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
    """ellgpu_ed_mul_sum on a Batch -> (xy, inf), written into buffers that were filled with 0xA5"""
    n = bt.n
    if mem == "dev_torch":
        import torch
        k, xy = torch.from_numpy(bt.k).cuda(), torch.from_numpy(bt.xy).cuda()
        out = (torch.full((n, 2 * B), FILL, dtype=torch.uint8, device="cuda"),
               torch.full((n,), FILL, dtype=torch.uint8, device="cuda"))
        got = ctx.ed_mul_sum(curve, k, xy, out=out)
        torch.cuda.synchronize()
        assert got[0] is out[0] and got[1] is out[1]
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    oxy, inf = np.full((n, 2 * B), FILL, np.uint8), np.full(n, FILL, np.uint8)
    if mem == "host":
        got = ctx.ed_mul_sum(curve, bt.k, bt.xy, out=(oxy, inf))
        assert got[0] is oxy and got[1] is inf
    else:
        P = lambda a: a.ctypes.data  # noqa: E731
        _raw(ctx, ctx._lib.ellgpu_ed_mul_sum(ctx._ctx, ctx._cid(curve), n, bt.m, P(bt.k), P(bt.xy), P(oxy), P(inf), 1, None))
    return oxy, inf


def check(ctx, curve, bt, mem="host"):
    """the engine's bytes are the expected ones; -> them"""
    oxy, inf = run(ctx, curve, bt, mem)
    bad = np.nonzero((inf != bt.want_inf) | (oxy != bt.want_xy).any(axis=1))[0]
    assert bad.size == 0, (curve, mem, bt.n, bt.m, [(int(i), bt.tags[i] if bt.tags else None, int(inf[i]),
                                                     int(bt.want_inf[i])) for i in bad[:8]])
    return oxy, inf
