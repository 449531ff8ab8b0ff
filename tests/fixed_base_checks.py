"""Fixed-base tables of caller-chosen points (ellgpu_base_define, ellgpu_mul_base, ellgpu_mul_base2):
the reference's recorded answers (tests/golden/fixed_base.json, tools/gen_golden_fixed_base.js), a
Python-integer model and the helpers the hostsim, device and N-API tests share.

The model is plain affine double-and-add over Python integers: for k * P and k1 * B1 + k2 * B2 the
group law is the whole contract (scalars are used as they stand, the answer at O is a zeroed point
beside inf = 1).  The fixture records a digest per answer -- the first 8 bytes of SHA-256(inf || x ||
y) -- and test_model_is_pinned_to_the_fixture holds the model to every one of them before anything
else relies on it.

Every call is run with one of three memory kinds: "host" (ELLGPU_MEM_HOST), "dev_np"
(ELLGPU_MEM_DEVICE on the hostsim build, where device memory is host memory) and "dev_torch"
(ELLGPU_MEM_DEVICE on device tensors, the current stream)."""
import hashlib
import json
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fixed_base.json")
FILL = 0xA5
PRESETS = ["secp256k1", "p192", "p224", "p256", "p384", "p521"]
SIGNED = ("secp256k1", "p256")                 # the curves with the signed comb (Work::COMB_SIGNED)
NAMES = PRESETS + ["brainpoolP256r1", "secp192k1", "cof_p10007"]
_cache = {}


def I(s):
    return int(s, 16)


def curves():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
    return _cache["golden"]


def spec_of(name):
    return next(c for c in curves() if c["name"] == name)


def rows(vals, B):
    return np.stack([np.frombuffer(int(v).to_bytes(B, "big"), np.uint8) for v in vals]) if len(vals) else np.zeros((0, B), np.uint8)


def xy_bytes(pt, B):
    return int(pt[0]).to_bytes(B, "big") + int(pt[1]).to_bytes(B, "big")


# ---- the model ------------------------------------------------------------------------------

class Model:
    """y^2 = x^3 + a x + b over p; points are (x, y) tuples, None is O"""

    def __init__(self, p, a, b):
        self.p, self.a, self.b = p, a % p, b % p

    def on_curve(self, P):
        return (P[1] * P[1] - (P[0] * P[0] * P[0] + self.a * P[0] + self.b)) % self.p == 0

    def add(self, P, Q):
        p = self.p
        if P is None:
            return Q
        if Q is None:
            return P
        if P[0] == Q[0]:
            if (P[1] + Q[1]) % p == 0:
                return None
            lam = (3 * P[0] * P[0] + self.a) * pow(2 * P[1], -1, p) % p
        else:
            lam = (Q[1] - P[1]) * pow(Q[0] - P[0], -1, p) % p
        x = (lam * lam - P[0] - Q[0]) % p
        return x, (lam * (P[0] - x) - P[1]) % p

    def neg(self, P):
        return None if P is None else (P[0], -P[1] % self.p)

    def mul(self, k, P):
        R = None
        for bit in bin(k)[2:] if k else "":
            R = self.add(R, R)
            if bit == "1":
                R = self.add(R, P)
        return R

    def mul2(self, k1, P1, k2, P2):
        return self.add(self.mul(k1, P1), self.mul(k2, P2))

    # the same group law for thousands of items on one base: Jacobian coordinates (one inversion
    # per answer, not one per step) over a table of the base's multiples d 16^w P, which the plain
    # `mul` above builds.  test_model_is_pinned_to_the_fixture holds mul_many to mul.
    def _jadd(self, R, Q):
        """Jacobian R + affine Q (neither O, R != +-Q is NOT assumed)"""
        p = self.p
        X, Y, Z = R
        zz = Z * Z % p
        h = (Q[0] * zz - X) % p
        r = (Q[1] * zz * Z - Y) % p
        if h == 0:
            if r:
                return None
            A = self.add(Q, Q)
            return None if A is None else (A[0], A[1], 1)
        hh = h * h % p
        v = X * hh % p
        hhh = h * hh % p
        x3 = (r * r - hhh - 2 * v) % p
        return x3, (r * (v - x3) - Y * hhh) % p, Z * h % p

    def table(self, P, bits):
        key = ("tbl", P, bits)
        if key not in _cache:
            t, W = [], P
            for _ in range((bits + 3) // 4):
                row, D = [None], None
                for _d in range(15):
                    D = self.add(D, W)
                    row.append(D)
                t.append(row)
                W = self.add(self.add(W, W), self.add(W, W))
                W = self.add(self.add(W, W), self.add(W, W))
            _cache[key] = t
        return _cache[key]

    def mul_many(self, ks, P, bits, acc=None):
        """[k * P (+ acc[i])] as affine points; acc: affine points or None"""
        t, out, p = self.table(P, bits), [], self.p
        for i, k in enumerate(ks):
            A = acc[i] if acc else None
            R = None if A is None else (A[0], A[1], 1)
            w = 0
            while k:
                Q = t[w][k & 15]
                if Q is not None:
                    R = (Q[0], Q[1], 1) if R is None else self._jadd(R, Q)
                k >>= 4
                w += 1
            if R is None:
                out.append(None)
            else:
                zi = pow(R[2], -1, p)
                out.append((R[0] * zi * zi % p, R[1] * zi * zi * zi % p))
        return out


def model_of(spec):
    if "p" in spec:
        return Model(I(spec["p"]), I(spec["a"]), I(spec["b"]))
    from oracle import ec_oracle as O
    c = O.get_curve(spec["name"], precompute=False)
    return Model(c.p, c.a, c.b)


def bases_of(spec):
    return [(I(x), I(y)) for x, y in spec["bases"]]


def answer(P, B):
    """a model point -> (x || y row, inf) as the engine writes it"""
    if P is None:
        return np.zeros(2 * B, np.uint8), 1
    return np.frombuffer(xy_bytes(P, B), np.uint8), 0


def digest(xy_row, inf):
    return hashlib.sha256(bytes([int(inf)]) + xy_row.tobytes()).hexdigest()[:16]


def golden_answers(spec):
    """the model's answers for every recorded case, computed once per curve:
    -> (mul: per base (xy (n, 2B), inf (n,)), pairs: (xy, inf))"""
    key = ("answers", spec["name"])
    if key not in _cache:
        m, B, pts = model_of(spec), spec["B"], bases_of(spec)
        ks = [I(k) for k in spec["k"]]
        mul = []
        for P in pts:
            a = [answer(m.mul(k, P), B) for k in ks]
            mul.append((np.stack([x for x, _ in a]), np.array([f for _, f in a], np.uint8)))
        a = [answer(m.mul2(I(k1), pts[i1], I(k2), pts[i2]), B) for i1, i2, k1, k2, _ in spec["pairs"]]
        _cache[key] = (mul, (np.stack([x for x, _ in a]), np.array([f for _, f in a], np.uint8)))
    return _cache[key]


def check_model_pinned(spec):
    mul, pairs = golden_answers(spec)
    m, pts, B = model_of(spec), bases_of(spec), spec["B"]
    ks = [I(k) for k in spec["k"]]
    fast = m.mul_many(ks, pts[3], 8 * B)
    assert all((answer(R, B)[0] == mul[3][0][j]).all() and answer(R, B)[1] == mul[3][1][j] for j, R in enumerate(fast))
    idx = [j for j, q in enumerate(spec["pairs"]) if (q[0], q[1]) == (0, 2)]
    fast = m.mul_many([I(spec["pairs"][j][3]) for j in idx], pts[2], 8 * B,
                      m.mul_many([I(spec["pairs"][j][2]) for j in idx], pts[0], 8 * B))
    assert all((answer(R, B)[0] == pairs[0][j]).all() and answer(R, B)[1] == pairs[1][j] for j, R in zip(idx, fast))
    for bi, (xy, inf) in enumerate(mul):
        assert [digest(xy[j], inf[j]) for j in range(len(inf))] == spec["mul"][bi], (spec["name"], bi)
    assert [digest(pairs[0][j], pairs[1][j]) for j in range(len(pairs[1]))] == [p[4] for p in spec["pairs"]], spec["name"]


# ---- the engine's side ----------------------------------------------------------------------

def curve_id(ctx, spec):
    """the preset's name, or the id of the user-defined curve (a domain where the fixture says so)"""
    if "p" not in spec:
        return spec["name"]
    p, a, b = I(spec["p"]), I(spec["a"]), I(spec["b"])
    if spec.get("domain"):
        return ctx.define_short_domain(p, a, b, I(spec["n"]), I(spec["g"][0]), I(spec["g"][1]))
    return ctx.define_short(p, a, b)


def widths_of(name):
    """the explicit table widths the CPU tests walk: 4 and 8 on the signed combs, 8 elsewhere"""
    return (4, 8) if name in SIGNED else (8,)


def _raw(ctx, rc):
    from elliptic_amd import _lib
    if rc != 0:
        raise _lib.EllgpuError(rc, ctx._lib.ellgpu_last_error().decode())


def _P(a):
    return a.ctypes.data if a is not None else None


def _torch_call(fn, ins, B):
    import torch
    di = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ins]
    n = ins[0].shape[0]
    xy = torch.full((n, 2 * B), FILL, dtype=torch.uint8, device="cuda")
    inf = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    fn(di, (xy, inf))
    torch.cuda.synchronize()
    return xy.cpu().numpy(), inf.cpu().numpy()


def run_mul(ctx, base, k, B, mem="host"):
    k = np.ascontiguousarray(k, np.uint8).reshape(-1, B)
    n = k.shape[0]
    if mem == "dev_torch":
        return _torch_call(lambda i, o: ctx.mul_base(base, i[0], out=o), [k], B)
    xy, inf = np.full((n, 2 * B), FILL, np.uint8), np.full(n, FILL, np.uint8)
    if mem == "host":
        ctx.mul_base(base, k, out=(xy, inf))
    else:
        _raw(ctx, ctx._lib.ellgpu_mul_base(ctx._ctx, base, n, _P(k), _P(xy), _P(inf), 1, None))
    return xy, inf


def run_mul2(ctx, b1, b2, k1, k2, B, mem="host"):
    k1 = np.ascontiguousarray(k1, np.uint8).reshape(-1, B)
    k2 = np.ascontiguousarray(k2, np.uint8).reshape(-1, B)
    n = k1.shape[0]
    if mem == "dev_torch":
        return _torch_call(lambda i, o: ctx.mul_base2(b1, b2, i[0], i[1], out=o), [k1, k2], B)
    xy, inf = np.full((n, 2 * B), FILL, np.uint8), np.full(n, FILL, np.uint8)
    if mem == "host":
        ctx.mul_base2(b1, b2, k1, k2, out=(xy, inf))
    else:
        _raw(ctx, ctx._lib.ellgpu_mul_base2(ctx._ctx, b1, b2, n, _P(k1), _P(k2), _P(xy), _P(inf), 1, None))
    return xy, inf


def define_bases(ctx, spec, width, cid=None):
    cid = curve_id(ctx, spec) if cid is None else cid
    B = spec["B"]
    return cid, [ctx.define_base(cid, xy_bytes(P, B), width) for P in bases_of(spec)]


def check_golden(ctx, spec, width, mem, cid=None):
    """every recorded case at one table width through one memory kind; -> the bytes the engine wrote"""
    B = spec["B"]
    cid, hs = define_bases(ctx, spec, width, cid)
    mul, pairs = golden_answers(spec)
    k = rows([I(v) for v in spec["k"]], B)
    got = []
    try:
        for bi, h in enumerate(hs):
            assert ctx.base_info(h)[1] == width
            xy, inf = run_mul(ctx, h, k, B, mem)
            assert (inf == mul[bi][1]).all() and (xy == mul[bi][0]).all(), (spec["name"], width, mem, bi)
            got.append((xy, inf))
        # the pairs, one call per (base1, base2) that occurs
        for i1, i2 in sorted({(p[0], p[1]) for p in spec["pairs"]}):
            idx = [j for j, p in enumerate(spec["pairs"]) if (p[0], p[1]) == (i1, i2)]
            k1 = rows([I(spec["pairs"][j][2]) for j in idx], B)
            k2 = rows([I(spec["pairs"][j][3]) for j in idx], B)
            xy, inf = run_mul2(ctx, hs[i1], hs[i2], k1, k2, B, mem)
            assert (inf == pairs[1][idx]).all() and (xy == pairs[0][idx]).all(), (spec["name"], width, mem, i1, i2)
            got.append((xy, inf))
    finally:
        for h in hs:
            ctx.release_base(h)
    return got


# ---- random batches -------------------------------------------------------------------------

def random_batch(spec, n, seed):
    """n items for mul_base on bases[3] and for mul_base2 on (bases[0], bases[2]) = (G, -G), with the
    model's answers.  A third of the scalars have a random bit length below the full width.  The
    first rows are there by construction.  Single batch: k = 0 and k = n (both O), then k = 1.  Pair
    batch: (5, 5), 5 G - 5 G = O; (n - 5, 5), where the second walk finds the accumulator -5 G equal to
    the entry 5 (-G) it adds (the doubling branch); (7, 7 + 3 2^16), where the accumulator is O after
    the second walk's first window and the additions start again from it; then random pairs."""
    rng = random.Random("fixed-base:%s:%d" % (spec["name"], seed))
    m, B, pts = model_of(spec), spec["B"], bases_of(spec)
    order = I(spec["n"])

    def draw():
        return rng.getrandbits(8 * B) if rng.random() < 0.65 else rng.getrandbits(rng.randrange(1, 8 * B)) | 1

    ks = [0, order, 1] + [draw() for _ in range(n - 3)]
    one = [answer(R, B) for R in m.mul_many(ks, pts[3], 8 * B)]
    k1 = [5, order - 5, 7] + [draw() for _ in range(n - 3)]
    k2 = [5, 5, 7 + (3 << 16)] + [draw() for _ in range(n - 3)]
    two = [answer(R, B) for R in m.mul_many(k2, pts[2], 8 * B, m.mul_many(k1, pts[0], 8 * B))]
    return {"k": rows(ks, B), "xy": np.stack([x for x, _ in one]), "inf": np.array([f for _, f in one], np.uint8),
            "k1": rows(k1, B), "k2": rows(k2, B), "xy2": np.stack([x for x, _ in two]),
            "inf2": np.array([f for _, f in two], np.uint8), "ints": (ks, k1, k2)}


def model_meets_conditions(spec, bt):
    """the first four rows hold an infinity in both batches, and the pair batch a row whose two
    products are the same point (the doubling branch) -- asserted on the model, before any device runs"""
    m, pts = model_of(spec), bases_of(spec)
    ks, k1, k2 = bt["ints"]
    same = [m.mul(a, pts[0]) == m.mul(b, pts[2]) and m.mul(a, pts[0]) is not None for a, b in zip(k1[:4], k2[:4])]
    return bt["inf"][:4].any() and bt["inf2"][:4].any() and any(same) and not bt["inf"][3:].all()


def check_batch(ctx, spec, bt, n, hs, mem):
    """the first n items of a batch: mul_base on hs[3], mul_base2 on (hs[0], hs[2])"""
    B = spec["B"]
    xy, inf = run_mul(ctx, hs[3], bt["k"][:n], B, mem)
    assert (inf == bt["inf"][:n]).all() and (xy == bt["xy"][:n]).all(), (spec["name"], n, mem)
    xy2, inf2 = run_mul2(ctx, hs[0], hs[2], bt["k1"][:n], bt["k2"][:n], B, mem)
    assert (inf2 == bt["inf2"][:n]).all() and (xy2 == bt["xy2"][:n]).all(), (spec["name"], n, mem)
    return xy, inf, xy2, inf2
