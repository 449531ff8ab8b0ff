"""The key side of user-defined Edwards curves (ellgpu_custom_ed_decompress, _decode_points, _validate,
_derive, _derive_wire, _encode_points): lib/elliptic/curve/edwards.js, curve/base.js and ec/key.js
restated over Python integers, the reference's recorded answers (tests/golden/custom_ed.json,
tools/gen_golden_custom_ed.js) and the helpers the hostsim, device and N-API tests share.

The model is the reference's own shape: pointFromX / pointFromY divide with redInvm (0 for 0), take
Red#sqrt (which answers 'invalid point' on a non-residue where p = 3 mod 4 and throws 'Assertion
failed' where p = 1 mod 4) and fix the parity; decodePoint is base.js:270-293; KeyPair#validate tests
(0, 1), the curve equation and order * P in that order; KeyPair#derive is validate, mul, getX.  The
scalar multiplication is the ENGINE's ladder (edcustom.h: signed 4-bit windows over P .. 8P,
add-2008-bbjlp / dbl-2008-bbjlp in projective coordinates), so that the model also says where Z = 0
on a curve whose addition law is incomplete; on a complete curve it is the group's own answer, which
the recorded cases confirm against the reference.

Every call is run in one of three forms: "host" (host buffers), "dev_np" (the _dev entry point on
the hostsim build, where device memory is host memory) and "dev_torch" (the _dev entry point on
device tensors)."""
import json
import os
import random

import numpy as np

import custom_wire_checks as CW

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "custom_ed.json")
FILL = CW.FILL
TOP = 1 << 256
BIG = ["curve1174", "e222", "twisted_a4", "twisted_am1", "p224_d11"]
TOY = ["p13_d4", "p13_d2", "p17_d3", "p19_d4"]
MSG = {"Unknown point format": 1, "invalid point": 2, "Assertion failed": 3}
REASON = {None: 0, "Invalid public key": 1, "Public key is not a point": 2, "Public key * N != O": 3}
_cache = {}


def I(s):
    return int(s, 16)


def b32(v):
    return np.frombuffer(int(v).to_bytes(32, "big"), np.uint8)


def rows(vals, width=32):
    if not len(vals):
        return np.zeros((0, width), np.uint8)
    return np.stack([np.frombuffer(int(v).to_bytes(width, "big"), np.uint8) for v in vals])


def xy_rows(pts):
    return rows([(x << 256) | y for x, y in pts], 64)


def ints(arr):
    return [int.from_bytes(r.tobytes(), "big") for r in arr]


def curves():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
    return _cache["golden"]


def spec_of(name):
    return next(c for c in curves() if c["name"] == name)


def params(spec):
    return I(spec["p"]), I(spec["a"]), I(spec["d"])


def define(ctx, spec):
    return ctx.define_edwards(*params(spec))


# ---- edwards.js, base.js and key.js over the integers -----------------------------------------

class Model:
    def __init__(self, p, a, d):
        self.p, self.a, self.d = p, a % p, d % p
        self.pl = (p.bit_length() + 7) // 8
        self.no_root = 3 if p % 4 == 1 else 2            # 'Assertion failed' / 'invalid point'
        self.memo = {}

    def inv0(self, v):
        return pow(v, self.p - 2, self.p)                # redInvm: 0 for 0

    def sqrt(self, v):
        """a root of v, or None"""
        p = self.p
        v %= p
        if v == 0:
            return 0
        if pow(v, (p - 1) // 2, p) != 1:
            return None
        if p % 4 == 3:
            return pow(v, (p + 1) // 4, p)
        q, s = p - 1, 0
        while q % 2 == 0:
            q, s = q // 2, s + 1
        z = next(z for z in range(2, p) if pow(z, (p - 1) // 2, p) == p - 1)
        c, r, t, m = pow(z, q, p), pow(v, (q + 1) // 2, p), pow(v, q, p), s
        while t != 1:
            i, u = 0, t
            while u != 1:
                u, i = u * u % p, i + 1
            b = pow(c, 1 << (m - i - 1), p)
            r, c, t, m = r * b % p, b * b % p, t * b * b % p, i
        return r

    def from_x(self, v, odd):
        """pointFromX -> ((x, y), 0) or (None, status)"""
        p = self.p
        x = v % p
        y2 = (1 - self.a * x * x) * self.inv0(1 - self.d * x * x) % p
        y = self.sqrt(y2)
        if y is None:
            return None, self.no_root
        if (y & 1) != (1 if odd else 0):
            y = -y % p
        return (x, y), 0

    def from_y(self, v, odd):
        p = self.p
        y = v % p
        x2 = (y * y - 1) * self.inv0(self.d * y * y - self.a) % p
        if x2 == 0:
            return (None, 2) if odd else ((0, y), 0)
        x = self.sqrt(x2)
        if x is None:
            return None, self.no_root
        if (x & 1) != (1 if odd else 0):
            x = -x % p
        return (x, y), 0

    def decode(self, enc):
        """decodePoint of a bytes object -> ((x, y), 0) or (None, status)"""
        pl = self.pl
        tag = enc[0] if len(enc) else 0
        if tag in (4, 6, 7) and len(enc) == 1 + 2 * pl:
            if (tag == 6 and enc[-1] & 1) or (tag == 7 and not enc[-1] & 1):
                return None, 3
            return (int.from_bytes(enc[1:1 + pl], "big") % self.p, int.from_bytes(enc[1 + pl:], "big") % self.p), 0
        if tag in (2, 3) and len(enc) == 1 + pl:
            return self.from_x(int.from_bytes(enc[1:], "big"), tag == 3)
        return None, 1

    def on_curve(self, x, y):
        p = self.p
        x, y = x % p, y % p
        return (self.a * x * x + y * y - 1 - self.d * x * x * y * y) % p == 0

    # the engine's group law and ladder (edcustom.h)
    def add(self, P, Q):
        p = self.p
        (X1, Y1, Z1), (X2, Y2, Z2) = P, Q
        A = Z1 * Z2 % p
        B = A * A % p
        C = X1 * X2 % p
        D = Y1 * Y2 % p
        E = self.d * C * D % p
        F, G = B - E, B + E
        return (A * F * ((X1 + Y1) * (X2 + Y2) - C - D) % p, A * G * (D - self.a * C) % p, F * G % p)

    def dbl(self, P):
        p = self.p
        X, Y, Z = P
        B = (X + Y) ** 2 % p
        C, D = X * X % p, Y * Y % p
        E = self.a * C % p
        F = E + D
        J = F - 2 * Z * Z
        return ((B - C - D) * J % p, F * (E - D) % p, F * J % p)

    def mul(self, k, x, y):
        """EdcWork::mul_var -> (X, Y, Z)"""
        p = self.p
        key = (k, x % p, y % p)
        if key not in self.memo:
            self.memo[key] = self._mul(*key)
        return self.memo[key]

    def _mul(self, k, x, y):
        p = self.p
        P = (x, y, 1)
        tbl = [P]
        for j in range(2, 9):
            tbl.append(self.add(tbl[j - 2], P) if j & 1 else self.dbl(tbl[j // 2 - 1]))
        kp = k + int("8" * 64, 16)
        acc = (0, 1, 1)
        for w in range(64, -1, -1):
            if w != 64:
                for _ in range(4):
                    acc = self.dbl(acc)
            dg = ((kp >> (4 * w)) & 15) - (8 if w < 64 else 0)
            if dg:
                X, Y, Z = tbl[abs(dg) - 1]
                acc = self.add(acc, (-X % p if dg < 0 else X, Y, Z))
        return acc

    def validate(self, x, y, order=None):
        """KeyPair#validate -> status"""
        p = self.p
        x, y = x % p, y % p
        if x == 0 and y == 1:
            return 1
        if not self.on_curve(x, y):
            return 2
        if order is not None:
            X, Y, Z = self.mul(order, x, y)
            if X % p != 0 or (Y - Z) % p != 0:
                return 3
        return 0

    def derive(self, k, x, y):
        """KeyPair#derive -> (x, status)"""
        if not self.on_curve(x, y):
            return 0, 1
        X, _, Z = self.mul(k, x, y)
        if Z % self.p == 0:
            return 0, 2
        return X * self.inv0(Z) % self.p, 0

    def derive_wire(self, k, enc):
        """-> (x, status, err)"""
        pt, err = self.decode(enc)
        if err:
            return 0, 3, err
        return self.derive(k, *pt) + (0,)

    def encode(self, x, y, compact):
        x, y = x % self.p, y % self.p
        if compact:
            return bytes([2 + (y & 1)]) + x.to_bytes(self.pl, "big")
        return b"\x04" + x.to_bytes(self.pl, "big") + y.to_bytes(self.pl, "big")


def model_of(spec):
    return Model(*params(spec))


# ---- the three forms of the calls -----------------------------------------------------------

def _P(a):
    return a.ctypes.data if a is not None else None


def _filled(*shapes):
    return [np.full(s, FILL, np.uint8) for s in shapes]


def _order(order):
    return None if order is None else int(order).to_bytes(32, "big")


def run_decompress(ctx, cid, v, odd, from_y, form="host"):
    v = np.ascontiguousarray(v, np.uint8).reshape(-1, 32)
    odd = np.ascontiguousarray(odd, np.uint8)
    n = v.shape[0]
    xy, st = _filled((n, 64), (n,))
    if form == "host":
        ctx.custom_ed_decompress(cid, v, odd, from_y, out=(xy, st))
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_ed_decompress_dev(ctx._ctx, cid, n, _P(v), _P(odd), int(from_y), _P(xy), _P(st), None))
    else:
        xy, st = CW._torch_call(lambda i, o: ctx.custom_ed_decompress_dev(cid, i[0], i[1], from_y, o[0], o[1]), [v, odd], [xy, st])
    return xy, st


def run_decode(ctx, cid, enc, form="host"):
    enc = np.ascontiguousarray(enc, np.uint8)
    n, enc_len = enc.shape
    xy, st = _filled((n, 64), (n,))
    if form == "host":
        ctx.custom_ed_decode_points(cid, enc, out=(xy, st))
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_ed_decode_points_dev(ctx._ctx, cid, n, _P(enc), enc_len, _P(xy), _P(st), None))
    else:
        xy, st = CW._torch_call(lambda i, o: ctx.custom_ed_decode_points_dev(cid, i[0], o[0], o[1]), [enc], [xy, st])
    return xy, st


def run_validate(ctx, cid, xy, order, form="host"):
    xy = np.ascontiguousarray(xy, np.uint8).reshape(-1, 64)
    n = xy.shape[0]
    st, = _filled((n,))
    if form == "host":
        ctx.custom_ed_validate(cid, xy, order, out=(st,))
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_ed_validate_dev(ctx._ctx, cid, n, _P(xy), _order(order), _P(st), None))
    else:
        st, = CW._torch_call(lambda i, o: ctx.custom_ed_validate_dev(cid, i[0], order, o[0]), [xy], [st])
    return st


def run_derive(ctx, cid, k, xy, form="host"):
    k = np.ascontiguousarray(k, np.uint8).reshape(-1, 32)
    xy = np.ascontiguousarray(xy, np.uint8).reshape(-1, 64)
    n = k.shape[0]
    ox, st = _filled((n, 32), (n,))
    if form == "host":
        ctx.custom_ed_derive(cid, k, xy, out=(ox, st))
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_ed_derive_dev(ctx._ctx, cid, n, _P(k), _P(xy), _P(ox), _P(st), None))
    else:
        ox, st = CW._torch_call(lambda i, o: ctx.custom_ed_derive_dev(cid, i[0], i[1], o[0], o[1]), [k, xy], [ox, st])
    return ox, st


def run_derive_wire(ctx, cid, k, enc, form="host", want_err=True):
    """-> (x, status, err); err is None with want_err=False (out_err = NULL)"""
    k = np.ascontiguousarray(k, np.uint8).reshape(-1, 32)
    enc = np.ascontiguousarray(enc, np.uint8)
    n = k.shape[0]
    ox, st, err = _filled((n, 32), (n,), (n,))
    if form == "host":
        ctx.custom_ed_derive_wire(cid, k, enc, out=(ox, st, err) if want_err else (ox, st), want_err=want_err)
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_ed_derive_wire_dev(ctx._ctx, cid, n, _P(k), _P(enc), enc.shape[1], _P(ox), _P(st),
                                                               _P(err) if want_err else None, None))
    else:
        ox, st, err = CW._torch_call(lambda i, o: ctx.custom_ed_derive_wire_dev(cid, i[0], i[1], o[0], o[1], o[2]),
                                     [k, enc], [ox, st, err if want_err else None])
    return ox, st, (err if want_err else None)


def run_encode(ctx, cid, xy, compact, pl, form="host"):
    xy = np.ascontiguousarray(xy, np.uint8).reshape(-1, 64)
    n = xy.shape[0]
    enc, = _filled((n, 1 + (1 if compact else 2) * pl))
    if form == "host":
        ctx.custom_ed_encode_points(cid, xy, compact, out=(enc,))
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_ed_encode_points_dev(ctx._ctx, cid, n, _P(xy), int(compact), _P(enc), None))
    else:
        enc, = CW._torch_call(lambda i, o: ctx.custom_ed_encode_points_dev(cid, i[0], compact, o[0]), [xy], [enc])
    return enc


def _raw_encode(ctx, cid, xy):
    """ellgpu_custom_ed_encode_points itself, whatever the binding knows about the id"""
    out = np.zeros((xy.shape[0], 65), np.uint8)
    CW._raw(ctx, ctx._lib.ellgpu_custom_ed_encode_points(ctx._ctx, cid, xy.shape[0], _P(xy), 0, _P(out)))
    return out


# ---- the recorded cases ---------------------------------------------------------------------

def _xy(h):
    return I(h[:64]), I(h[64:])


def _by_len(cases):
    """encodings grouped by their length: one call per length"""
    groups = {}
    for c in cases:
        groups.setdefault(len(c["enc"]) // 2, []).append(c)
    return groups


def check_golden(ctx, spec, form="host", cid=None):
    """every recorded case of a large curve through the engine and through the model; -> the set of
    (op, status) seen"""
    cid = define(ctx, spec) if cid is None else cid
    m = model_of(spec)
    n_ord = I(spec["n"])
    assert spec["pl"] == m.pl and spec["pmod4"] == m.p % 4
    cs = spec["cases"]
    seen = set()
    for op, from_y in (("fromx", False), ("fromy", True)):
        sel = [c for c in cs if c["op"] == op]
        want = [(_xy(c["xy"]), 0) if "xy" in c else (None, MSG[c["msg"]]) for c in sel]
        for c, w in zip(sel, want):
            assert (m.from_y if from_y else m.from_x)(I(c["v"]), c["odd"]) == w, (spec["name"], c)
        xy, st = run_decompress(ctx, cid, rows([I(c["v"]) for c in sel]), np.array([c["odd"] * 255 for c in sel], np.uint8),
                                from_y, form)
        for c, w, g, s in zip(sel, want, xy, st.tolist()):
            assert (s, _xy(g.tobytes().hex())) == (w[1], w[0] or (0, 0)), (spec["name"], c)
            seen.add((op, s))
    for ln, sel in sorted(_by_len([c for c in cs if c["op"] == "decode"]).items()):
        want = [(_xy(c["xy"]), 0) if "xy" in c else (None, MSG[c["msg"]]) for c in sel]
        for c, w in zip(sel, want):
            assert m.decode(bytes.fromhex(c["enc"])) == w, (spec["name"], c)
        xy, st = run_decode(ctx, cid, np.stack([np.frombuffer(bytes.fromhex(c["enc"]), np.uint8) for c in sel]), form)
        for c, w, g, s in zip(sel, want, xy, st.tolist()):
            assert (s, _xy(g.tobytes().hex())) == (w[1], w[0] or (0, 0)), (spec["name"], c)
            seen.add(("decode", s))
    sel = [c for c in cs if c["op"] == "validate"]
    want = [REASON[c["reason"]] for c in sel]
    pts = [_xy(c["xy"]) for c in sel]
    assert all((w == 0) == (c["result"] == 1) for c, w in zip(sel, want))
    assert [m.validate(x, y, n_ord) for x, y in pts] == want
    assert run_validate(ctx, cid, xy_rows(pts), n_ord, form).tolist() == want, spec["name"]
    assert run_validate(ctx, cid, xy_rows(pts), None, form).tolist() == [0 if w == 3 else w for w in want], spec["name"]
    seen.update(("validate", w) for w in want)
    # derive: raw keys, then the keys over the wire
    DM = {"public point not validated": 1}
    sel = [c for c in cs if c["op"] == "derive" and "xy" in c]
    want = [(I(c["x"]), 0) if "x" in c else (0, DM[c["xmsg"]]) for c in sel]
    assert not any(c.get("z0") for c in cs)                    # complete curves: Z = 0 never occurs
    for c, w in zip(sel, want):
        assert m.derive(I(c["priv"]), *_xy(c["xy"])) == w, (spec["name"], c["tag"])
    ox, st = run_derive(ctx, cid, rows([I(c["priv"]) for c in sel]), xy_rows([_xy(c["xy"]) for c in sel]), form)
    assert list(zip(ints(ox), st.tolist())) == want, spec["name"]
    seen.update(("derive", w[1]) for w in want)
    for ln, sel in sorted(_by_len([c for c in cs if c["op"] == "derive" and "enc" in c]).items()):
        want = [(0, 3, MSG[c["dmsg"]]) if "dmsg" in c else (I(c["x"]), 0, 0) if "x" in c else (0, DM[c["xmsg"]], 0) for c in sel]
        for c, w in zip(sel, want):
            assert m.derive_wire(I(c["priv"]), bytes.fromhex(c["enc"])) == w, (spec["name"], c["tag"])
        k = rows([I(c["priv"]) for c in sel])
        enc = np.stack([np.frombuffer(bytes.fromhex(c["enc"]), np.uint8) for c in sel])
        ox, st, err = run_derive_wire(ctx, cid, k, enc, form)
        assert list(zip(ints(ox), st.tolist(), err.tolist())) == want, (spec["name"], ln)
        ox2, st2, _ = run_derive_wire(ctx, cid, k, enc, form, want_err=False)
        assert (ox2 == ox).all() and (st2 == st).all()
        seen.update(("derive_wire", w[1]) for w in want)
    sel = [c for c in cs if c["op"] == "encode"]
    pts = xy_rows([_xy(c["xy"]) for c in sel])
    for compact, f in ((True, "compact"), (False, "full")):
        enc = run_encode(ctx, cid, pts, compact, m.pl, form)
        for c, g in zip(sel, enc):
            assert g.tobytes().hex() == c[f] == m.encode(*_xy(c["xy"]), compact).hex(), (spec["name"], c["tag"])
    return seen


def toy_result(r):
    return ((r[0], r[1]), 0) if isinstance(r, list) else (None, MSG[r])


def check_toy(ctx, spec, form="host"):
    """the exhaustive rows of a toy curve: every abscissa and ordinate, both parities; then every
    point of the plane through validate and, with small scalars, through derive -- the engine's
    ladder against its model, Z = 0 included (d is a square on p13_d4: an incomplete law)
    -> the statuses seen: (decompress, derive)"""
    cid = define(ctx, spec)
    m = model_of(spec)
    p = m.p
    seen = set()
    for f, from_y in (("fx", False), ("fy", True)):
        for odd in (0, 1):
            want = [toy_result(r[f][odd]) for r in spec["rows"]]
            for r, w in zip(spec["rows"], want):
                assert (m.from_y if from_y else m.from_x)(r["v"], odd) == w, (spec["name"], f, r["v"], odd)
            xy, st = run_decompress(ctx, cid, rows([r["v"] for r in spec["rows"]]), np.full(p, odd, np.uint8), from_y, form)
            assert [(s, _xy(g.tobytes().hex())) for g, s in zip(xy, st.tolist())] == [(w[1], w[0] or (0, 0)) for w in want], \
                (spec["name"], f, odd)
            seen.update(st.tolist())
    plane = [(x, y) for x in range(p) for y in range(p)]
    assert run_validate(ctx, cid, xy_rows(plane), None, form).tolist() == [m.validate(x, y) for x, y in plane]
    on = [pt for pt in plane if m.on_curve(*pt)]
    dseen = set()
    for k in (0, 1, 2, 3, 5, 8, 13, 2 * p + 3):
        ox, st = run_derive(ctx, cid, rows([k] * len(on)), xy_rows(on), form)
        assert list(zip(ints(ox), st.tolist())) == [m.derive(k, x, y) for x, y in on], (spec["name"], k)
        assert run_validate(ctx, cid, xy_rows(on), k, form).tolist() == [m.validate(x, y, k) for x, y in on], (spec["name"], k)
        dseen.update(st.tolist())
    return seen, dseen


# ---- random batches -------------------------------------------------------------------------

def _curve_point(m, rng):
    while True:
        pt, st = m.from_y(rng.randrange(2, m.p), rng.random() < 0.5)
        if st == 0 and pt[0]:
            return pt


def random_batch(spec, n, seed, distinct=257):
    """n items and the model's answers, for every call.
    Coordinates (decompress): random values, about half with a root; the first items are 0, 1, p - 1
    and a value >= p.  Keys (validate, derive, derive_wire): about 70 % points of the curve, 10 % the
    identity or (0, -1), 20 % points off the curve; over the wire a tenth of the keys do not decode
    (bad prefix, hybrid mismatch, an x without a root).  The first items hold one of each status the
    curve can give.  The model's roots and ladders are slow in Python, so the items repeat with period
    `distinct` (a prime: no multiple of a wave, a workgroup or an inversion group)."""
    rng = random.Random("custom-ed:%s:%d" % (spec["name"], seed))
    m = model_of(spec)
    p = m.p
    d = min(n, distinct)
    bad_x = next(x for x in range(2, 1000) if m.from_x(x, 0)[1])
    bad_y = next(y for y in range(2, 1000) if m.from_y(y, 0)[1])
    vs = [0, 1, p - 1, p + 1 if p + 1 < TOP else 2, bad_x, bad_y] + [rng.getrandbits(256) if rng.random() < 0.2 else rng.randrange(p) for _ in range(d)]
    vs = vs[:d]
    odd = [rng.getrandbits(1) * rng.choice([1, 2, 255]) for _ in range(d)]          # a non-zero byte means true
    odd[:4] = [0, 1, 0, 1][:d]                                # pointFromY(1, true): 'invalid point' before any root
    fx = [m.from_x(v, o) for v, o in zip(vs, odd)]
    fy = [m.from_y(v, o) for v, o in zip(vs, odd)]
    order = rng.getrandbits(256) | 1
    ks, pts, kinds, enc_full, enc_comp = [], [], [], [], []
    for i in range(d):
        r = rng.random()
        kind = i if i < 4 else (0 if r < 0.70 else 1 if r < 0.80 else 2 if r < 0.9 else 3)
        k = rng.getrandbits(256) if rng.random() < 0.7 else rng.getrandbits(rng.randrange(1, 256))
        pt = _curve_point(m, rng)
        if kind == 1:
            pt = (0, 1) if i & 1 else (0, p - 1)
        if kind in (2, 3):                                    # off the curve; over the wire kind 3 does not decode
            pt = (pt[0], (pt[1] + 1 + rng.randrange(p - 2)) % p)
            if m.on_curve(*pt):
                pt = (pt[0], (pt[1] + 1) % p)
        if pt[0] + p < TOP and pt[1] + p < TOP and rng.random() < 0.1:
            pt = (pt[0] + p, pt[1] + p)
        full, comp = m.encode(*pt, False), m.encode(*pt, True)
        if kind == 3:                                         # a bad prefix, a hybrid mismatch / a short-form prefix, no root
            c = i % 3
            full = (b"\x05" + full[1:], bytes([7 - (full[-1] & 1)]) + full[1:], b"\x03" + full[1:])[c]
            comp = (b"\x05" + comp[1:], b"\x04" + comp[1:], b"\x02" + bad_x.to_bytes(m.pl, "big"))[c]
        elif rng.random() < 0.5:
            full = bytes([6 + (full[-1] & 1)]) + full[1:]
        ks.append(k)
        pts.append(pt)
        kinds.append(kind)
        enc_full.append(full)
        enc_comp.append(comp)
    val = [m.validate(x, y) for x, y in pts]
    valo = [m.validate(x, y, order) for x, y in pts]
    der = [m.derive(k, x, y) for k, (x, y) in zip(ks, pts)]
    tile = lambda a: [a[i % d] for i in range(n)]
    wire = {}
    for name, encs in (("full", enc_full), ("comp", enc_comp)):
        w = [m.derive_wire(k, e) for k, e in zip(ks, encs)]
        wire[name] = {"k": rows(tile(ks)), "enc": np.stack([np.frombuffer(e, np.uint8) for e in tile(encs)]),
                      "x": rows(tile([a[0] for a in w])), "st": np.array(tile([a[1] for a in w]), np.uint8),
                      "err": np.array(tile([a[2] for a in w]), np.uint8)}
    good = [pt for pt, v in zip(pts, val) if v != 2]
    return {"n": n, "v": rows(tile(vs)), "odd": np.array(tile(odd), np.uint8), "order": order, "pl": m.pl,
            "fx_xy": xy_rows(tile([r[0] or (0, 0) for r in fx])), "fx_st": np.array(tile([r[1] for r in fx]), np.uint8),
            "fy_xy": xy_rows(tile([r[0] or (0, 0) for r in fy])), "fy_st": np.array(tile([r[1] for r in fy]), np.uint8),
            "k": rows(tile(ks)), "xy": xy_rows(tile(pts)), "kind": np.array(tile(kinds)),
            "val": np.array(tile(val), np.uint8), "valo": np.array(tile(valo), np.uint8),
            "dx": rows(tile([a[0] for a in der])), "dst": np.array(tile([a[1] for a in der]), np.uint8),
            "wire": wire, "enc_c": np.stack([np.frombuffer(m.encode(*pt, True), np.uint8) for pt in tile(pts)]),
            "enc_f": np.stack([np.frombuffer(m.encode(*pt, False), np.uint8) for pt in tile(pts)]),
            "statuses": statuses_of(spec), "good": good}


def statuses_of(spec):
    """what each call can answer on a complete curve: (decompress, validate without order, derive,
    derive_wire)"""
    nr = 3 if I(spec["p"]) % 4 == 1 else 2
    return {"fx": {0, nr}, "fy": {0, 2, nr}, "val": {0, 1, 2}, "dst": {0, 1}, "wst": {0, 1, 3}}


def model_meets_conditions(bt, n):
    """every status the curve can give occurs within the first 257 items, and at least 60 % of the
    derive items are shared secrets"""
    h = min(n, 257)
    s = bt["statuses"]
    wst = set(bt["wire"]["full"]["st"][:h].tolist()) | set(bt["wire"]["comp"]["st"][:h].tolist())
    return (set(bt["fx_st"][:h].tolist()) == s["fx"] and set(bt["fy_st"][:h].tolist()) == s["fy"]
            and set(bt["val"][:h].tolist()) == s["val"] and set(bt["dst"][:h].tolist()) == s["dst"] and wst == s["wst"]
            and (bt["dst"][:n] == 0).sum() >= 0.6 * n)


def check_batch(ctx, spec, bt, n, form="host", cid=None):
    """the first n items of a batch through every call"""
    cid = define(ctx, spec) if cid is None else cid
    tag = (spec["name"], n, form)
    for f, from_y in (("fx", False), ("fy", True)):
        xy, st = run_decompress(ctx, cid, bt["v"][:n], bt["odd"][:n], from_y, form)
        assert (st == bt[f + "_st"][:n]).all() and (xy == bt[f + "_xy"][:n]).all(), tag + (f,)
    assert (run_validate(ctx, cid, bt["xy"][:n], None, form) == bt["val"][:n]).all(), tag
    assert (run_validate(ctx, cid, bt["xy"][:n], bt["order"], form) == bt["valo"][:n]).all(), tag
    dx, dst = run_derive(ctx, cid, bt["k"][:n], bt["xy"][:n], form)
    assert (dst == bt["dst"][:n]).all() and (dx == bt["dx"][:n]).all(), tag
    for w in bt["wire"].values():
        ox, st, err = run_derive_wire(ctx, cid, w["k"][:n], w["enc"][:n], form)
        assert (st == w["st"][:n]).all() and (err == w["err"][:n]).all() and (ox == w["x"][:n]).all(), tag
        xy, st = run_decode(ctx, cid, w["enc"][:n], form)
        assert (st == w["err"][:n]).all(), tag
    for compact, f in ((True, "enc_c"), (False, "enc_f")):
        assert (run_encode(ctx, cid, bt["xy"][:n], compact, bt["pl"], form) == bt[f][:n]).all(), tag
    return dx, dst


def check_derive_wire_regrow(make_ctx, spec, w, forms, sizes=(3, 257, 3)):
    """custom_ed_derive_wire in ONE context on one curve at n = 3, 257 and 3 again, each size through
    every form: the scratch arena regrows between the calls, under the decoder's passes, which work in
    buffers that the derive chunk holds.  w: one of random_batch()'s wire sets, of at least max(sizes)
    items.  Every result equals the same batch in a fresh context of its own, and the model's answer."""
    ctx = make_ctx()
    try:
        cid = define(ctx, spec)
        got = [(n, form, run_derive_wire(ctx, cid, w["k"][:n], w["enc"][:n], form)) for n in sizes for form in forms]
    finally:
        ctx.close()
    for n, form, (ox, st, err) in got:
        fresh = make_ctx()
        try:
            fx, fst, ferr = run_derive_wire(fresh, define(fresh, spec), w["k"][:n], w["enc"][:n], form)
        finally:
            fresh.close()
        tag = (spec["name"], n, form)
        assert (ox == fx).all() and (st == fst).all() and (err == ferr).all(), tag
        assert (ox == w["x"][:n]).all() and (st == w["st"][:n]).all() and (err == w["err"][:n]).all(), tag
    return got


def check_symmetry(ctx, spec, n, seed, form="host", cid=None):
    """derive(a, b G) = derive(b, a G) through the engine alone: G from custom_ed_decompress, a G and
    b G from mul_var, the second leg over the wire through custom_ed_encode_points"""
    cid = define(ctx, spec) if cid is None else cid
    m = model_of(spec)
    rng = random.Random("custom-ed-ecdh:%s:%d" % (spec["name"], seed))
    y = next(y for y in range(2, 1000) if m.from_y(y, 0)[1] == 0 and m.from_y(y, 0)[0][0])
    g, st = run_decompress(ctx, cid, rows([y] * n), np.zeros(n, np.uint8), True, form)
    assert not st.any()
    a = rows([rng.getrandbits(256) for _ in range(n)])
    b = rows([rng.getrandbits(256) for _ in range(n)])
    ag, ia = ctx.mul_var(cid, a, g)
    bg, ib = ctx.mul_var(cid, b, g)
    assert not ia.any() and not ib.any()
    assert not run_validate(ctx, cid, ag, None, form).any()
    s1, st1 = run_derive(ctx, cid, a, bg, form)
    for compact in (True, False):
        s2, st2, err = run_derive_wire(ctx, cid, b, run_encode(ctx, cid, ag, compact, m.pl, form), form)
        assert not st1.any() and not st2.any() and not err.any() and (s1 == s2).all() and s1.any(axis=1).all()
