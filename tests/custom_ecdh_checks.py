"""Checks of the key side on user-defined short-curve domains -- ellgpu_custom_derive,
_custom_derive_wire, _custom_validate, _custom_encode_points -- shared by the CPU test
(tests/test_custom_ecdh_hostsim.py, the hostsim build of the device code) and the GPU test
(tests/test_custom_ecdh_gpu.py):

  * the reference's shared secrets, statuses, thrown messages and encodings recorded in
    tests/golden/custom_ecdh.json (tools/gen_golden_custom_ecdh.js);
  * random batches against a model over Python integers that restates KeyPair#derive
    (ec/key.js:101-107), KeyPair#validate (key.js:40-51), BaseCurve#decodePoint (base.js:270-293)
    and BasePoint#encode (base.js:295-311): toRed, the curve equation, double-and-add,
    x.to_bytes(PL).

The model's multiplication is done twice: by the C oracle's mul for every item, and by
double-and-add over Python integers for a sample of them (the first SAMPLE_HEAD items, every
SAMPLE_STEP-th after, and every constructed item), which must agree -- the whole batch over
integers alone would take a minute at the largest size.

Every call is run in one of three forms: "host" (host buffers), "dev_np" (the _dev entry point on
the hostsim build, where device memory is host memory) and "dev_torch" (the _dev entry point on
torch tensors).  Result arrays are pre-filled with 0xA5, so a byte the call leaves unwritten shows."""
import json
import os
import random

import numpy as np

import custom_domain_checks as CD
import custom_wire_checks as CW
import custom_recover_checks as CR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "custom_ecdh.json")
FILL = CW.FILL
ERR_OF = {"Unknown point format": 1, "invalid point": 2, "Assertion failed": 3}
SAMPLE_HEAD, SAMPLE_STEP = 48, 37
ALWAYS_BELOW = 400               # constructed items below this index always go through the integers too
TOP = 1 << 256

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


def xy64(x, y):
    return np.concatenate([b32(x), b32(y)])


# ---- the three forms of the calls -----------------------------------------------------------

def _P(a):
    return a.ctypes.data if a is not None else None


def run_derive(ctx, cid, priv, pub, form="host"):
    priv, pub = (np.ascontiguousarray(a, np.uint8) for a in (priv, pub))
    n = priv.shape[0]
    x, st = np.full((n, 32), FILL, np.uint8), np.full((n,), FILL, np.uint8)
    if form == "host":
        ctx.custom_derive(cid, priv, pub, out=(x, st))
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_derive_dev(ctx._ctx, cid, n, _P(priv), _P(pub), _P(x), _P(st), None))
    else:
        x, st = CW._torch_call(lambda i, o: ctx.custom_derive_dev(cid, i[0], i[1], o[0], o[1]), [priv, pub], [x, st])
    return x, st


def run_derive_wire(ctx, cid, priv, enc, form="host", want_err=True):
    priv, enc = (np.ascontiguousarray(a, np.uint8) for a in (priv, enc))
    n, pub_len = enc.shape
    x, st = np.full((n, 32), FILL, np.uint8), np.full((n,), FILL, np.uint8)
    err = np.full((n,), FILL, np.uint8) if want_err else None
    if form == "host":
        if want_err:
            ctx.custom_derive_wire(cid, priv, enc, out=(x, st, err))
        else:
            assert ctx.custom_derive_wire(cid, priv, enc, out=(x, st), want_err=False)[2] is None
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_derive_wire_dev(ctx._ctx, cid, n, _P(priv), _P(enc), pub_len, _P(x), _P(st),
                                                            _P(err), None))
    else:
        x, st, err = CW._torch_call(lambda i, o: ctx.custom_derive_wire_dev(cid, i[0], i[1], o[0], o[1], o[2]),
                                    [priv, enc], [x, st, err])
    return x, st, err


def run_validate(ctx, cid, xy, inf, check_order, form="host"):
    xy = np.ascontiguousarray(xy, np.uint8)
    inf = np.ascontiguousarray(inf, np.uint8) if inf is not None else None
    n = xy.shape[0]
    st = np.full((n,), FILL, np.uint8)
    if form == "host":
        ctx.custom_validate(cid, xy, inf, check_order, out=(st,))
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_validate_dev(ctx._ctx, cid, n, _P(xy), _P(inf), 1 if check_order else 0,
                                                         _P(st), None))
    else:
        st, = CW._torch_call(lambda i, o: ctx.custom_validate_dev(cid, i[0], i[1], check_order, o[0]), [xy, inf], [st])
    return st


def run_encode(ctx, cid, xy, compact, pl, form="host"):
    xy = np.ascontiguousarray(xy, np.uint8)
    n = xy.shape[0]
    enc = np.full((n, 1 + pl if compact else 1 + 2 * pl), FILL, np.uint8)
    if form == "host":
        ctx.custom_encode_points(cid, xy, compact, out=(enc,))
        assert ctx.custom_encode_points(cid, xy[:1], compact).shape == (1, enc.shape[1])
    elif form == "dev_np":
        CW._raw(ctx, ctx._lib.ellgpu_custom_encode_points_dev(ctx._ctx, cid, n, _P(xy), 1 if compact else 0, _P(enc),
                                                              None))
    else:
        enc, = CW._torch_call(lambda i, o: ctx.custom_encode_points_dev(cid, i[0], compact, o[0]), [xy], [enc])
    return enc


# ---- the reference's recorded answers ---------------------------------------------------------

def _want_x(c):
    return b32(I(c["out"])).tobytes() if c["st"] == 0 else bytes(32)


def check_golden(ctx, spec, form="host", cid=None):
    """every recorded case of the four calls; returns the statuses seen per call"""
    cid = define(ctx, spec) if cid is None else cid
    p, n = I(spec["p"]), I(spec["n"])
    pl = spec["pl"]
    assert pl == (p.bit_length() + 7) // 8
    seen = {}
    # derive
    cs = spec["derive"]
    priv = np.stack([b32(I(c["priv"])) for c in cs])
    pub = np.stack([xy64(I(c["x"]), I(c["y"])) for c in cs])
    x, st = run_derive(ctx, cid, priv, pub, form)
    for i, c in enumerate(cs):
        what = (spec["name"], "derive", c["tag"], c, int(st[i]))
        assert (c["st"] == 1) == (c.get("msg") == "public point not validated"), what
        assert st[i] == c["st"] and x[i].tobytes() == _want_x(c), what
    seen["derive"] = set(int(v) for v in st)
    assert seen["derive"] == {0, 1, 2}
    tags = {c["tag"] for c in cs}
    assert {"pair", "priv_1", "priv_n_minus_1", "priv_n", "priv_n_plus_1", "priv_0", "off_curve_y"} <= tags
    assert "priv_all_ones" in tags and (2 * p >= TOP or "xy_plus_p" in tags)
    # ECDH symmetry of the recorded pairs
    pairs = [c for c in cs if c["tag"] == "pair"]
    assert len(pairs) == 8 and all(pairs[i]["out"] == pairs[i + 1]["out"] for i in range(0, 8, 2))
    # derive_wire: one call per encoding length
    groups = {}
    for c in spec["derive_wire"]:
        groups.setdefault(len(c["enc"]) // 2, []).append(c)
    assert {1 + pl, 1 + 2 * pl} < set(groups)                   # both lengths, and wrong ones
    seen["wire"], seen["err"] = set(), set()
    for ln, cs in sorted(groups.items()):
        priv = np.stack([b32(I(c["priv"])) for c in cs])
        enc = np.stack([np.frombuffer(bytes.fromhex(c["enc"]), np.uint8) for c in cs])
        x, st, err = run_derive_wire(ctx, cid, priv, enc, form)
        for i, c in enumerate(cs):
            what = (spec["name"], "derive_wire", c["tag"], c, int(st[i]), int(err[i]))
            assert (c["st"] == 3) == (c["err"] != 0) and ERR_OF.get(c.get("msg"), 0) == c["err"], what
            assert st[i] == c["st"] and err[i] == c["err"] and x[i].tobytes() == _want_x(c), what
        if ln in (1 + pl, 1 + 2 * pl):
            x2, st2, none = run_derive_wire(ctx, cid, priv, enc, form, want_err=False)
            assert none is None and (x2 == x).all() and (st2 == st).all()
        seen["wire"] |= set(int(v) for v in st)
        seen["err"] |= set(int(v) for v in err)
    assert seen["wire"] == {0, 1, 2, 3}
    assert seen["err"] == ({0, 1, 2, 3} if p % 4 == 3 else {0, 1, 3}), seen["err"]
    prefixes = {c["enc"][:2] for c in spec["derive_wire"] if c["err"] == 0}
    assert {"02", "03", "04"} <= prefixes and prefixes & {"06", "07"}
    # validate, with and without the order test
    cs = spec["validate"]
    xy = np.stack([xy64(I(c["x"]), I(c["y"])) for c in cs])
    inf = np.array([c["inf"] for c in cs], np.uint8)
    st = run_validate(ctx, cid, xy, inf, True, form)
    st0 = run_validate(ctx, cid, xy, inf, False, form)
    for i, c in enumerate(cs):
        what = (spec["name"], "validate", c["tag"], c, int(st[i]), int(st0[i]))
        assert st[i] == c["st"] and st0[i] == c["st0"], what
    fin = inf == 0
    assert (run_validate(ctx, cid, xy[fin], None, True, form) == st[fin]).all()       # inf may be NULL
    seen["validate"] = set(int(v) for v in st)
    assert seen["validate"] == ({0, 1, 2, 3} if p // n >= 7 else {0, 1, 2})
    if p // n >= 7:
        assert {"order_2", "order_4", "order_8", "order_8n"} <= {c["tag"] for c in cs if c["st"] == 3}
    # encode
    cs = spec["encode"]
    xy = np.stack([xy64(I(c["x"]), I(c["y"])) for c in cs])
    for compact, key in ((False, "full"), (True, "compact")):
        enc = run_encode(ctx, cid, xy, compact, pl, form)
        for i, c in enumerate(cs):
            assert enc[i].tobytes().hex() == c[key], (spec["name"], "encode", c["tag"], key, enc[i].tobytes().hex())
    assert any(c["full"][2:4] == "00" for c in cs)                                   # leading zero bytes
    return seen


# ---- the model over Python integers -----------------------------------------------------------

def pt_mul(p, a, k, P):
    """k P by double-and-add; None is the point at infinity"""
    acc = None
    for i in range(k.bit_length() - 1, -1, -1):
        acc = CR.pt_add(p, a, acc, acc)
        if (k >> i) & 1:
            acc = CR.pt_add(p, a, acc, P)
    return acc


def pt_dbl_safe(p, a, P):
    return CR.pt_add(p, a, P, P)


def on_curve(p, a, b, x, y):
    return (y * y - (x * x * x + a * x + b)) % p == 0


def model_decode(spec, enc):
    """BaseCurve#decodePoint -> (err, (x, y) reduced or None)"""
    p, a, b = I(spec["p"]), I(spec["a"]), I(spec["b"])
    pl = spec["pl"]
    enc = bytes(enc)
    tag = enc[0] if enc else 0
    if tag in (4, 6, 7) and len(enc) == 1 + 2 * pl:
        if (tag == 6 and enc[-1] & 1) or (tag == 7 and not enc[-1] & 1):
            return 3, None
        return 0, (int.from_bytes(enc[1:1 + pl], "big") % p, int.from_bytes(enc[1 + pl:], "big") % p)
    if tag in (2, 3) and len(enc) == 1 + pl:
        x = int.from_bytes(enc[1:], "big") % p
        rhs = (x * x * x + a * x + b) % p
        if rhs != 0 and pow(rhs, (p - 1) // 2, p) != 1:
            return (2 if p % 4 == 3 else 3), None
        y = CR.sqrt_mod(rhs, p)
        if (y & 1) != (tag & 1):
            y = (p - y) % p
        return 0, (x, y)
    return 1, None


def model_mul_x(spec, ks, pts, always=(), head=SAMPLE_HEAD):
    """x of k P per item (None: infinity): the C oracle for all, integers for a sample (the first
    `head` items and every SAMPLE_STEP-th) and for the items listed in `always`"""
    from oracle import c_oracle
    p, a = I(spec["p"]), I(spec["a"])
    name = CD.oracle_name(spec)
    cnt = len(ks)
    out = [None] * cnt
    if cnt:
        q, inf = c_oracle.mul_mt(name, np.stack([b32(k) for k in ks]), np.stack([xy64(*P) for P in pts]), threads=8)
        for i in range(cnt):
            out[i] = None if inf[i] else int.from_bytes(q[i, :32].tobytes(), "big")
    sample = set(i for i in range(cnt) if i < head or i % SAMPLE_STEP == 0) | set(always)
    for i in sorted(sample):
        Q = pt_mul(p, a, ks[i], pts[i])
        assert out[i] == (None if Q is None else Q[0]), (spec["name"], i, hex(ks[i]), pts[i])
    return out


def model_derive(spec, priv, points, always=(), head=SAMPLE_HEAD):
    """priv: ints; points: (x, y) ints as given (unreduced) or None for a key that did not decode
    -> (st list, x bytes list)"""
    p, a, b = I(spec["p"]), I(spec["a"]), I(spec["b"])
    cnt = len(priv)
    st = [0] * cnt
    live = []
    for i in range(cnt):
        if points[i] is None:
            st[i] = 3
        else:
            x, y = points[i][0] % p, points[i][1] % p                # toRed
            if on_curve(p, a, b, x, y):
                live.append((i, priv[i], (x, y)))
            else:
                st[i] = 1
    pos = {i: m for m, (i, _, _) in enumerate(live)}
    xs = model_mul_x(spec, [k for _, k, _ in live], [P for _, _, P in live], [pos[i] for i in always if i in pos], head)
    out = [bytes(32)] * cnt
    for (i, _, _), x in zip(live, xs):
        if x is None:
            st[i] = 2
        else:
            out[i] = x.to_bytes(32, "big")
    return st, out


def low_order_points(spec):
    """points of order 2, 4, 8 recorded for a cofactor curve (the fixture's `order_*` cases), else []"""
    return [(I(c["x"]), I(c["y"])) for c in spec["validate"] if c["tag"] in ("order_2", "order_4", "order_8")]


def random_batch(spec, n, seed):
    """n items by rule, of every 20: 13 valid subgroup peers d G (the oracle's), 3 off the curve,
    2 with a coordinate >= p where 32 bytes hold it (else the peer as it is), 2 constructed:
    priv = 0 / n / a multiple of n and, on a cofactor curve, low-order peers.  Private keys are
    random 256-bit values for every fourth item (Point#mul takes them as they stand), else below n.
    -> dict priv (n, 32), pub (n, 64), own (n, 32: the peer's private key, zeros where there is
    none), st, x (the model's answers), constructed (indices)"""
    key = ("batch", spec["name"], n, seed)
    if key in _cache:
        return _cache[key]
    from oracle import c_oracle
    p, a, b, nn, gx, gy = CD.params(spec)
    name = CD.oracle_name(spec)
    rnd = random.Random(seed)
    d = [rnd.randrange(1, nn) for _ in range(n)]
    pts, inf = c_oracle.mul_mt(name, np.stack([b32(v) for v in d]), threads=8)
    assert not inf.any()
    low = low_order_points(spec)
    priv, pub, constructed = [], [], []
    own = np.zeros((n, 32), np.uint8)
    nc = 0
    for i in range(n):
        kind = i % 20
        k = rnd.randrange(0, TOP) if i % 4 == 3 else rnd.randrange(1, nn)
        x = int.from_bytes(pts[i, :32].tobytes(), "big")
        y = int.from_bytes(pts[i, 32:].tobytes(), "big")
        if kind < 13:
            own[i] = b32(d[i])
        elif kind < 16:
            which = rnd.randrange(3)
            if which == 0:
                y = (y + 1 + rnd.randrange(p - 1)) % p
            elif which == 1:
                x, y = rnd.randrange(p), rnd.randrange(p)
                if on_curve(p, a, b, x, y):
                    y = (y + 1) % p
            else:
                x, y = y, x
                if on_curve(p, a, b, x, y):
                    y = (y + 1) % p
        elif kind < 18:
            if kind == 16 and x + p < TOP:
                x += p
            elif y + p < TOP:
                y += p
            elif x + p < TOP:
                x += p
        else:
            constructed.append(i)
            choice = nc % (6 if low else 3)
            nc += 1
            if choice == 0:
                k = 0
            elif choice == 1:
                k = nn
            elif choice == 2:
                k = nn * rnd.randrange(2, max(3, TOP // nn)) if 2 * nn < TOP else nn
            else:
                x, y = low[choice - 3]
                if rnd.randrange(2):
                    k = 8 * rnd.randrange(1, 1 << 200)
        priv.append(k)
        pub.append((x, y))
    out = {"priv": np.stack([b32(k) for k in priv]), "pub": np.stack([xy64(*P) for P in pub]), "own": own,
           "constructed": np.array(constructed, np.int64)}
    checked = [i for i in constructed if i < ALWAYS_BELOW]
    st, xs = model_derive(spec, priv, pub, checked)
    out["st"] = np.array(st, np.uint8)
    out["x"] = np.frombuffer(b"".join(xs), np.uint8).reshape(n, 32).copy()
    # validate's answers for the same points: every third item flagged as infinity
    out["inf"] = np.array([1 if i % 3 == 2 else 0 for i in range(n)], np.uint8)
    vst0 = [1 if out["inf"][i] else (2 if st[i] == 1 else 0) for i in range(n)]
    live = [i for i in range(n) if vst0[i] == 0]
    pos = {i: m for m, i in enumerate(live)}
    nx = model_mul_x(spec, [nn] * len(live), [(pub[i][0] % p, pub[i][1] % p) for i in live],
                     [pos[i] for i in checked if i in pos])
    vst = list(vst0)
    for i, v in zip(live, nx):
        if v is not None:
            vst[i] = 3
    out["vst0"], out["vst"] = np.array(vst0, np.uint8), np.array(vst, np.uint8)
    for v in out.values():
        v.setflags(write=False)
    _cache[key] = out
    return out


def model_meets_conditions(bt, n):
    """what check_batch asks of a batch of n >= 257 items, on the model alone"""
    st = bt["st"][:n]
    return set(int(v) for v in st) == {0, 1, 2} and (st == 0).sum() >= 0.6 * n


def check_batch(ctx, spec, bt, n, form="host", cid=None):
    """derive and validate on the first n items of a random batch, item by item against the model"""
    cid = define(ctx, spec) if cid is None else cid
    p, nn = I(spec["p"]), I(spec["n"])
    x, st = run_derive(ctx, cid, bt["priv"][:n], bt["pub"][:n], form)
    bad = np.nonzero(st != bt["st"][:n])[0]
    assert bad.size == 0, (spec["name"], n, form, bad[:10], st[bad[:10]], bt["st"][bad[:10]])
    bad = np.nonzero((x != bt["x"][:n]).any(axis=1))[0]
    assert bad.size == 0, (spec["name"], n, form, bad[:10])
    vst = run_validate(ctx, cid, bt["pub"][:n], bt["inf"][:n], True, form)
    bad = np.nonzero(vst != bt["vst"][:n])[0]
    assert bad.size == 0, (spec["name"], n, form, "validate", bad[:10], vst[bad[:10]], bt["vst"][bad[:10]])
    vst0 = run_validate(ctx, cid, bt["pub"][:n], bt["inf"][:n], False, form)
    assert (vst0 == bt["vst0"][:n]).all(), (spec["name"], n, form, "validate without the order test")
    if n >= 257:
        # conditions, so that the test cannot pass on a batch of error rows
        assert set(int(v) for v in st) == {0, 1, 2}, set(int(v) for v in st)
        assert (st == 0).sum() >= 0.6 * n, (int((st == 0).sum()), n)
        if p // nn >= 7:
            assert {0, 2, 3} <= set(int(v) for v in vst), set(int(v) for v in vst)
        else:
            assert {0, 1, 2} <= set(int(v) for v in vst)
    return x, st


def check_symmetry(ctx, spec, bt, n, form="host", cid=None):
    """ECDH through the engine alone: derive(a, b G) = derive(b, a G) for the batch's valid peers
    b G and fresh keys a, with a G from the engine's own mul_fixed"""
    cid = define(ctx, spec) if cid is None else cid
    nn = I(spec["n"])
    idx = np.nonzero(bt["own"][:n].any(axis=1) & (bt["st"][:n] == 0))[0]
    assert idx.size >= min(n, 13) * 0.6
    rnd = random.Random(n)
    a = np.stack([b32(rnd.randrange(1, nn)) for _ in idx])
    aG, inf = ctx.mul_fixed(cid, a)
    assert not inf.any()
    s1, st1 = run_derive(ctx, cid, a, bt["pub"][idx], form)
    s2, st2 = run_derive(ctx, cid, bt["own"][idx], aG, form)
    assert not st1.any() and not st2.any() and (s1 == s2).all() and s1.any(axis=1).all()


def wire_batch(spec, bt, n, compact):
    """the first n items of a random batch as SEC1 encodings of one length: the points reduced mod p
    (PL bytes cannot hold more), 02 / 03 or 04 / 06 / 07 with the right prefix -- except, of every
    20 items, one with a wrong prefix (err 1) and one that does not decode: a compressed x without
    a root (err 2 where p = 3 mod 4, else 3) or a hybrid prefix contradicting y (err 3).  A
    compressed off-curve peer keeps its x: it decodes to a curve point or to no point.
    -> (enc (n, len), st, x, err: the model's answers)"""
    key = ("wire", spec["name"], id(bt), n, compact)
    if key in _cache:
        return _cache[key]
    p = I(spec["p"])
    pl = spec["pl"]
    encs, pts = [], []
    priv = [int.from_bytes(r.tobytes(), "big") for r in bt["priv"][:n]]
    for i in range(n):
        x = int.from_bytes(bt["pub"][i, :32].tobytes(), "big") % p
        y = int.from_bytes(bt["pub"][i, 32:].tobytes(), "big") % p
        kind = i % 20
        if compact:
            tag = 2 + (y & 1)
            if kind == 5:
                tag = (4, 0, 5, 7)[(i // 20) % 4]
            elif kind == 11:
                while model_decode(spec, bytes([tag]) + x.to_bytes(pl, "big"))[0] == 0:
                    x = (x + 1) % p
            e = bytes([tag]) + x.to_bytes(pl, "big")
        else:
            tag = (4, 6 + (y & 1), 4)[i % 3]
            if kind == 5:
                tag = (2, 3, 0, 8)[(i // 20) % 4]
            elif kind == 11:
                tag = 7 - (y & 1)
            e = bytes([tag]) + x.to_bytes(pl, "big") + y.to_bytes(pl, "big")
        encs.append(np.frombuffer(e, np.uint8))
        pts.append(model_decode(spec, e))
    # (the same multiplications as the raw batch's, which the integers have sampled: a short head here)
    st, xs = model_derive(spec, priv, [P for _, P in pts], head=12)
    out = (np.stack(encs), np.array(st, np.uint8), np.frombuffer(b"".join(xs), np.uint8).reshape(n, 32).copy(),
           np.array([e for e, _ in pts], np.uint8))
    _cache[key] = out
    return out


def check_wire_batch(ctx, spec, bt, n, form="host", cid=None):
    """derive_wire on the first n items, compressed and uncompressed, against the model"""
    cid = define(ctx, spec) if cid is None else cid
    p = I(spec["p"])
    errs = set()
    for compact in (True, False):
        enc, wst, wx, werr = wire_batch(spec, bt, n, compact)
        x, st, err = run_derive_wire(ctx, cid, bt["priv"][:n], enc, form)
        bad = np.nonzero((st != wst) | (err != werr))[0]
        assert bad.size == 0, (spec["name"], n, form, compact, bad[:10], st[bad[:10]], wst[bad[:10]], err[bad[:10]], werr[bad[:10]])
        bad = np.nonzero((x != wx).any(axis=1))[0]
        assert bad.size == 0, (spec["name"], n, form, compact, bad[:10])
        assert ((err != 0) == (st == 3)).all()
        errs |= set(int(v) for v in err)
        if n >= 257:
            # (a compressed key carries no y to be wrong: 'not validated' needs the uncompressed form)
            assert ({0, 2, 3} if compact else {0, 1, 2, 3}) <= set(int(v) for v in st), (compact, set(st))
            assert (st == 0).sum() >= 0.6 * n, (compact, int((st == 0).sum()), n)
    if n >= 257:
        # 'invalid point' (2) exists only where p = 3 (mod 4): elsewhere bn.js asserts first (3)
        assert errs == ({0, 1, 2, 3} if p % 4 == 3 else {0, 1, 3}), errs


def check_encode_batch(ctx, spec, bt, n, form="host", cid=None):
    cid = define(ctx, spec) if cid is None else cid
    p = I(spec["p"])
    pl = spec["pl"]
    for compact in (False, True):
        enc = run_encode(ctx, cid, bt["pub"][:n], compact, pl, form)
        for i in range(n):
            x = int.from_bytes(bt["pub"][i, :32].tobytes(), "big") % p
            y = int.from_bytes(bt["pub"][i, 32:].tobytes(), "big") % p
            want = (bytes([2 + (y & 1)]) + x.to_bytes(pl, "big")) if compact else (b"\x04" + x.to_bytes(pl, "big") + y.to_bytes(pl, "big"))
            assert enc[i].tobytes() == want, (spec["name"], n, form, compact, i)


def check_random(ctx, spec, n, seed, form="host", cid=None):
    """all four calls on a random batch of n items against the model; returns derive's (x, st)"""
    bt = random_batch(spec, n, seed)
    cid = define(ctx, spec) if cid is None else cid
    out = check_batch(ctx, spec, bt, n, form, cid)
    check_wire_batch(ctx, spec, bt, n, form, cid)
    check_encode_batch(ctx, spec, bt, n, form, cid)
    return out
