"""Checks of the run-time-modulus field (csrc/fp_rt.h: FpMontRT over a user-defined curve's p,
FpMontRTn over a domain's n) and of the group law on user-defined curves across the prime range,
shared by the CPU test (tests/test_rt_field_hostsim.py, the hostsim build of the device code) and
the GPU test (tests/test_gpu_rt_field.py).

Field operations go through the white-box probe (ellgpu_debug_field_op ids 100+slot / 200+slot,
hs_rt_field_op in the hostsim build) and are compared with Python integers, exactly.  The module
restates Montgomery reduction and modular addition on plain integers only to CLASSIFY its own
vectors (which branch of FpMontRTm::redc / mod_add an operand pair takes) and asserts that every
class is populated on the primes where it exists.

Group-law expectations: the preset curves' own results (a preset defined again as a user-defined
curve must compute the same numbers), the recorded EC#verify verdicts and the C oracle, and --
for primes no fixture has -- an affine chord-and-tangent law on Python integers that shares no
formula with the device's Jacobian code.

required_classes() holds the minima asserted per modulus, as classify() counts the vectors (redc:
the mul and the sqr of every operand pair, two per pair; add: one per pair): 50 in each redc class
on P08; u >= 2^256: 300 on the primes above 2^256 - 2^225; p <= u < 2^256: 100 on the two 2^255
primes; sum >= 2^256: 300 wherever 2p > 2^256; p <= sum < 2^256: 300 wherever p < 2^255."""
import ctypes
import json
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
R = 1 << 256


def _custom_ecdsa():
    with open(os.path.join(HERE, "golden", "custom_ecdsa.json")) as f:
        return {c["name"]: c for c in json.load(f)}


def _oracle_curve(name):
    from oracle import ec_oracle as O
    return O.get_curve(name, False)


BRAINPOOL = _custom_ecdsa()["brainpoolP256r1"]
BP_P, BP_N = int(BRAINPOOL["p"], 16), int(BRAINPOOL["n"], 16)
K256_P = 2 ** 256 - 2 ** 32 - 977
P256_P = 2 ** 256 - 2 ** 224 + 2 ** 192 + 2 ** 96 - 1
# the smallest prime = 3 (mod 4) above 0.8 * 2^256: all three outcomes of the reduction's last step
# (u < p, p <= u < 2^256, u >= 2^256) are common for random operands (about 77 / 15 / 8 per cent)
P08 = 0xCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCD9F

MODULI_P = [5, 7, 13, 2 ** 31 - 1, 2 ** 32 - 5, 2 ** 32 + 15, 2 ** 64 - 59, 2 ** 64 + 13, 2 ** 128 - 159, 2 ** 128 + 51,
            2 ** 224 - 63, 2 ** 224 + 735, 2 ** 255 - 19, 2 ** 255 + 95, BP_P, P08,
            2 ** 256 - 2 ** 224 + 223, P256_P, K256_P, 2 ** 256 - 189]
NEAR_2_256 = [2 ** 256 - 2 ** 224 + 223, P256_P, K256_P, 2 ** 256 - 189]      # the primes above 2^256 - 2^225
NEAR_2_255 = [2 ** 255 - 19, 2 ** 255 + 95]
# order fields: (label, n, how the domain is registered)
MODULI_N = ["secp256k1", "p256", "p224", "brainpoolP256r1", "m61"]
# primes the fixtures do not have, all = 3 (mod 4): group law against the affine reference
NEW_PRIMES = [7, 2 ** 31 - 1, 2 ** 32 - 5, 2 ** 32 + 15, 2 ** 128 + 51, 2 ** 224 + 735, 2 ** 255 + 95,
              2 ** 256 - 2 ** 224 + 223, 2 ** 256 - 189]
TOY_PRIMES = [5, 7, 13]
PRESETS = ["secp256k1", "p256", "p224", "p192"]


def order_modulus(label):
    if label == "brainpoolP256r1":
        return BP_N
    if label == "m61":
        return 2 ** 61 - 1
    return _oracle_curve(label).n


def is_prime(n):
    """Miller-Rabin: the first twelve primes as bases (a proof below 3.3e24) and sixteen seeded ones"""
    small = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37]
    if n < 2:
        return False
    for q in small:
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    rnd = random.Random(n)
    for a in small + [rnd.randrange(2, n - 1) for _ in range(16)]:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


# ---- how a test reaches the library ------------------------------------------------------------

class Env:
    """lib: the loaded library (libellgpu.so or the hostsim build); contexts are made on demand --
    at most 16 definitions fit in one -- and closed by close()"""

    def __init__(self, lib, hostsim):
        import elliptic_amd
        self._mk = (lambda: elliptic_amd.Context(0, lib_path=lib)) if hostsim else (lambda: elliptic_amd.Context(0))
        self.lib = lib if hostsim else None
        self.hostsim = hostsim
        self._ctxs = []
        self._fields = {}
        self._pool, self._used = None, 0
        self._fn = None
        if hostsim:
            self._fn = lib.hs_rt_field_op                        # (the library's own probe is declared by elliptic_amd._lib)
            self._fn.restype = ctypes.c_int
            self._fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_void_p]

    def new_ctx(self):
        c = self._mk()
        self._ctxs.append(c)
        return c

    def close(self):
        for c in self._ctxs:
            c.close()
        self._ctxs = []
        self._fields = {}
        self._pool, self._used = None, 0

    def _room(self):
        """a context with a free definition slot (16 definitions fit in one)"""
        if self._pool is None or self._used >= 16:
            self._pool, self._used = self.new_ctx(), 0
        self._used += 1
        return self._pool

    def probe(self, ctx, field, op, A, B):
        """r = a <op> b on (n, 8) uint32 arrays; returns (status, R)"""
        A, B = np.ascontiguousarray(A, np.uint32), np.ascontiguousarray(B, np.uint32)
        out = np.zeros_like(A)
        fn = self._fn if self.hostsim else ctx._lib.ellgpu_debug_field_op
        rc = fn(ctx._ctx, field, op, A.shape[0], A.ctypes.data, B.ctypes.data, out.ctypes.data)
        return rc, out

    def field_p(self, p):
        """(ctx, field id) of FpMontRT over p: any curve over p will do"""
        key = ("p", p)
        if key not in self._fields:
            ctx = self._room()
            cid = ctx.define_short(p, 1, 1)
            self._fields[key] = (ctx, 100 + cid - 16)
        return self._fields[key]

    def field_n(self, label):
        """(ctx, field id) of FpMontRTn over the order `label` names: the real curve where n is a
        group order, secp192k1's curve and G for 2^61 - 1 (n need not be G's order)"""
        key = ("n", label)
        if key not in self._fields:
            ctx = self._room()
            cid = ctx.define_short_domain(*domain_params(label))
            self._fields[key] = (ctx, 200 + cid - 16)
        return self._fields[key]


def domain_params(label):
    specs = _custom_ecdsa()
    if label in specs or label == "m61":
        s = specs["secp192k1" if label == "m61" else label]
        n = 2 ** 61 - 1 if label == "m61" else int(s["n"], 16)
        return int(s["p"], 16), int(s["a"], 16), int(s["b"], 16), n, int(s["g"]["x"], 16), int(s["g"]["y"], 16)
    c = _oracle_curve(label)
    return c.p, c.a, c.b, c.n, c.g.x, c.g.y


def pack(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), "<u4").reshape(-1, 8).copy()


def unpack(arr):
    raw = np.ascontiguousarray(arr, "<u4").tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(arr))]


# ---- the vectors -------------------------------------------------------------------------------

def edge_values(p):
    """the edge list of test_field_ops_gpu (8 limbs), reduced"""
    top = R - 1
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, p >> 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1,
            top, top >> 1, int("ffffffff00000000" * 8, 16), int("00000000ffffffff" * 8, 16)]
    return [v % p for v in vals]


def unreduced_values(p, rnd):
    """operands in [p, 2^256): the edge list lifted by multiples of p, the top of the range, and
    random ones (none for a p so close to 2^256 that the range is all but empty)"""
    out = [p, p + 1, R - 1, R - 2, R - p if R - p >= p else p, (R - 1) // p * p, (R - 1) // p * p - 1 if (R - 1) // p > 1 else p]
    for v in edge_values(p):
        k = (R - 1 - v) // p                                  # the largest lift that still fits
        if k >= 1:
            out += [v + p, v + k * p]
    out += [rnd.randrange(p, R) for _ in range(64)]
    assert all(p <= v < R for v in out)
    return out


def binary_operands(p, seed):
    """(a, b): edge pairs, the rare pairs of test_field_ops_gpu, unreduced operands on either side,
    pairs whose Montgomery forms sit just under p (their sum wraps 2^256 for every p > 2^255, however
    close to 2^255), and 1500 random pairs"""
    import math
    rnd = random.Random(seed)
    edge = edge_values(p)
    a = list(edge)
    b = [edge[(i * 7 + 3) % len(edge)] for i in range(len(edge))]
    rare = [(2, (p + 1) // 2), (3, (p + 2) // 3), (math.isqrt(p) + 1, math.isqrt(p) + 1),
            (math.isqrt(p) + 1, math.isqrt(p) + 2), (p - 1, p - 1), (p - 1, 2),
            (1, p - 1), (p - 1, 1), (2, p - 1), (p - 2, 2), (p - 2, 3), (0, 1), (1, 2), (0, p - 1)]
    a += [x % p for x, _ in rare]
    b += [y % p for _, y in rare]
    unr = unreduced_values(p, rnd)
    a += unr + [edge[i % len(edge)] for i in range(len(unr))] + unr
    b += [edge[(i * 5 + 1) % len(edge)] for i in range(len(unr))] + unr + unr[::-1]
    if p > 64:
        rinv = pow(R, -1, p)
        for i in range(20):
            for j in range(20):
                a.append((p - 1 - i) * rinv % p)              # Montgomery form p - 1 - i
                b.append((p - 1 - j) * rinv % p)
    a += [rnd.randrange(p) for _ in range(1500)]
    b += [rnd.randrange(p) for _ in range(1500)]
    return a, b


def inv_operands(p, seed):
    rnd = random.Random(seed ^ 0x1234)
    vals = edge_values(p) + [3, (p + 1) // 2, 1 << 30, (1 << 30) - 1, (1 << 60) + 1]
    vals += [(1 << k) for k in range(0, 256, 7)]               # powers of two, reduced or not
    vals += [p, p + 1, R - 1] + [rnd.randrange(p, R) for _ in range(8)]
    vals += [rnd.randrange(p) for _ in range(300)]
    return vals


OPS = ((0, lambda x, y, p: (x + y) % p), (1, lambda x, y, p: (x - y) % p), (2, lambda x, y, p: x * y % p),
       (3, lambda x, y, p: x * x % p), (5, lambda x, y, p: (-x) % p), (6, lambda x, y, p: 2 * x % p),
       (7, lambda x, y, p: 4 * x % p), (8, lambda x, y, p: 8 * x % p))


def redc_class(t, p, ninv):
    """Montgomery reduction on integers: u = (t + (t * -p^-1 mod R) * p) / R before the final
    subtraction; 0: u < p, 1: p <= u < 2^256, 2: u >= 2^256"""
    u = (t + (t * ninv % R) * p) >> 256
    assert u < 2 * p
    return 0 if u < p else 1 if u < R else 2


def add_class(s, p):
    """modular addition of two residues: 0: sum < p, 1: p <= sum < 2^256, 2: sum >= 2^256"""
    return 0 if s < p else 1 if s < R else 2


def classify(p, a, b):
    """per class, the number of (mul, a, b) and (sqr, a) vectors whose product of Montgomery forms
    reduces there, and of (add, a, b) vectors whose sum of Montgomery forms lands there"""
    ninv = (-pow(p, -1, R)) % R
    redc, add = [0, 0, 0], [0, 0, 0]
    for x, y in zip(a, b):
        xm, ym = x * R % p, y * R % p
        redc[redc_class(xm * ym, p, ninv)] += 1
        redc[redc_class(xm * xm, p, ninv)] += 1
        add[add_class(xm + ym, p)] += 1
    return redc, add


def required_classes(p):
    """what the vectors must hold for modulus p: {(kind, class): minimum}"""
    need = {}
    if p == P08:
        need.update({("redc", 0): 50, ("redc", 1): 50, ("redc", 2): 50})
    if p > R - 2 ** 225:
        need[("redc", 2)] = 300
    if p in NEAR_2_255:
        need[("redc", 1)] = 100
    if 2 * p > R:
        need[("add", 2)] = 300
    if p < 2 ** 255:
        need[("add", 1)] = 300
    return need


def check_field(env, ctx, field, p, seed):
    """every operation of the probe on the vectors of modulus p against Python integers; returns
    the class counts (redc, add) of the vectors"""
    a, b = binary_operands(p, seed)
    A, B = pack(a), pack(b)
    for op, fn in OPS:
        rc, out = env.probe(ctx, field, op, A, B)
        assert rc == 0, (field, op, rc)
        got = unpack(out)
        for i in range(len(a)):
            assert got[i] == fn(a[i], b[i], p), (hex(p), op, hex(a[i]), hex(b[i]), hex(got[i]))
    inv_in = inv_operands(p, seed)
    A2 = pack(inv_in)
    rc, out = env.probe(ctx, field, 4, A2, A2)
    assert rc == 0
    for v, g in zip(inv_in, unpack(out)):
        assert g == (pow(v % p, -1, p) if v % p else 0), (hex(p), "inv", hex(v), hex(g))
    rc, out = env.probe(ctx, field, 4, pack([0]), pack([0]))
    assert rc == 0 and unpack(out) == [0]
    redc, add = classify(p, a, b)
    for (kind, cls), least in required_classes(p).items():
        have = (redc if kind == "redc" else add)[cls]
        assert have >= least, (hex(p), kind, cls, have, least)
    return redc, add


def check_probe_refusals(env):
    """ids without a domain, unknown slots, unknown ids and, on the run-time fields, ops other than
    0..8 answer ELLGPU_E_ARG"""
    ctx = env.new_ctx()
    plain = ctx.define_short(P08, 1, 1)
    dom = ctx.define_short_domain(*domain_params("secp192k1"))
    z = pack([1])
    assert env.probe(ctx, 100 + plain - 16, 0, z, z)[0] == 0
    assert env.probe(ctx, 200 + plain - 16, 0, z, z)[0] == -2          # a plain curve has no order
    assert env.probe(ctx, 200 + dom - 16, 0, z, z)[0] == 0
    assert env.probe(ctx, 100 + dom - 16, 0, z, z)[0] == 0
    for field in (100 + 2, 200 + 2, 100 + 15, 200 + 15, 99, 116, 216, 300):
        assert env.probe(ctx, field, 0, z, z)[0] == -2, field
    for field in (100 + plain - 16, 200 + dom - 16):
        for op in (-1, 9, 10, 13):
            assert env.probe(ctx, field, op, z, z)[0] == -2, (field, op)
        assert env.probe(ctx, field, 8, z, z)[0] == 0
    # the two blocks of one context do not leak into each other: p of one, then n of the other
    rc, out = env.probe(ctx, 100 + plain - 16, 2, pack([P08 - 1]), pack([P08 - 1]))
    assert rc == 0 and unpack(out) == [1]
    n192 = domain_params("secp192k1")[3]
    rc, out = env.probe(ctx, 200 + dom - 16, 2, pack([n192 - 1]), pack([n192 - 2]))
    assert rc == 0 and unpack(out) == [2]


# ---- group law ---------------------------------------------------------------------------------

def b32(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in vals), np.uint8).reshape(-1, 32).copy()


def xy32(pts):
    """affine points (None -> zeros) -> (n, 64) bytes"""
    return np.concatenate([b32([0 if q is None else q[0] for q in pts]), b32([0 if q is None else q[1] for q in pts])], axis=1)


def results(xy, inf):
    """(n, 2B) bytes + flags -> list of None (infinity) / (x, y) / ('status', v)"""
    B = xy.shape[1] // 2
    out = []
    for i in range(len(xy)):
        if inf[i] == 1:
            out.append(None)
        elif inf[i] != 0:
            out.append(("status", int(inf[i])))
        else:
            out.append((int.from_bytes(xy[i, :B].tobytes(), "big"), int.from_bytes(xy[i, B:].tobytes(), "big")))
    return out


def aff_add(P, Q, a, p):
    """chord and tangent on affine points, None = the point at infinity"""
    if P is None:
        return Q
    if Q is None:
        return P
    (x1, y1), (x2, y2) = P, Q
    if x1 == x2:
        if (y1 + y2) % p == 0:
            return None
        lam = (3 * x1 * x1 + a) * pow(2 * y1, -1, p) % p
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return x3, (lam * (x1 - x3) - y1) % p


def aff_mul(k, P, a, p):
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = aff_add(acc, acc, a, p)
        if bit == "1":
            acc = aff_add(acc, P, a, p)
    return acc


def seeded_curve(p, seed):
    """a, b with 4a^3 + 27b^2 != 0 and a pool of points from an x-scan (p = 3 mod 4)"""
    assert p % 4 == 3
    rnd = random.Random(seed)
    while True:
        a, b = rnd.randrange(1, p), rnd.randrange(1, p)
        if (4 * a ** 3 + 27 * b * b) % p == 0:
            continue
        pts = []
        x = rnd.randrange(p)
        for _ in range(min(p, 400)):
            v = (x * x * x + a * x + b) % p
            y = pow(v, (p + 1) // 4, p)
            if y * y % p == v:
                pts.append((x, y if rnd.random() < 0.5 else (-y) % p))
            if len(pts) == 24:
                break
            x = (x + 1) % p
        if len(pts) >= 3:
            return a, b, pts


def check_new_prime(ctx, p):
    """mul_var on 200 items, mul_add2 on 100, point_add on 100 plus the exceptional pairs, and the
    off-curve statuses, against the affine law; returns the number of items"""
    a, b, pts = seeded_curve(p, 77 + p % 1000)
    cid = ctx.define_short(p, a, b)
    rnd = random.Random(p % 65521)
    n = 200
    ks = [0, 1, 2, 3, R - 1, p, p - 1, p + 1] + [rnd.getrandbits(rnd.choice((8, 64, 255, 256))) for _ in range(n - 8)]
    ps = [pts[rnd.randrange(len(pts))] for _ in range(n)]
    want = [aff_mul(k, P, a, p) for k, P in zip(ks, ps)]
    got = results(*ctx.mul_var(cid, b32(ks), xy32(ps)))
    for i in range(n):
        assert got[i] == want[i], (hex(p), "mul_var", hex(ks[i]), ps[i], got[i], want[i])
    m = 100
    k2 = [rnd.getrandbits(256) for _ in range(m - 4)] + [0, 1, ks[10], 0]
    q2 = [pts[rnd.randrange(len(pts))] for _ in range(m - 4)] + [ps[0], ps[1], (ps[10][0], (-ps[10][1]) % p), ps[3]]
    k1 = ks[:m - 4] + [5, 0, ks[10], 0]                          # ..., k*P + k*(-P) = O, 0*P + 0*Q = O
    p1 = ps[:m - 4] + [ps[0], ps[1], ps[10], ps[2]]
    want2 = [aff_add(aff_mul(k1[i], p1[i], a, p), aff_mul(k2[i], q2[i], a, p), a, p) for i in range(m)]
    got = results(*ctx.mul_add2(cid, b32(k1), xy32(p1), b32(k2), xy32(q2)))
    for i in range(m):
        assert got[i] == want2[i], (hex(p), "mul_add2", i, got[i], want2[i])
    assert want2[-1] is None and want2[-2] is None
    # point_add: random pairs, P + P, P + (-P), infinity on either side and on both
    A = [pts[rnd.randrange(len(pts))] for _ in range(m)]
    Bq = [pts[rnd.randrange(len(pts))] for _ in range(m)]
    for i in range(0, 24, 4):
        Bq[i] = A[i]
        Bq[i + 1] = (A[i + 1][0], (-A[i + 1][1]) % p)
        A[i + 2] = None
        Bq[i + 3] = None
    A[30] = Bq[30] = None
    want3 = [aff_add(A[i], Bq[i], a, p) for i in range(m)]
    i1 = np.array([1 if q is None else 0 for q in A], np.uint8)
    i2 = np.array([1 if q is None else 0 for q in Bq], np.uint8)
    got = results(*ctx.point_add(cid, xy32(A), xy32(Bq), inf1=i1, inf2=i2))
    for i in range(m):
        assert got[i] == want3[i], (hex(p), "point_add", A[i], Bq[i], got[i], want3[i])
    # y + 1 is never on the curve together with y unless y = (p - 1) / 2
    off = [(x, (y + 1) % p) for x, y in ps]
    really = [(y + 1) % p != (-y) % p for _, y in ps]
    assert sum(really) > n // 2
    xy, inf = ctx.mul_var(cid, b32(ks), xy32(off))
    for i in range(n):
        if really[i]:
            assert inf[i] == 2 and not xy[i].any(), (hex(p), "off-curve mul_var", i)
    xy, inf = ctx.mul_add2(cid, b32(ks[:m]), xy32(ps[:m]), b32(ks[:m]), xy32(off[:m]))
    for i in range(m):
        if really[i]:
            assert inf[i] == 2 and not xy[i].any(), (hex(p), "off-curve mul_add2", i)
    return n + 2 * m


def toy_curve(p):
    """the first non-singular (a, b) over a toy prime whose group has a point of order two (y = 0)
    and points that are not; returns (a, b, every affine point)"""
    for a in range(1, p):
        for b in range(p):
            if (4 * a ** 3 + 27 * b * b) % p == 0:
                continue
            pts = [(x, y) for x in range(p) for y in range(p) if (y * y - x * x * x - a * x - b) % p == 0]
            if any(y == 0 for _, y in pts) and sum(1 for _, y in pts if y) >= 4:
                return a, b, pts
    raise AssertionError("no toy curve over %d" % p)


def check_toy_exhaustive(ctx, p):
    """every point times every k in [0, 2 #E + 2], and every ordered pair (infinity included)
    through point_add, on one curve over a toy prime"""
    a, b, pts = toy_curve(p)
    cid = ctx.define_short(p, a, b)
    order = len(pts) + 1
    ks, ps = [], []
    for P in pts:
        for k in range(2 * order + 3):
            ks.append(k)
            ps.append(P)
    want = [aff_mul(k, P, a, p) for k, P in zip(ks, ps)]
    assert all(aff_mul(order, P, a, p) is None for P in pts)              # the reference itself: #E kills every point
    assert any(aff_add(P, P, a, p) is None for P in pts)                  # a 2-torsion point is among them
    got = results(*ctx.mul_var(cid, b32(ks), xy32(ps)))
    for i in range(len(ks)):
        assert got[i] == want[i], (p, "mul_var", ks[i], ps[i], got[i], want[i])
    allp = pts + [None]
    A = [P for P in allp for _ in allp]
    Bq = [Q for _ in allp for Q in allp]
    i1 = np.array([1 if q is None else 0 for q in A], np.uint8)
    i2 = np.array([1 if q is None else 0 for q in Bq], np.uint8)
    got = results(*ctx.point_add(cid, xy32(A), xy32(Bq), inf1=i1, inf2=i2))
    for i in range(len(A)):
        assert got[i] == aff_add(A[i], Bq[i], a, p), (p, "point_add", A[i], Bq[i], got[i])
    # and every pair of points with small multipliers through the two-scalar ladder
    k1 = [(3 * i + 1) % (order + 2) for i in range(len(pts) ** 2)]
    k2 = [(5 * i + 2) % (order + 3) for i in range(len(pts) ** 2)]
    P1 = [P for P in pts for _ in pts]
    P2 = [Q for _ in pts for Q in pts]
    got = results(*ctx.mul_add2(cid, b32(k1), xy32(P1), b32(k2), xy32(P2)))
    for i in range(len(P1)):
        w = aff_add(aff_mul(k1[i], P1[i], a, p), aff_mul(k2[i], P2[i], a, p), a, p)
        assert got[i] == w, (p, "mul_add2", k1[i], P1[i], k2[i], P2[i], got[i], w)
    return len(ks) + len(A) + len(P1)


# ---- presets defined again as user-defined curves ----------------------------------------------

def preset_spec(name):
    """a preset in the shape custom_domain_checks works with"""
    c = _oracle_curve(name)
    return {"name": "preset_" + name, "p": "%x" % c.p, "a": "%x" % c.a, "b": "%x" % c.b, "n": "%x" % c.n,
            "g": {"x": "%x" % c.g.x, "y": "%x" % c.g.y}}


def _widen(xy, B):
    """(n, 2B) preset bytes -> (n, 64)"""
    n = xy.shape[0]
    out = np.zeros((n, 64), np.uint8)
    out[:, 32 - B:32] = xy[:, :B]
    out[:, 64 - B:] = xy[:, B:]
    return out


def _narrow_k(ks, c, B):
    """scalars for the preset's B-byte interface: k itself where it fits, k mod n where it does not
    (every point in these tests lies in the group of prime order n)"""
    from elliptic_amd import ints_to_be
    return ints_to_be([k if k < (1 << (8 * B)) else k % c.n for k in ks], B)


def check_preset_as_custom(ctx, name):
    """mul_var, mul_add2 (two points; p1 = None on the domain), mul_fixed and point_add on the
    preset's parameters registered through define_short and define_short_domain: the numbers the
    preset id gives, on 300 seeded items plus k = 0, 1, 2, n - 1, n, n + 1, 2^256 - 1"""
    from elliptic_amd import FIELD_BYTES, ints_to_be
    c = _oracle_curve(name)
    B = FIELD_BYTES[name]
    plain = ctx.define_short(c.p, c.a, c.b)
    dom = ctx.define_short_domain(c.p, c.a, c.b, c.n, c.g.x, c.g.y)
    assert plain != dom
    rnd = random.Random(sum(map(ord, name)))
    edge = [0, 1, 2, c.n - 1, c.n, c.n + 1, R - 1]
    ks = edge + [rnd.getrandbits(256) for _ in range(300)]
    n = len(ks)
    # points: multiples of G by the preset's comb, one of them with every edge scalar
    seeds = ints_to_be([rnd.randrange(1, c.n) for _ in range(n)], B)
    pxy, pinf = ctx.mul_fixed(name, seeds)
    assert not pinf.any()
    pts = _widen(pxy, B)
    kb = b32(ks)
    kn = _narrow_k(ks, c, B)
    wxy, winf = ctx.mul_var(name, kn, pxy)
    assert winf[0] == 1 and winf[4] == 1 and not winf[7:].any()
    for cid in (plain, dom):
        xy, inf = ctx.mul_var(cid, kb, pts)
        assert np.array_equal(inf, winf) and np.array_equal(xy, _widen(wxy, B)), (name, cid, "mul_var")
    # k1*P1 + k2*P2: the edge scalars on either side
    k2 = ks[::-1]
    p2 = np.roll(pts, 1, axis=0)
    wxy, winf = ctx.mul_add2(name, kn, pxy, _narrow_k(k2, c, B), np.roll(pxy, 1, axis=0))
    for cid in (plain, dom):
        xy, inf = ctx.mul_add2(cid, kb, pts, b32(k2), p2)
        assert np.array_equal(inf, winf) and np.array_equal(xy, _widen(wxy, B)), (name, cid, "mul_add2")
    # the domain's own generator: k*G and k1*G + k2*P
    wxy, winf = ctx.mul_fixed(name, kn)
    xy, inf = ctx.mul_fixed(dom, kb)
    assert np.array_equal(inf, winf) and np.array_equal(xy, _widen(wxy, B)), (name, "mul_fixed")
    assert winf[0] == 1 and winf[4] == 1
    wxy, winf = ctx.mul_add2(name, kn, None, _narrow_k(k2, c, B), np.roll(pxy, 1, axis=0))
    xy, inf = ctx.mul_add2(dom, kb, None, b32(k2), p2)
    assert np.array_equal(inf, winf) and np.array_equal(xy, _widen(wxy, B)), (name, "mul_add2 with G")
    # Point#add: random pairs, P + P, P + (-P), infinity flags
    q = np.roll(pxy, 5, axis=0)
    q[:20] = pxy[:20]
    neg = ints_to_be([(c.p - int.from_bytes(pxy[i, B:].tobytes(), "big")) % c.p for i in range(20, 40)], B)
    q[20:40, :B] = pxy[20:40, :B]
    q[20:40, B:] = neg
    i1 = np.zeros(n, np.uint8)
    i2 = np.zeros(n, np.uint8)
    i1[40:50] = 1
    i2[45:60] = 1
    wxy, winf = ctx.point_add(name, pxy, q, inf1=i1, inf2=i2)
    assert winf[20:40].all() and winf[45:50].all() and not winf[:20].any()
    for cid in (plain, dom):
        xy, inf = ctx.point_add(cid, pts, _widen(q, B), inf1=i1, inf2=i2)
        assert np.array_equal(inf, winf) and np.array_equal(xy, _widen(wxy, B)), (name, cid, "point_add")
    return n


def check_preset_verify(ctx, name):
    """ecdsa_verify on the preset's parameters as a domain: the recorded EC#verify verdicts whose
    digest, r and s fit 32 bytes (with the preset's status), and 2048 random items against the C
    oracle; returns the number of recorded cases"""
    import custom_domain_checks as CD
    from elliptic_amd import ORDER_BYTES, FIELD_BYTES, ints_to_be
    from golden_util import I, verify_cases
    c = _oracle_curve(name)
    B, NB = FIELD_BYTES[name], ORDER_BYTES[name]
    dom = ctx.define_short_domain(c.p, c.a, c.b, c.n, c.g.x, c.g.y)
    cs = [v for v in verify_cases(name) if len(v["z"]) == 64 and len(v["r"]) <= 64 and len(v["s"]) <= 64]
    assert len(cs) >= 15
    z = np.frombuffer(b"".join(bytes.fromhex(v["z"]) for v in cs), np.uint8).reshape(-1, 32)
    r = [I(v["r"]) % R for v in cs]
    s = [I(v["s"]) % R for v in cs]
    q = np.concatenate([ints_to_be([I(v["qx"]) for v in cs], 32), ints_to_be([I(v["qy"]) for v in cs], 32)], axis=1)
    ok, st = ctx.ecdsa_verify(dom, z, b32(r), b32(s), q, status=True)
    # the preset's own answer where r and s fit its NB-byte interface; wider ones are out of range
    # for n < 2^(8 NB): verdict 0, status 0
    fits = [i for i in range(len(cs)) if r[i] < (1 << (8 * NB)) and s[i] < (1 << (8 * NB))]
    pq = np.concatenate([q[:, 32 - B:32], q[:, 64 - B:]], axis=1)
    pok, pst = ctx.ecdsa_verify(name, z[fits], ints_to_be([r[i] for i in fits], NB), ints_to_be([s[i] for i in fits], NB),
                                pq[fits], status=True)
    want_ok = np.zeros(len(cs), np.uint8)
    want_st = np.zeros(len(cs), np.uint8)
    want_ok[fits], want_st[fits] = pok, pst
    assert np.array_equal(st, want_st), (name, np.nonzero(st != want_st)[0])
    assert np.array_equal(ok, want_ok), (name, np.nonzero(ok != want_ok)[0])
    for i, v in enumerate(cs):
        if st[i] == 0:
            assert ok[i] == (1 if v["ok"] else 0), (name, v)
    assert 0 < int(ok.sum()) < len(cs)
    spec = preset_spec(name)
    h, rr, ss, qq, expect = CD.random_batch(spec, 2048, seed=256 + len(name))
    ok, st = ctx.ecdsa_verify(dom, h, rr, ss, qq, status=True)
    want = CD.oracle_verify(spec, h, rr, ss, qq)
    assert not st.any()
    assert np.array_equal(ok, want), np.nonzero(ok != want)[0][:10]
    known = [i for i, e in enumerate(expect) if e is not None]
    assert len(known) > 700 and all(ok[i] == 1 for i in known)
    assert 0 < int(ok.sum()) < len(ok)
    return len(cs)


def check_ed25519_as_custom(ctx):
    """ed25519's (p, a = -1, d) through define_edwards: mul_var, mul_add2 and point_add give the
    preset's bytes on 200 items.  The flags differ by contract (include/ellgpu.h): the preset's
    out_inf mirrors Point#isInfinity(), a user-defined Edwards curve leaves it 0 -- the identity is
    the ordinary point (0, 1) on both"""
    from elliptic_amd import ints_to_be
    c = _oracle_curve("ed25519")
    cid = ctx.define_edwards(c.p, c.a, c.d)
    rnd = random.Random(25519)
    n = 200
    pxy, pinf = ctx.mul_fixed("ed25519", ints_to_be([rnd.randrange(1, c.n) for _ in range(n)], 32))
    assert not pinf.any()
    ks = [0, 1, 2, c.n - 1, c.n, c.n + 1, R - 1] + [rnd.getrandbits(256) for _ in range(n - 7)]
    kb = b32(ks)
    wxy, winf = ctx.mul_var("ed25519", kb, pxy)
    xy, inf = ctx.mul_var(cid, kb, pxy)
    ident = np.concatenate([b32([0]), b32([1])], axis=1)[0]

    def same(what):
        assert np.array_equal(xy, wxy) and not inf.any(), what
        assert np.array_equal(winf == 1, (wxy == ident).all(axis=1)), what
    same("mul_var")
    assert winf[0] == 1 and winf[4] == 1 and winf.sum() == 2
    k2 = b32(ks[::-1])
    p2 = np.roll(pxy, 1, axis=0)
    wxy, winf = ctx.mul_add2("ed25519", kb, pxy, k2, p2)
    xy, inf = ctx.mul_add2(cid, kb, pxy, k2, p2)
    same("mul_add2")
    q = np.roll(pxy, 3, axis=0)
    q[:20] = pxy[:20]                                             # P + P
    q[20:40, :32] = ints_to_be([(c.p - int.from_bytes(pxy[i, :32].tobytes(), "big")) % c.p for i in range(20, 40)], 32)
    q[20:40, 32:] = pxy[20:40, 32:]                               # P + (-P) = (0, 1)
    wxy, winf = ctx.point_add("ed25519", pxy, q)
    xy, inf = ctx.point_add(cid, pxy, q)
    same("point_add")
    assert winf[20:40].all() and winf.sum() == 20
    return n
