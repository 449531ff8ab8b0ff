"""Checks of the lanes-per-item field layers -- FpK256C / FpK256R (csrc/coop.h), FpMontC / FpFoldC
(csrc/coop_mont.h), FpFoldW (csrc/coop_wide.h), Fp25519C (csrc/coop_ed.h) -- operation by operation
against Python integers, shared by the CPU test (tests/test_coop_field_hostsim.py: the hostsim build,
whose rows are arrays of sixteen lanes) and the GPU test (tests/test_gpu_coop_field.py: the DPP,
readlane and permlane moves themselves).

Everything goes through the white-box probe (ellgpu_debug_field_op on the device, hs_field_op in the
hostsim build; the same field ids and ops) and every comparison is exact equality with a Python
integer.  Nothing here compares one build with the other, or a row field with a one-lane field.

Field ids: 3 FpK256C, 4 FpK256R (four items per wave, one per row), 5 Fp25519C, 31 / 32 / 33 the row
fields of p192 / p224 / p256, 34 / 35 the wave-wide fields of p384 / p521.

Operands above p: every from_plain of the layer takes any value of the field's 32-bit words (coop.h and
coop_ed.h scatter the exact digits of a 256-bit value, coop_mont.h and coop_wide.h reduce by a product);
on 35 the top digit keeps 32 bits from bit 504, and the header promises the 66 bytes of the ABI: the
lists stay below 2^528 there.

coverage() restates no code under test: it classifies the operand pairs on integers (sums below and
at or above p, differences of both signs, a zero product of non-zero factors, a product whose lowest
digit is zero) and both test files assert that every class is populated for every field."""
import ctypes
import math
import random

import numpy as np

import field_vectors

K256_P = 2 ** 256 - 2 ** 32 - 977
P25519 = 2 ** 255 - 19
FIELDS = {
    3: K256_P, 4: K256_P, 5: P25519,
    31: 2 ** 192 - 2 ** 64 - 1, 32: 2 ** 224 - 2 ** 96 + 1, 33: 2 ** 256 - 2 ** 224 + 2 ** 192 + 2 ** 96 - 1,
    34: 2 ** 384 - 2 ** 128 - 2 ** 96 + 2 ** 32 - 1, 35: 2 ** 521 - 1,
}
LIMBS = {3: 8, 4: 8, 5: 8, 31: 6, 32: 7, 33: 8, 34: 12, 35: 17}          # 32-bit words of a plain value
RADIX = {3: 29, 4: 29, 5: 29, 31: 29, 32: 29, 33: 29, 34: 28, 35: 28}    # bits of a digit (one per lane)
DIGITS = {3: 9, 4: 9, 5: 9, 31: 9, 32: 9, 33: 9, 34: 14, 35: 19}
CAP = {f: (1 << 528) if f == 35 else (1 << (32 * LIMBS[f])) for f in FIELDS}   # operands lie below this
K256_ROWS = (3, 4)
QUAD4 = (3, 5)                     # pack4 / unpack4: ops 20..23
QUAD = (3, 5, 31, 32, 33)          # pack2 / pack3: ops 24..28


def expected(field, op, x, y):
    """what op returns for the plain operands x, y (any admitted value), as an integer in [0, p)"""
    p = FIELDS[field]
    s, d = x + y, x - y
    return {
        0: lambda: s % p, 1: lambda: d % p, 2: lambda: x * y % p, 3: lambda: x * x % p,
        4: lambda: pow(x, -1, p) if x % p else 0, 5: lambda: -x % p,
        6: lambda: 2 * x % p, 7: lambda: 4 * x % p, 8: lambda: 8 * x % p, 9: lambda: x % p,
        11: lambda: (2 * x * y - x * x) % p, 12: lambda: 3 * x * x * pow(2, -1, p) % p,
        14: lambda: x * y % p, 15: lambda: d * s % p, 16: lambda: (-x if y & 1 else x) % p,
        20: lambda: x * y % p, 21: lambda: y * s % p, 22: lambda: s * d % p, 23: lambda: d * x % p,
        24: lambda: x * y % p, 25: lambda: x * y % p,
        26: lambda: y * s % p, 27: lambda: y * s % p, 28: lambda: s * d % p,
    }[op]()


def ops_of(field):
    """every op the probe takes for the field, the four-products ops apart"""
    ops = [0, 1, 2, 3, 5, 6, 7, 8, 9]
    if field in K256_ROWS:
        ops += [11, 12, 14, 15, 16]
    return ops


def quad_ops_of(field):
    return ([20, 21, 22, 23] if field in QUAD4 else []) + ([24, 25, 26, 27, 28] if field in QUAD else [])


def refused_ops_of(field):
    taken = set(ops_of(field)) | set(quad_ops_of(field)) | (set() if field in K256_ROWS else {4})
    return [op for op in list(range(-1, 31)) + [100] if op not in taken]


# ---- how a test reaches the library ------------------------------------------------------------

def pack(vals, L):
    return np.frombuffer(b"".join(int(v).to_bytes(4 * L, "little") for v in vals), "<u4").reshape(-1, L).copy()


def unpack(arr):
    L = arr.shape[1]
    raw = np.ascontiguousarray(arr, "<u4").tobytes()
    return [int.from_bytes(raw[4 * L * i:4 * L * (i + 1)], "little") for i in range(len(arr))]


class Env:
    """lib: the hostsim build (hostsim=True: hs_field_op, one item per call), or None for libellgpu.so
    on device 0 (ellgpu_debug_field_op, one call per batch)"""

    def __init__(self, lib, hostsim):
        self.hostsim = hostsim
        self.ctx = None
        if hostsim:
            self._fn = lib.hs_field_op
            self._fn.restype = ctypes.c_int
            self._fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
            lib.hs_field_limbs.restype = ctypes.c_int
            lib.hs_field_limbs.argtypes = [ctypes.c_int]
            for f, L in LIMBS.items():
                assert lib.hs_field_limbs(f) == L, f
        else:
            import elliptic_amd
            self.ctx = elliptic_amd.Context(0)          # raises if libellgpu.so or the GPU is missing

    def close(self):
        if self.ctx is not None:
            self.ctx.close()
            self.ctx = None

    def probe(self, field, op, A, B):
        """r = a <op> b on (n, L) uint32 arrays -> (status, R); the batch is one device call"""
        A, B = np.ascontiguousarray(A, np.uint32), np.ascontiguousarray(B, np.uint32)
        out = np.zeros_like(A)
        if not self.hostsim:
            rc = self.ctx._lib.ellgpu_debug_field_op(self.ctx._ctx, field, op, A.shape[0], A.ctypes.data, B.ctypes.data,
                                                     out.ctypes.data)
            return rc, out
        step = 4 * A.shape[1]
        pa, pb, po = A.ctypes.data, B.ctypes.data, out.ctypes.data
        for i in range(A.shape[0]):
            rc = self._fn(field, op, pa + i * step, pb + i * step, po + i * step)
            if rc != 0:
                return rc, out
        return 0, out


def run(env, field, op, pairs):
    """the batch `pairs` through one probe call, every result against its integer"""
    L = LIMBS[field]
    rc, out = env.probe(field, op, pack([x for x, _ in pairs], L), pack([y for _, y in pairs], L))
    assert rc == 0, (field, op, rc)
    got = unpack(out)
    for i, ((x, y), g) in enumerate(zip(pairs, got)):
        assert g == expected(field, op, x, y), (field, op, i, len(pairs), hex(x), hex(y), hex(g))
    return len(pairs)


# ---- the operands ------------------------------------------------------------------------------

def fit(field, v):
    """v as an operand of the field: as it is where from_plain admits it, reduced otherwise"""
    return v if 0 <= v < CAP[field] else v % FIELDS[field]


def edge_pairs(field):
    """the `edge` and `rare` lists of tests/test_gpu_field.py::test_field_ops_gpu"""
    p, L = FIELDS[field], LIMBS[field]
    top = (1 << (32 * L)) - 1
    edge = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, p >> 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1,
            top % p, (top >> 1) % p, int("ffffffff00000000" * L, 16) % p, int("00000000ffffffff" * L, 16) % p]
    rt = math.isqrt(p)
    rare = [(2, (p + 1) // 2), (3, (p + 2) // 3), (rt + 1, rt + 1), (rt + 1, rt + 2), (p - 1, p - 1), (p - 1, 2),
            (1, p - 1), (p - 1, 1), (2, p - 1), (p - 2, 2), (p - 2, 3), (0, 1), (1, 2), (0, p - 1)]
    return [(edge[i], edge[(i * 7 + 3) % len(edge)]) for i in range(len(edge))] + rare


def limb_values(field):
    """values at the digit boundaries of the layer's own radix, for every digit k: 2^(w k) and its two
    neighbours, digit k all ones alone, p - 2^(w k); and every digit all ones"""
    p, w, nd = FIELDS[field], RADIX[field], DIGITS[field]
    vals = []
    for k in range(nd):
        b = 1 << (w * k)
        vals += [b, b - 1, b + 1, ((1 << w) - 1) << (w * k), (p - b) % p]
    vals.append(((1 << (w * nd)) - 1) % p)
    out = []
    for v in vals:
        v = fit(field, v)
        if v not in out:
            out.append(v)
    return out


def limb_pairs(field):
    """every boundary value beside itself, beside another boundary value (both orders), beside p - 1,
    1 and a random residue: what drives a carry across a lane and off the end of the row"""
    p = FIELDS[field]
    rnd = random.Random(2900 + field)
    vals = limb_values(field)
    out = []
    for i, v in enumerate(vals):
        o = vals[(i * 5 + 1) % len(vals)]
        out += [(v, v), (v, o), (o, v), (v, p - 1), (v, 1), (v, rnd.randrange(p)), (rnd.randrange(p), v)]
    return out


def above_p_pairs(field):
    """operands in [p, CAP): p itself and its neighbours, multiples of p, the top of the range, random"""
    p, cap = FIELDS[field], CAP[field]
    rnd = random.Random(5100 + field)
    vals = [p, p + 1, p + 2, cap - 1, cap - 2, cap >> 1, (cap >> 1) + 1, 2 * p, 2 * p + 1, 3 * p, cap - p, (cap // p) * p,
            (cap // p) * p - 1]
    if field == 5:
        vals += [2 ** 255 + 18, 2 ** 255, 2 ** 255 - 1, 2 ** 256 - 1, 2 ** 256 - 38, 2 ** 256 - 39]
    vals = [v for v in vals if p <= v < cap]
    small = [0, 1, 2, p - 1, (p + 1) // 2, 1 << RADIX[field]]
    out = [(x, y) for x in vals for y in (1, p - 1, x)] + [(y, x) for x in vals for y in small]
    out += [(vals[i], vals[(i * 3 + 1) % len(vals)]) for i in range(len(vals))]
    out += [(rnd.randrange(cap), rnd.randrange(cap)) for _ in range(100)]
    return out


def corner_pairs():
    """the `pairs` of tests/test_hostsim_golden.py::test_row_field_corners (fields 3 and 4): factors whose
    product is 0 or p exactly, near misses, products that are small multiples of 2^29, random 256-bit values"""
    p = K256_P
    rnd = random.Random(1234)
    rt = math.isqrt(p)
    pairs = [(0, 5), (5, 0), (1, p), (p, 1), (p, p), (2, (p + 1) // 2), (p - 1, p - 1), (1, 0), (rt, rt), (rt + 1, rt + 1),
             (1 << 29, 1 << 227), (1 << 128, 1 << 128), ((1 << 256) - 1, (1 << 256) - 1), (977, 1 << 29), (p - 977, 3)]
    pairs += [(1 << 29, k) for k in (1, 2, 3, 1 << 29, (1 << 58) + 1)]
    return pairs + [(rnd.getrandbits(256), rnd.getrandbits(256)) for _ in range(300)]


def directed_pairs(field):
    """the one-lane fields' directed vectors over the same prime (tests/field_vectors.py), as operand
    pairs: every op of this module runs on them, the one they were built for among them"""
    if field in K256_ROWS:
        vecs = [v for v in field_vectors.rare_vectors() + field_vectors.shift_vectors() + field_vectors.fold_vectors()
                if v[0] == 0]
        return [(v[2], v[3]) for v in vecs] + corner_pairs()
    if field == 5:
        vecs = [v for v in field_vectors.rare_vectors() + field_vectors.fold25519_vectors() + field_vectors.shift_vectors()
                if v[0] == 1 and v[1] != 10]
        return [(v[2], v[3]) for v in vecs]
    return []


def random_pairs(field, n, seed):
    p = FIELDS[field]
    rnd = random.Random(seed + field)
    return [(rnd.randrange(p), rnd.randrange(p)) for _ in range(n)]


_LISTS = {}


def main_pairs(field):
    """the operand list of a field: edge, digit boundaries, directed, above p, 1500 random pairs.  Field 4
    gets its list shuffled (a wave's four rows then hold unrelated operands, directed vectors beside
    random ones) at a length = 1 (mod 4): the last wave has one item and three empty rows"""
    if field not in _LISTS:
        pairs = (edge_pairs(field) + limb_pairs(field) + directed_pairs(field) + above_p_pairs(field)
                 + random_pairs(field, 1500, 4242))
        for x, y in pairs:
            assert 0 <= x < CAP[field] and 0 <= y < CAP[field], (field, hex(x), hex(y))
        if field == 4:
            random.Random(404).shuffle(pairs)
            pairs += random_pairs(field, (1 - len(pairs)) % 4, 99)
            assert len(pairs) % 4 == 1
        _LISTS[field] = pairs
    return _LISTS[field]


def quad_pairs(field):
    """edge, digit-boundary and 300 random pairs for the four-products ops"""
    return edge_pairs(field) + limb_pairs(field) + random_pairs(field, 300, 777)


def inv_values(field):
    """the `inv_in` list of test_field_ops_gpu: edge values, powers of two, long zero runs, random"""
    p = FIELDS[field]
    rnd = random.Random(4242 + field)
    vals = [0, 1, 2, 3, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << 30, (1 << 30) - 1, (1 << 60) + 1, p >> 1]
    vals += [(1 << k) % p for k in range(1, p.bit_length(), 29)]
    vals += [((rnd.randrange(p) >> k) << k) % p for k in (1, 17, 30, 31, 61, 90)]
    vals += [p, p + 1, CAP[field] - 1]
    return vals + [rnd.randrange(p) for _ in range(30)]


def coverage(field, pairs):
    """how many pairs of the list fall into each class the checks need (integers only)"""
    p, w = FIELDS[field], RADIX[field]
    c = dict(sum_below_p=0, sum_wraps=0, diff_nonneg=0, diff_neg=0, zero_product=0, low_digit_zero=0)
    for x, y in pairs:
        if x < p and y < p:
            c["sum_below_p" if x + y < p else "sum_wraps"] += 1
            c["diff_nonneg" if x >= y else "diff_neg"] += 1
        if x and y and x * y % p == 0:
            c["zero_product"] += 1                          # (needs an operand above p: p is prime)
        if x and y and x * y % (1 << w) == 0:
            c["low_digit_zero"] += 1
    return c


def check_coverage(field):
    c = coverage(field, main_pairs(field))
    assert all(n >= 1 for n in c.values()), (field, c)
    cq = coverage(field, quad_pairs(field))
    assert all(cq[k] >= 1 for k in ("sum_below_p", "sum_wraps", "diff_nonneg", "diff_neg", "low_digit_zero")), (field, cq)
    return c


# ---- the checks --------------------------------------------------------------------------------

def check_ops(env, field):
    """every op of the field on its whole list; the one-item-per-wave fields also on one item alone"""
    pairs = main_pairs(field)
    total = 0
    for op in ops_of(field):
        total += run(env, field, op, pairs)
        if field != 4:
            run(env, field, op, pairs[3:4])
    return total


def check_inversion(env, field):
    vals = inv_values(field)
    n = run(env, field, 4, [(v, v) for v in vals])
    run(env, field, 4, [(vals[5], 0)])
    return n


def check_quad(env, field):
    """mulq over pack4 / pack2 / pack3, each row read back through unpack*"""
    pairs = quad_pairs(field)
    total = 0
    for op in quad_ops_of(field):
        total += run(env, field, op, pairs)
        run(env, field, op, pairs[20:21])
    return total


def check_ragged(env, n):
    """field 4 with n items: a last (or only) wave with empty rows"""
    pairs = main_pairs(4)
    for k, op in enumerate(ops_of(4)):
        run(env, 4, op, pairs[7 * k:7 * k + n])
    return n


def check_neighbour_rows(env):
    """field 4: three rows of every wave hold fixed operands (0, p - 1, 2^256 - 1), the fourth walks a list;
    then the walking row rotates.  A result that depends on the row beside it differs from its integer"""
    p = K256_P
    fixed = [(0, p - 1), (p - 1, (1 << 256) - 1), ((1 << 256) - 1, 0)]
    walk = edge_pairs(4) + limb_pairs(4)[::3] + corner_pairs()[:20] + random_pairs(4, 60, 31)
    total = 0
    for rot in range(4):
        batch = []
        for pr in walk:
            wave = list(fixed)
            wave.insert(rot, pr)
            batch += wave
        for op in ops_of(4):
            total += run(env, 4, op, batch)
    return total


def check_refusals(env):
    """an op a field does not take is refused, and nothing is written"""
    for field in sorted(FIELDS):
        L = LIMBS[field]
        A = pack([3, 5], L)
        for op in refused_ops_of(field):
            rc, out = env.probe(field, op, A, A)
            assert rc != 0 and not out.any(), (field, op, rc)
