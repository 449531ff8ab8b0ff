"""FpK256's pair products (mul_sub_mul, mul_sub_sqr: a difference of two wide products, folded once)
and the secp256k1 group law built on them, on the CPU build of the device headers
(tests/hostsim/k256_pair_probe.cpp), against Python integers and the Python oracle's affine
group law."""
import ctypes
import hashlib
import itertools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import ec_oracle as O  # noqa: E402

P = 2 ** 256 - 2 ** 32 - 977
DELTA = 2 ** 32 + 977
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
M32 = 2 ** 32 - 1


def build_probe():
    src = os.path.join(HERE, "hostsim", "k256_pair_probe.cpp")
    cs = os.path.join(ROOT, "elliptic_amd", "csrc")
    out = os.path.join(HERE, "hostsim", "_build")
    os.makedirs(out, exist_ok=True)
    h = hashlib.sha256()
    for f in [src] + sorted(os.path.join(cs, f) for f in os.listdir(cs) if f.endswith(".h")):
        with open(f, "rb") as fh:
            h.update(fh.read())
    lib = os.path.join(out, "libk256_pair_probe.so")
    stamp = os.path.join(out, "stamp_k256_pair_probe")
    if not (os.path.exists(lib) and os.path.exists(stamp) and open(stamp).read() == h.hexdigest()):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fno-strict-aliasing", "-o", lib, src],
                       check=True)
        with open(stamp, "w") as f:
            f.write(h.hexdigest())
    return lib


@pytest.fixture(scope="module")
def lib():
    l = ctypes.CDLL(build_probe())
    u32p = ctypes.POINTER(ctypes.c_uint32)
    l.kp_field_op.argtypes = [ctypes.c_int, ctypes.c_size_t, u32p, u32p, u32p, u32p, u32p]
    l.kp_dbl.argtypes = [ctypes.c_size_t, u32p, u32p]
    l.kp_add_mixed.argtypes = [ctypes.c_int, ctypes.c_size_t, u32p, u32p, ctypes.POINTER(ctypes.c_ubyte), u32p, u32p]
    # the default build takes the pair form in the addition and in the doubling
    assert l.kp_config() == 3
    return l


def words(vals, per=1):
    """rows of `per` field elements -> uint32 array (rows, 8 * per), little-endian words"""
    a = np.zeros((len(vals), 8 * per), np.uint32)
    for i, row in enumerate(vals):
        row = row if per > 1 else (row,)
        for j, v in enumerate(row):
            assert 0 <= v < P
            for k in range(8):
                a[i, 8 * j + k] = (v >> (32 * k)) & M32
    return a


def ints(arr, per=1):
    out = []
    for row in arr:
        vs = [sum(int(row[8 * j + k]) << (32 * k) for k in range(8)) for j in range(per)]
        out.append(vs[0] if per == 1 else tuple(vs))
    return out


def ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def field_op(lib, op, quads):
    a, b, c, d = (words([q[i] for q in quads]) for i in range(4))
    r = np.zeros_like(a)
    assert lib.kp_field_op(op, len(quads), ptr(a), ptr(b), ptr(c), ptr(d), ptr(r)) == 0
    return ints(r)


def check_pairs(lib, quads):
    got = field_op(lib, 0, quads)
    sep = field_op(lib, 3, quads)
    got2 = field_op(lib, 1, quads)
    sep2 = field_op(lib, 4, quads)
    for i, (a, b, c, d) in enumerate(quads):
        want = (a * b - c * d) % P
        assert got[i] == want, ("mul_sub_mul", hex(a), hex(b), hex(c), hex(d), hex(got[i]))
        assert sep[i] == want
        want2 = (a * b - c * c) % P
        assert got2[i] == want2, ("mul_sub_sqr", hex(a), hex(b), hex(c), hex(got2[i]))
        assert sep2[i] == want2


# the 512-bit value the pair product hands to the fold: a b - c d, plus p 2^256 where that is negative
def folded_value(a, b, c, d):
    v = a * b - c * d
    return v + (P << 256) if v < 0 else v


def word(v, i):
    return (v >> (32 * i)) & M32


EDGES = [0, 1, 2, P - 1, P - 2, 2 ** 255, 2 ** 256 - 2 ** 32 - 978, BETA,
         2 ** 256 - 2 ** 33,                   # words 2..7 all ones
         P - 2 ** 32,                          # words 1..7: fffffffd, ffffffff ...
         2 ** 256 - 2 ** 32 - 2 ** 31]         # words 2..7 all ones, word 1 = fffffffe, word 0 = 2^31


def test_every_combination_of_the_edge_values(lib):
    quads = list(itertools.product(EDGES, repeat=4))
    assert len(quads) == len(EDGES) ** 4
    check_pairs(lib, quads)
    vals = [folded_value(*q) for q in quads]
    assert all(0 <= v < (P << 256) for v in vals)          # the bound written above reduce_wide_diff
    # the first fold's multiply-add overflows (fold4's carry-out path) when a high word reaches 2^32 - 977
    assert sum(1 for v in vals if any(word(v, 8 + i) >= 2 ** 32 - 977 for i in range(8))) > 1000
    # in the additive form a b + (p - c) d these reach 2^512, a seventeenth word; here they do not exist
    assert sum(1 for (a, b, c, d) in quads if a * b + (P - c) * d >= 2 ** 512) > 100


def test_equal_smaller_and_larger_products(lib):
    rnd = random.Random(1901)
    quads = []
    for _ in range(300):
        x, y = rnd.randrange(P), rnd.randrange(P)
        quads.append((x, y, y, x))                            # a b = c d
        lo, hi = sorted((x, y))
        z = rnd.randrange(P)
        if lo != hi and z:
            quads.append((lo, z, hi, z))                      # a b < c d
            quads.append((hi, z, lo, z))                      # a b > c d
        if y:
            quads.append((x, y, x, y - 1))                    # by one multiple of x
            quads.append((x, y - 1, x, y))
    quads += [(0, 0, 1, 1), (1, 1, 0, 0), (0, 5, P - 1, P - 1), (P - 1, P - 1, P - 1, P - 1), (P - 1, P - 1, 0, 0),
              (P - 1, P - 2, P - 1, P - 1), (P - 1, P - 1, P - 1, P - 2)]
    assert any(a * b == c * d for a, b, c, d in quads)
    assert any(a * b < c * d for a, b, c, d in quads) and any(a * b > c * d for a, b, c, d in quads)
    check_pairs(lib, quads)


def test_carry_out_and_borrow_ripple_paths(lib):
    quads = []
    # (1) high words of the folded value at 2^32 - 977 and above, positive and negative differences:
    # a b (c d) just below a chosen 512-bit target T with all-ones / boundary words
    rnd = random.Random(1902)
    targets = []
    for w in (2 ** 32 - 977, 2 ** 32 - 976, 2 ** 32 - 1, 2 ** 32 - 978):
        for pos in range(8, 16):
            hi = [rnd.getrandbits(32) for _ in range(16)]
            hi[pos] = w
            hi[15] = min(hi[15], 0xFFFFFFF0) if pos != 15 else w
            targets.append(sum(x << (32 * i) for i, x in enumerate(hi)))
    for T in targets:
        if T >= (P - 1) ** 2:
            T = (P - 1) ** 2 - rnd.getrandbits(200)
        a = P - 1 - rnd.getrandbits(64)
        b = T // a
        if b >= P:
            continue
        quads.append((a, b, 0, 0))                            # folded value a b: T minus less than 2^256
        # negative: c d - a' b' = p 2^256 - T', so that the folded value is T' near T
        m = (P << 256) - T
        if 0 < m <= (P - 1) ** 2:
            c = P - 1 - rnd.getrandbits(64)
            d = m // c
            if d < P:
                quads.append((0, 0, c, d))
    n_carry = sum(1 for q in quads if any(word(folded_value(*q), 8 + i) >= 2 ** 32 - 977 for i in range(8)))
    assert n_carry >= 40
    # (2) the borrow out of word 9 when delta comes off a negative difference: the words of
    # 2^512 + (a b - c d) have word 9 = 0, or word 9 = 1 and word 8 < 977
    c = d = P - 1
    K = 2 ** 512 - c * d
    ripple = []
    for j in (1, 2, 0xFFFFFFFF, 2 ** 64 + 1, 2 ** 160):       # X = 2^320 j + r, r < 2^288: word 9 = 0
        for abits in (161, 200, 255):
            a = (1 << abits) + rnd.getrandbits(abits - 1)
            b = -(-((j << 320) - K) // a)
            if 0 < b < P:
                ripple.append((a, b, c, d))
    for j in (1, 3):                                          # X = 2^320 j + 2^288 + r, r < 2^256: word 9 = 1, word 8 = 0
        a = (1 << 100) + rnd.getrandbits(99)
        b = -(-((j << 320) + (1 << 288) - K) // a)
        ripple.append((a, b, c, d))
    hit = 0
    for (a, b, c, d) in ripple:
        assert a * b < c * d
        X = 2 ** 512 + a * b - c * d
        if word(X, 9) * 2 ** 32 + word(X, 8) < DELTA:
            hit += 1
    assert hit >= 10
    check_pairs(lib, quads + ripple)


def test_random_quadruples(lib):
    rnd = random.Random(1903)
    check_pairs(lib, [tuple(rnd.randrange(P) for _ in range(4)) for _ in range(10000)])


def test_half(lib):
    rnd = random.Random(1904)
    vals = EDGES + [3, 5, 2 ** 32 + 1, 2 ** 32 + 3, 2 ** 64 + 1, 2 ** 33 - 1, 0x100000001, 2 ** 224 + 1, P - 3]
    vals += [rnd.randrange(P) for _ in range(2000)]
    got = field_op(lib, 2, [(v, 0, 0, 0) for v in vals])
    inv2 = (P + 1) // 2
    for v, g in zip(vals, got):
        assert g == v * inv2 % P, hex(v)


# ---- group law ---------------------------------------------------------------------------------

def curve():
    return O.get_curve("secp256k1", False)


def jac_of(pt, z):
    return (pt.x * z * z % P, pt.y * z * z * z % P, z)


def affine_of(j):
    X, Y, Z = j
    if Z == 0:
        return None
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


@pytest.fixture(scope="module")
def points():
    """random affine points k G, computed once"""
    cur = curve()
    rnd = random.Random(1905)
    pts = []
    acc = cur.g.mul(rnd.randrange(1, cur.n))
    step = cur.g.mul(rnd.randrange(1, cur.n))
    for _ in range(120):
        acc = acc.add(step)
        pts.append(acc)
    return pts


def run_dbl(lib, jacs):
    p = words(jacs, 3)
    out = np.zeros_like(p)
    lib.kp_dbl(len(jacs), ptr(p), ptr(out))
    return ints(out, 3)


def run_add(lib, form, jacs, qs, pinf=None):
    p = words(jacs, 3)
    q = words(qs, 2)
    inf = np.array(pinf if pinf is not None else [0] * len(jacs), np.uint8)
    h = np.zeros((len(jacs), 8), np.uint32)
    out = np.zeros_like(p)
    assert lib.kp_add_mixed(form, len(jacs), ptr(p), ptr(q), inf.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
                            ptr(h), ptr(out)) == 0
    return ints(out, 3), inf.tolist(), ints(h)


def test_doubling_on_random_points(lib, points):
    rnd = random.Random(1906)
    zs = [1, 2, P - 1] + [rnd.randrange(1, P) for _ in range(len(points) - 3)]
    got = run_dbl(lib, [jac_of(pt, z) for pt, z in zip(points, zs)])
    for pt, z, g in zip(points, zs, got):
        assert affine_of(g) == pt.dbl().xy()
        assert g[2] == pt.y * z % P * z * z % P * z % P      # Z3 = Y Z: the triple of the 1/2-scaled formulas


def test_doubling_of_o_and_of_y_zero(lib, points):
    pt = points[0]
    got = run_dbl(lib, [(pt.x, pt.y, 0), (1, 1, 0), (5, 0, 7), (0, 0, 1)])
    assert all(g[2] == 0 for g in got)


@pytest.mark.parametrize("form", [0, 1, 2])
def test_mixed_addition_on_random_points(lib, points, form):
    rnd = random.Random(1907 + form)
    half = len(points) // 2
    ps, qs = points[:half], points[half:2 * half]
    zs = [1, P - 1] + [rnd.randrange(1, P) for _ in range(half - 2)]
    jacs = [jac_of(pt, z) for pt, z in zip(ps, zs)]
    got, inf, h = run_add(lib, form, jacs, [q.xy() for q in qs])
    for pt, q, j, g, f, hh in zip(ps, qs, jacs, got, inf, h):
        assert affine_of(g) == pt.add(q).xy()
        assert f == 0
        if form == 2:
            assert g[2] == j[2] * hh % P


@pytest.mark.parametrize("form", [0, 1])
def test_mixed_addition_exceptional_inputs(lib, points, form):
    rnd = random.Random(1909)
    cases = []                                               # (P as Jacobian, "P is O", Q, expected affine)
    for q in points[:12]:
        z = rnd.randrange(1, P)
        cases.append(((1, 1, 0), 1, q, q.xy()))                         # O + Q
        cases.append(((q.x, q.y, 0), 1, q, q.xy()))                     # O with other coordinates
        cases.append((jac_of(q, z), 0, q, q.dbl().xy()))                # P = Q
        cases.append((jac_of(q, 1), 0, q, q.dbl().xy()))
        cases.append((jac_of(q.neg(), z), 0, q, None))                  # P = -Q
        cases.append((jac_of(q.neg(), 1), 0, q, None))
    got, inf, _ = run_add(lib, form, [c[0] for c in cases], [c[2].xy() for c in cases], [c[1] for c in cases])
    for c, g, f in zip(cases, got, inf):
        assert affine_of(g) == c[3], c
        if form == 0:
            assert f == (1 if c[3] is None else 0)
