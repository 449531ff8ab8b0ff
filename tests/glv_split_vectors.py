"""The integer model of secp256k1's GLV split (csrc/ladder.h: glv_split, its ROT form) and the
scalars that the split's tests run: shared by test_glv_split_bound.py (CPU build of the headers) and
test_gpu_glv_split.py.

The model follows the device code step by step: the multiply-shift rounding with the constants of
curve_consts.h, the reduction by the lattice basis v1 = (a1, -|b1|), v2 = (a2, b2), and then the
choice that makes both halves odd: a translation by -+v1 where both are even, a multiplication of
z = k1 + k2 lambda by the unit lambda or lambda^2 where one is, with P replaced by lambda^2 P or
lambda P.  Its claim, proven above glv_split: both halves odd and below 2^128 for every k < 2^256."""
import random

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
P = 2 ** 256 - 2 ** 32 - 977
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
A1 = 0x3086D221A7D46BCDE86C90E49284EB15
MB1 = 0xE4437ED6010E88286F547FA90ABFE4C3          # |b1|, b1 < 0
A2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8
B2 = A1
G1 = ((B2 << 384) * 2 + N) // (2 * N)              # round(2^384 b2 / n)
G2 = ((MB1 << 384) * 2 + N) // (2 * N)             # round(2^384 |b1| / n)
BOUND = 1 << 128


def reduce(k):
    """(k1, k2) = (k, 0) - c1 v1 - c2 v2, c_i the multiply-shift roundings"""
    c1 = (k * G1 + (1 << 383)) >> 384
    c2 = (k * G2 + (1 << 383)) >> 384
    return k - c1 * A1 - c2 * A2, c1 * MB1 - c2 * B2


def split_rot(k):
    """-> (k1, k2, rot): both odd, k == (k1 + k2 lambda) lambda^rot (mod n), the ladder's point is
    lambda^rot P = (beta^rot x, y)"""
    k1, k2 = reduce(k)
    if k1 % 2 == 0 and k2 % 2 == 0:
        if k2 >= 0:
            return k1 + A1, k2 - MB1, 0
        return k1 - A1, k2 + MB1, 0
    if k2 % 2 == 0:
        return k2 - k1, -k1, 1
    if k1 % 2 == 0:
        return -k2, k1 - k2, 2
    return k1, k2, 0


def check(k):
    """the model's claims for one scalar; -> (|k1|, |k2|)"""
    k1, k2, rot = split_rot(k)
    assert k1 & 1 and k2 & 1, hex(k)
    assert abs(k1) < BOUND and abs(k2) < BOUND, hex(k)
    assert ((k1 + k2 * LAMBDA) * pow(LAMBDA, rot, N) - k) % N == 0, hex(k)
    return abs(k1), abs(k2)


def edge_scalars():
    return [0, 1, 2, N - 1, N, N + 1, 2 ** 256 - 1, LAMBDA]


def boundary_scalars():
    """k whose coordinates in the lattice basis lie next to the rounding boundaries -- half-integer
    t1, t2, the corners and edge midpoints of the reduced parallelogram, where |k1|, |k2| and
    |k1 - k2| are largest -- and next to the lattice points themselves (reduced pair near (0, 0))"""
    out = []
    for m1 in (-3, -2, -1, 0, 1, 2, 3):
        for m2 in (-3, -2, -1, 0, 1, 2, 3):
            # (m1 v1 + m2 v2) / 2, rounded, and its neighbours
            x = (m1 * A1 + m2 * A2) // 2
            y = (-m1 * MB1 + m2 * B2) // 2
            for dx in (-2, -1, 0, 1, 2):
                for dy in (-1, 0, 1):
                    out.append(((x + dx) + (y + dy) * LAMBDA) % N)
    return out


def half_scalars():
    """k = k1 + k2 lambda mod n for halves on +-(2^128 - 1), +-2^127, 0 and +-1"""
    hs = [BOUND - 1, -(BOUND - 1), 1 << 127, -(1 << 127), 0, 1, -1]
    return [(a + b * LAMBDA) % N for a in hs for b in hs]


def engine_scalars(n_random=2048, seed=20):
    """the scalars of the engine tests, in a fixed order, without repeats"""
    rnd = random.Random(seed)
    ks = edge_scalars() + half_scalars() + boundary_scalars()
    ks += [rnd.getrandbits(256) for _ in range(n_random)]
    seen, out = set(), []
    for k in ks:
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out



_cases = None


def engine_cases():
    """Inputs and the C oracle's results for the engine tests, computed once: P*k for every scalar
    of engine_scalars() over points d*G, and ECDSA tuples built so that u2 = s^-1 r IS the scalar
    (R = u1 G + u2 Q from the oracle, r = x(R) mod n, s = r / u2, z = u1 s), every fifth with a
    flipped digest bit."""
    global _cases
    if _cases is not None:
        return _cases
    import numpy as np
    from elliptic_amd import ints_to_be
    from oracle import c_oracle
    curve = "secp256k1"
    rnd = random.Random(21)
    ks = engine_scalars()
    m = len(ks)
    keys, kinf = c_oracle.mul(curve, ints_to_be([rnd.randrange(1, N) for _ in range(m)], 32))
    assert not kinf.any()
    k = ints_to_be(ks, 32)
    want_xy, want_inf = c_oracle.mul(curve, k, keys)
    # verify tuples for the scalars that can be a u2 (non-zero mod n; u2 arrives reduced)
    idx = [i for i in range(m) if ks[i] % N != 0 and (ks[i] < N or ks[i] - N not in ks[:i])]
    u2 = [ks[i] % N for i in idx]
    u1 = [rnd.randrange(N) for _ in idx]
    pub = np.ascontiguousarray(keys[idx])
    rxy, rinf = c_oracle.mul_add(curve, ints_to_be(u1, 32), None, ints_to_be(u2, 32), pub)
    zs, rs, ss = [], [], []
    for j in range(len(idx)):
        r = int.from_bytes(rxy[j, :32].tobytes(), "big") % N
        if rinf[j] or r == 0:
            r = 1
        s = r * pow(u2[j], -1, N) % N
        z = u1[j] * s % N
        if j % 5 == 4:
            z ^= 1
        zs.append(z); rs.append(r); ss.append(s)
    z, r, s = ints_to_be(zs, 32), ints_to_be(rs, 32), ints_to_be(ss, 32)
    want_ok = np.asarray(c_oracle.verify(curve, z, r, s, pub), np.uint8)
    assert int(want_ok.sum()) > len(idx) * 3 // 4 and int((want_ok == 0).sum()) > len(idx) // 8
    _cases = dict(k=k, pts=keys, want_xy=want_xy, want_inf=np.asarray(want_inf, np.uint8),
                  z=z, r=r, s=s, pub=pub, want_ok=want_ok)
    return _cases
