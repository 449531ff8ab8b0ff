"""The shared-inversion kernels with more than one item per inversion: the cases, shared by the
hostsim and the device runner (test_inv_batch_hostsim.py, test_inv_batch_gpu.py).

Fifteen device routines invert once for K items (Montgomery's trick): thread t of T = ceil(n / K)
owns the items t, t + T, t + 2 T, ... and has to replace a zero or refused element by one on the way
up and again on the way down.  K comes from Engine::norm_batch_for / inv_batch_for /
inv_batch_beside, which give 1 below 65 536 items, so the batches of the other suites run every one
of these routines as an inversion of a single element.  ELLGPU_NORM_K and ELLGPU_PREP_K (read when a
context is created) force K; here they are forced on batches of a few items up to 64 K + 37.

A case is one call on one curve (CASES, one row per call; `routines` names the device routines the
row is there for, `kernels` the launches that have to be seen).  Its items come from a small pool:
inputs and the expected outputs, by the integer models and oracles the other suites use
(fixed_base_checks.Model, verify_base_checks.Domain, oracle/ec_oracle.py, custom_*_checks), each item
labelled refused (a zero, an infinity, a status other than 0) or ordinary.  compose() lays pool
items out over a batch of n items by a mask, placement() makes the mask per thread group {t, t + T,
...}: first only, last only, one in the middle, two adjacent, all but one, all, none -- a pattern
per group, rotated over the groups, so that the groups of the tail (fewer than K items) get theirs
too.  Every batch is run in a forced context and in the K = 1 context; the bytes have to be the
same, and the pool's.  Result buffers are filled with 0xA5 before each call (the run_* helpers of
the suites this one borrows from do that).

Memory kinds: "dev_np" (the _dev entry points on the hostsim build, where device memory is host
memory) and "dev_torch" (device tensors).  The device forms launch a batch whole, so T is the T of
placement(); the host forms of the CPU build would cut it into chunks of eight."""
import os
import random
import re

import numpy as np

import custom_ecdh_checks as CH
import custom_ed_checks as CE
import custom_ed_ecdsa_checks as CEE
import custom_mont_checks as CM
import custom_recover_checks as CR
import custom_sign_checks as CS
import custom_wire_checks as CW
import fixed_base_checks as FB
import fixed_base_ed_checks as FBE
import verify_base_checks as VB

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "elliptic_amd", "csrc")
FILL = FB.FILL
I = FB.I
PRESETS = FB.PRESETS
REFERENCE_K = (1, 1)
DEVICE_KS = [(16, 8), (3, 3)]                  # (ELLGPU_NORM_K, ELLGPU_PREP_K): the production maxima, and odd
HOST_KS = DEVICE_KS + [(64, 64), (2, 2)]
# the lanes-per-item forms invert per item and would take small batches away from these kernels
ONE_LANE = {"ELLGPU_COOP_GRID": "0", "ELLGPU_WIDE_GRID": "0", "ELLGPU_ROW_GRID": "0", "ELLGPU_PARTED_GRID": "0"}
PATTERNS = ("first", "last", "middle", "adjacent", "all_but_one", "all", "none")
_cache = {}


# ---- contexts -------------------------------------------------------------------------------

def make_context(monkeypatch, ks, comb_max_bytes=0, **kw):
    """a context whose shared inversions take ks = (NORM_K, PREP_K) items and whose batches all run
    one item per lane; the environment is as it was afterwards (the overrides are read once).
    comb_max_bytes: ELLGPU_COMB_MAX_BYTES, so that the 256-bit curves' own tables are built at 16 bits
    (36 MB) and not at 22 (1.6 GB each, in every context): the table width is not under test here"""
    import elliptic_amd
    env = dict(ONE_LANE, ELLGPU_NORM_K=str(ks[0]), ELLGPU_PREP_K=str(ks[1]))
    if comb_max_bytes:
        env["ELLGPU_COMB_MAX_BYTES"] = str(comb_max_bytes)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        ctx = elliptic_amd.Context(0, **kw)
    finally:
        for k in env:
            monkeypatch.delenv(k)
    ctx.inv_ks = ks
    ctx.inv_handles = {}
    return ctx


# ---- where the refused items go ---------------------------------------------------------------

def sizes_of(K):
    """n < K (one thread, cnt < K), exact multiples, one thread with one item more, a wave of threads
    with an uneven tail"""
    return sorted({n for n in (1, K - 1, K, K + 1, 2 * K + 1, 64 * K + 37) if n > 0})


def groups_of(n, K):
    """the items of every thread: T = ceil(n / K) lists"""
    T = (n + K - 1) // K
    return [list(range(t, n, T)) for t in range(T)]


def rotations_of(n, K):
    """how many placements a size needs for every pattern to occur: one where there are seven groups"""
    return 1 if (n + K - 1) // K >= len(PATTERNS) else len(PATTERNS)


def pattern_positions(pattern, cnt, t):
    """positions within a group of cnt items"""
    mid = cnt // 2
    return {"first": {0}, "last": {cnt - 1}, "middle": {mid}, "adjacent": {max(0, mid - 1), mid},
            "all_but_one": set(range(cnt)) - {t % cnt}, "all": set(range(cnt)), "none": set()}[pattern]


def placement(n, K, rot=0):
    """-> (mask (n,) bool: refused here, [(pattern, cnt) per group])"""
    mask = np.zeros(n, bool)
    plan = []
    for t, g in enumerate(groups_of(n, K)):
        assert 0 < len(g) <= K
        pat = PATTERNS[(t + rot) % len(PATTERNS)]
        for j in pattern_positions(pat, len(g), t):
            mask[g[j]] = True
        plan.append((pat, len(g)))
    return mask, plan


# ---- pools and batches ------------------------------------------------------------------------

class Pool:
    """ins / outs: lists of arrays with one row per pool item; refused: (m,) bool"""

    def __init__(self, ins, outs, refused):
        self.ins = [np.ascontiguousarray(a) for a in ins]
        self.outs = [np.ascontiguousarray(a) for a in outs]
        self.refused = np.asarray(refused, bool)
        m = len(self.refused)
        assert all(a.shape[0] == m for a in self.ins + self.outs)
        assert self.refused.any() and not self.refused.all(), "a pool needs both kinds"
        for a in self.ins + self.outs:
            a.setflags(write=False)


def compose(pool, mask):
    """-> (inputs, expected outputs) of a batch: refused pool items where mask says so, ordinary ones
    elsewhere, each kind taken in turn"""
    ref, ordn = np.nonzero(pool.refused)[0], np.nonzero(~pool.refused)[0]
    idx = np.empty(len(mask), np.int64)
    idx[mask] = ref[np.arange(mask.sum()) % len(ref)]
    idx[~mask] = ordn[np.arange((~mask).sum()) % len(ordn)]
    return [a[idx] for a in pool.ins], [a[idx] for a in pool.outs]


def _rows(vals, B):
    return FB.rows(vals, B)


def _tile(row, m):
    return np.tile(np.frombuffer(bytes(row), np.uint8), (m, 1))


def _pts(answers):
    return np.stack([a[0] for a in answers]), np.array([a[1] for a in answers], np.uint8)


def _draws(rng, order, bits, m):
    """m scalars: below the order, and one in four of the full operand width"""
    return [rng.getrandbits(bits) if i % 4 == 3 else rng.randrange(2, order) for i in range(m)]


# the calls of the presets, in the two device forms (the other suites' run_* helpers cover the rest)

def _dev_call(ctx, form, name, args, out_shapes):
    """ellgpu_<name>_dev(ctx, *args, *results, stream): integers and None as they are, arrays by
    address; the results are filled with 0xA5 first"""
    outs = [np.full(sh, FILL, np.uint8) for sh in out_shapes]
    if form == "dev_np":
        ptr = [a.ctypes.data if isinstance(a, np.ndarray) else a for a in list(args) + outs]
        CW._raw(ctx, getattr(ctx._lib, "ellgpu_" + name + "_dev")(ctx._ctx, *ptr, None))
        return outs
    assert form == "dev_torch"
    import torch
    dev = [torch.from_numpy(a).cuda() if isinstance(a, np.ndarray) else a for a in list(args) + outs]
    ctx._call(name, True, *dev)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in dev[len(args):]]


def _cid(curve):
    from elliptic_amd.engine import CURVE_ID
    return CURVE_ID[curve] if isinstance(curve, str) else int(curve)


def _c(a):
    return np.ascontiguousarray(a, np.uint8)


def run_mul_var(ctx, curve, B, ins, form):
    k, xy = map(_c, ins)
    return _dev_call(ctx, form, "mul_var", [_cid(curve), len(k), k, xy], [(len(k), 2 * B), (len(k),)])


def run_mul_fixed(ctx, curve, B, ins, form):
    k = _c(ins[0])
    return _dev_call(ctx, form, "mul_fixed", [_cid(curve), len(k), k], [(len(k), 2 * B), (len(k),)])


def run_mul_add2(ctx, curve, B, ins, form):
    k1, p1, k2, p2 = map(_c, ins)
    return _dev_call(ctx, form, "mul_add2", [_cid(curve), len(k1), k1, p1, k2, p2], [(len(k1), 2 * B), (len(k1),)])


def run_x25519(ctx, ins, form):
    k, x = map(_c, ins)
    return _dev_call(ctx, form, "x25519_ladder", [len(k), k, x], [(len(k), 32), (len(k),)])


def run_verify(ctx, curve, ins, form):
    h, r, s, pub = map(_c, ins)
    return _dev_call(ctx, form, "ecdsa_verify", [_cid(curve), len(h), h, h.shape[1], 0, r, s, pub], [(len(h),), (len(h),)])


def run_recover(ctx, curve, B, ins, form):
    h, r, s, j = map(_c, ins)
    return _dev_call(ctx, form, "ecdsa_recover", [_cid(curve), len(h), h, h.shape[1], r, s, j], [(len(h), 2 * B), (len(h),)])


def run_sign(ctx, curve, NB, ins, form):
    h, d, k = map(_c, ins)
    n = len(h)
    return _dev_call(ctx, form, "ecdsa_sign", [_cid(curve), n, h, h.shape[1], 0, d, k, 0], [(n, NB), (n, NB), (n,), (n,)])


# ---- the pools ----------------------------------------------------------------------------------

def _short_pool(name, op):
    """Work::normalize on a preset: results at O beside ordinary ones -- k = 0, k = n, 2 n where the
    operand holds it; k G + k (-G)"""
    spec = FB.spec_of(name)
    m, B, pts, order = FB.model_of(spec), spec["B"], FB.bases_of(spec), I(spec["n"])
    bits = 8 * B
    rng = random.Random("inv-batch:%s:%s" % (name, op))
    if op == "mul_add2":
        k1 = _draws(rng, order, bits, 10) + [0, 5, order, order - 1, rng.randrange(order)]
        k2 = _draws(rng, order, bits, 10) + [0, 5, 0, order - 1]
        k2.append(k1[-1])
        res = m.mul_many(k2, pts[2], bits, m.mul_many(k1, pts[0], bits))
        xy, inf = _pts([FB.answer(R, B) for R in res])
        g, ng = FB.xy_bytes(pts[0], B), FB.xy_bytes(pts[2], B)
        return Pool([_rows(k1, B), _tile(g, 15), _rows(k2, B), _tile(ng, 15)], [xy, inf], inf == 1)
    P = pts[0] if op == "mul_fixed" else pts[3]
    ks = _draws(rng, order, bits, 10) + [0, order] + ([2 * order] if 2 * order < 1 << bits else [])
    xy, inf = _pts([FB.answer(R, B) for R in m.mul_many(ks, P, bits)])
    assert inf[10:].all() and not inf[:10].any()
    if op == "mul_fixed":
        return Pool([_rows(ks, B)], [xy, inf], inf == 1)
    return Pool([_rows(ks, B), _tile(FB.xy_bytes(P, B), len(ks))], [xy, inf], inf == 1)


def _edwards_pool(name, op):
    """EdWork::normalize / edcustom.h normalize: the identity and the point of order two among the
    results (Z is never 0 on a complete curve: what counts is that the neighbours are right)"""
    spec = FBE.spec_of(name)
    m, pts, order, p = FBE.model_of(spec), FBE.bases_of(spec), I(spec["n"]), I(spec["p"])
    rng = random.Random("inv-batch:%s:%s" % (name, op))
    two = (0, p - 1)
    assert m.add(two, two) == m.ID and m.mul(order, pts[3]) == m.ID
    if op == "mul_add2":
        a = rng.randrange(2, order)
        items = [(k1, pts[0], k2, pts[3]) for k1, k2 in zip(_draws(rng, order, 256, 8), _draws(rng, order, 256, 8))]
        special = [(a, pts[0], a, pts[2]), (0, pts[0], 0, pts[3]), (1, two, 0, pts[0]), (order, pts[0], 2, two)]
        res = [m.mul2(k1, P1, k2, P2) for k1, P1, k2, P2 in items + special]
        assert res[8] == res[9] == res[11] == m.ID and res[10] == two
        xy, inf = _pts([FBE.answer(spec, R) for R in res])
        it = items + special
        return Pool([_rows([x[0] for x in it], 32), np.stack([_tile(FB.xy_bytes(x[1], 32), 1)[0] for x in it]),
                     _rows([x[2] for x in it], 32), np.stack([_tile(FB.xy_bytes(x[3], 32), 1)[0] for x in it])],
                    [xy, inf], [False] * 8 + [True] * 4)
    items = [(k, pts[3]) for k in _draws(rng, order, 256, 8)]
    special = [(0, pts[3]), (order, pts[3]), (2, two), (3, two), (8 * order, pts[1])]
    res = [m.mul(k, P) for k, P in items + special]
    assert res[8] == res[9] == res[10] == res[12] == m.ID and res[11] == two
    xy, inf = _pts([FBE.answer(spec, R) for R in res])
    it = items + special
    return Pool([_rows([x[0] for x in it], 32), np.stack([_tile(FB.xy_bytes(x[1], 32), 1)[0] for x in it])],
                [xy, inf], [False] * 8 + [True] * 5)


def _edwards_base_pool(name, op):
    """mul_base / mul_base2 over tables of a user-defined Edwards id: identity results"""
    spec = FBE.spec_of(name)
    m, pts, order = FBE.model_of(spec), FBE.bases_of(spec), I(spec["n"])
    rng = random.Random("inv-batch:%s:%s" % (name, op))
    if op == "mul_base2":
        a = rng.randrange(2, order)
        k1 = _draws(rng, order, 256, 8) + [a, 0, order, 5]
        k2 = _draws(rng, order, 256, 8) + [a, 0, 0, 5]
        res = [m.mul2(x, pts[0], y, pts[2]) for x, y in zip(k1, k2)]
        xy, inf = _pts([FBE.answer(spec, R) for R in res])
        assert all(R == m.ID for R in res[8:])
        return Pool([_rows(k1, 32), _rows(k2, 32)], [xy, inf], [False] * 8 + [True] * 4)
    ks = _draws(rng, order, 256, 8) + [0, order, 2 * order]
    res = [m.mul(k, pts[3]) for k in ks]
    assert all(R == m.ID for R in res[8:])
    xy, inf = _pts([FBE.answer(spec, R) for R in res])
    return Pool([_rows(ks, 32)], [xy, inf], [False] * 8 + [True] * 3)


def _x25519_pool():
    """mont.h normalize: Z = 0 from the abscissae of low order (0, 1, the two of order eight, p - 1)
    under scalars that are multiples of their order, beside ordinary products"""
    from oracle import ec_oracle as O
    p = (1 << 255) - 19
    m, cur = CM.Model(p, 486662), O.get_curve("curve25519", precompute=False)
    rng = random.Random("inv-batch:x25519")
    low = [0, 1, p - 1, 325606250916557431795983626356110631294008115727848805560023387167927233504,
           39382357235489614581723060781553021112529911719440698176882885853963445705823]
    items = [(rng.getrandbits(255), 9 if i < 3 else rng.randrange(2, p)) for i in range(10)]
    items += [(8 * rng.getrandbits(200), u) for u in low] + [(0, 9), (8 * rng.getrandbits(200) + 1, 0)]
    res = [m.ladder(k, x) for k, x in items]
    for (k, x), (gx, inf) in zip(items, res):
        want = cur.mul_x(x, k)
        assert (want is None and inf == 1) or (want == gx and inf == 0) or (want == 0 and inf == 1), (k, x)
    inf = np.array([r[1] for r in res], np.uint8)
    assert inf[10:].all() and not inf[:10].any()
    return Pool([_rows([k for k, _ in items], 32), _rows([x for _, x in items], 32)], [_rows([r[0] for r in res], 32), inf], inf == 1)


def _signatures(D, d, rng, m, hash_len):
    out = []
    while len(out) < m:
        h, k = rng.randbytes(hash_len), rng.randrange(2, D.n - 1)
        r, s, R = D.sign(d, h, 0, k)
        if r and s:
            out.append((h, r, s, R))
    return out


def _verify_pool(name):
    """ecdsa_prep: r = 0, s = 0, r = n, s = n, s = 2^bits - 1 beside valid and tampered signatures"""
    spec = VB.spec_of(name)
    D = VB.domain_of(spec)
    d, Q = VB.keys_of(spec)[3]
    rng = random.Random("inv-batch:verify:" + name)
    sig = _signatures(D, d, rng, 15, D.B)
    top = (1 << (8 * D.B)) - 1
    hs = [x[0] for x in sig]
    rs = [x[1] for x in sig[:10]] + [0, sig[11][1], D.n, sig[13][1], sig[14][1]]
    ss = [x[2] for x in sig[:8]] + [sig[8][2] ^ 1, sig[9][2] ^ 2] + [sig[10][2], 0, sig[12][2], D.n, top]
    ok = np.array(D.verify_many(hs, 0, rs, ss, Q), np.uint8)
    assert ok[:8].all() and not ok[8:].any()
    m = len(hs)
    pool = Pool([np.stack([np.frombuffer(h, np.uint8) for h in hs]), _rows(rs, D.B), _rows(ss, D.B), _tile(FB.xy_bytes(Q, D.B), m)],
                [ok, np.zeros(m, np.uint8)], [False] * 10 + [True] * 5)
    return pool


def _recover_pool(name):
    """recover_prep: r = 0, r >= n, recid > 3, the second candidate with r >= p - n; beside them
    signatures with their recovery parameter and random (r, s) whose x may have no point"""
    from oracle import ec_oracle as O
    spec = VB.spec_of(name)
    D = VB.domain_of(spec)
    cur = O.get_curve(name, precompute=False)
    B, n, p = D.B, D.n, D.p
    rng = random.Random("inv-batch:recover:" + name)
    d = rng.randrange(2, n)
    items = []
    for h, r, s, R in _signatures(D, d, rng, 7, 32):
        items.append((h, r, s, (R[1] & 1) | (2 if R[0] != r else 0)))
    items += [(rng.randbytes(32), rng.randrange(1, n), rng.randrange(1, n), rng.randrange(2)) for _ in range(3)]
    pmn = p % n
    top = (1 << (8 * B)) - 1
    refused = [(0, 0), (0, 3), (n, 1), (min(n + 1, top), 0), (top, 2), (rng.randrange(1, n), 4), (rng.randrange(1, n), 5),
               (rng.randrange(pmn, n), 2), (pmn, 3)]
    items += [(rng.randbytes(32), r, rng.randrange(1, n), j) for r, j in refused]
    st, xy = [], []
    for h, r, s, j in items:
        if r == 0 or r >= n:
            st.append(3), xy.append(bytes(2 * B))
            continue
        try:
            Qr = O.ecdsa_recover(cur, int.from_bytes(h, "big"), r, s, j)
            st.append(1 if Qr.inf else 0), xy.append(bytes(2 * B) if Qr.inf else FB.xy_bytes((Qr.x, Qr.y), B))
        except ValueError as e:
            assert str(e) in CR.THROWN, e
            st.append(2), xy.append(bytes(2 * B))
    st = np.array(st, np.uint8)
    assert (st[:7] == 0).all() and st[10:15].tolist() == [3] * 5 and (st[15:] == 2).all()
    return Pool([np.stack([np.frombuffer(x[0], np.uint8) for x in items]), _rows([x[1] for x in items], B),
                 _rows([x[2] for x in items], B), np.array([x[3] for x in items], np.uint8)],
                [np.stack([np.frombuffer(x, np.uint8) for x in xy]), st], [False] * 10 + [True] * 9)


def _sign_pool(name):
    """sign_finish: what its code refuses -- k <= 1, k >= n - 1 (k = 0, 1, n - 1, n, all ones) and
    s = 0 (d = -e / r); r = 0 and k G = O cannot be built (k = 0 mod n is out of range first).  On
    p521 a nonce of 66 significant bytes is shifted down by seven bits first, as options.k's BN is:
    n - 1 and n are ordinary nonces there, and the items are labelled by the oracle's answer"""
    from oracle import ec_oracle as O
    spec = VB.spec_of(name)
    D = VB.domain_of(spec)
    cur = O.get_curve(name, precompute=True)
    NB, n = D.B, D.n
    rng = random.Random("inv-batch:sign:" + name)
    items = [(rng.randbytes(NB), rng.randrange(1, n), rng.randrange(2, n - 1)) for _ in range(10)]
    h0, k0 = rng.randbytes(NB), rng.randrange(2, n - 1)
    r0 = D.m.mul(k0, D.G)[0] % n
    d0 = (n - O.truncate_to_n(cur, int.from_bytes(h0, "big"), NB)) * pow(r0, -1, n) % n
    items += [(rng.randbytes(NB), rng.randrange(1, n), k) for k in (0, 1, n - 1, n, (1 << (8 * NB)) - 1)] + [(h0, d0, k0)]
    res = [O.ecdsa_sign(cur, int.from_bytes(h, "big"), NB, d, k.to_bytes(NB, "big")) for h, d, k in items]
    assert all(g is not None for g in res[:10]) and sum(g is None for g in res[10:]) >= 4 and res[-1] is None
    m = len(items)
    r, s = np.zeros((m, NB), np.uint8), np.zeros((m, NB), np.uint8)
    j, ok = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    for i, g in enumerate(res):
        if g is not None:
            r[i], s[i], j[i], ok[i] = _rows([g[0]], NB)[0], _rows([g[1]], NB)[0], g[2], 1
    return Pool([np.stack([np.frombuffer(x[0], np.uint8) for x in items]), _rows([x[1] for x in items], NB),
                 _rows([x[2] for x in items], NB)], [r, s, j, ok], ok == 0)


def _rt_recover_pool(name):
    bt = CR.random_batch(CR.spec_of(name), 80, 11)
    return Pool([bt["h"], bt["r"], bt["s"], bt["j"]], [bt["xy"], bt["st"]], bt["st"] != 0)


def _rt_sign_pool(name):
    bt = CS.sup_batch(CS.spec_of(name), 64, 11, 32, 0)
    return Pool([bt["h"], bt["d"], bt["k"]], [bt["r"], bt["s"], bt["j"], bt["ok"]], bt["ok"] == 0)


def _rt_derive_pool(name, wire):
    """rt_derive_finish: every status -- 1 not validated, 2 the product at infinity, 3 undecoded (wire)"""
    spec = CH.spec_of(name)
    bt = CH.random_batch(spec, 80, 11)
    if not wire:
        assert {1, 2} <= set(bt["st"].tolist())
        return Pool([bt["priv"], bt["pub"]], [bt["x"], bt["st"]], bt["st"] != 0)
    enc, st, x, err = CH.wire_batch(spec, bt, 80, False)
    assert {1, 2, 3} <= set(st.tolist())
    return Pool([bt["priv"][:80], enc], [x, st, err], st != 0)


def _ed_decompress_pool(name, from_y):
    """edckey.h quotient through custom_ed_decompress: 0, 1, p - 1 and values without a root beside
    ordinary ones (and the coordinates whose denominator is 0, on a curve that has them: the
    fixtures' do not -- their zero denominators come over the wire, _ed_derive_pool)"""
    m = CE.model_of(CE.spec_of(name))
    p = m.p
    rng = random.Random("inv-batch:ed-decompress:%s:%d" % (name, from_y))
    f = m.from_y if from_y else m.from_x
    # from_x divides by 1 - d x^2, from_y by d y^2 - a
    z = m.sqrt((m.a if from_y else 1) * m.inv0(m.d) % p)
    zero_den = [] if z is None else [z, p - z]
    good = [v for v in (rng.randrange(2, p) for _ in range(200)) if f(v, 0)[1] == 0][:10]
    bad = [v for v in (rng.randrange(2, p) for _ in range(200)) if f(v, 0)[1] != 0][:4]
    vs = good + [0, 1, p - 1] + zero_den + bad
    odd = [rng.getrandbits(1) for _ in vs]
    res = [f(v, o) for v, o in zip(vs, odd)]
    st = np.array([r[1] for r in res], np.uint8)
    refused = [False] * 10 + [True] * (len(vs) - 10)
    return Pool([CE.rows(vs), np.array(odd, np.uint8)], [CE.xy_rows([r[0] or (0, 0) for r in res]), st], refused)


def _ed_derive_pool(name, wire):
    """edckey.h derive_finish: every status.  wire = "comp": the keys as 02 / 03 || x, where the
    quotient has work to do -- and a key with another prefix at that length ('Unknown point format',
    err 1) has no fraction: its planes hold 0 / 0, the zero denominators beside the real ones.  (On
    the fixtures' curves no coordinate has a zero denominator: d and a / d are non-residues.)"""
    bt = CE.random_batch(CE.spec_of(name), 64, 11, distinct=64)
    if not wire:
        return Pool([bt["k"], bt["xy"]], [bt["dx"], bt["dst"]], bt["dst"] != 0)
    w = bt["wire"][wire]
    assert {1, 3} <= set(w["st"].tolist()) if wire == "full" else (w["err"] == 1).sum() >= 2
    return Pool([w["k"], w["enc"]], [w["x"], w["st"], w["err"]], w["st"] != 0 if wire == "full" else w["err"] == 1)


def _ed_decode_pool(name):
    """edckey.h quotient through custom_ed_decode_points: compressed keys beside keys without a
    fraction (0 / 0), as in _ed_derive_pool"""
    bt = CE.random_batch(CE.spec_of(name), 64, 11, distinct=64)
    m = CE.model_of(CE.spec_of(name))
    enc = bt["wire"]["comp"]["enc"]
    res = [m.decode(e.tobytes()) for e in enc]
    st = np.array([r[1] for r in res], np.uint8)
    assert (st == bt["wire"]["comp"]["err"]).all() and (st == 1).sum() >= 2
    return Pool([enc], [CE.xy_rows([r[0] or (0, 0) for r in res]), st], st == 1)


def _ed_verify_pool(name):
    bt = CEE.verify_batch(CEE.spec_of(name), 64, 11, distinct=64)
    special = np.isin(bt["kind"], ["r_0", "s_0", "r_n", "s_n", "p_is_identity", "key_identity", "key_small_order", "off_curve"])
    return Pool([bt["h"], bt["r"], bt["s"], bt["q"]], [bt["ok"], bt["st"]], special)


def _ed_sign_pool(name):
    bt = CEE.sup_batch(CEE.spec_of(name), 64, 11, 32, 0, distinct=64)
    return Pool([bt["h"], bt["d"], bt["k"]], [bt["r"], bt["s"], bt["j"], bt["ok"]], bt["ok"] == 0)


def _mont_pool(name, derive):
    bt = CM.random_batch(CM.spec_of(name), 64, 11)
    if derive:
        assert bt["statuses"] <= set(bt["dst"].tolist())
        return Pool([bt["k"], bt["x"]], [bt["dx"], bt["dst"]], bt["dst"] != 0)
    return Pool([bt["k"], bt["x"]], [bt["ox"], bt["inf"]], bt["inf"] != 0)


# ---- the case table -----------------------------------------------------------------------------

class Case:
    """id; routines: "<header>:<function>" of the shared-inversion routines the row is there for;
    kind: which override sets their K ("norm" / "prep"); kernels: launch names that have to be seen;
    pool(); setup(ctx) -> what run needs of the context (a curve id, handles), made once per context;
    run(ctx, handle, inputs, form) -> outputs"""

    def __init__(self, id, routines, kind, kernels, pool, setup, run, setup_kernels=()):
        self.id, self.routines, self.kind, self.kernels = id, tuple(routines), kind, tuple(kernels)
        self._pool, self._setup, self._run, self.setup_kernels = pool, setup, run, tuple(setup_kernels)

    def pool(self):
        if self.id not in _cache:
            _cache[self.id] = self._pool()
        return _cache[self.id]

    def K(self, ctx):
        return ctx.inv_ks[0 if self.kind == "norm" else 1]

    def handle(self, ctx):
        if self.id not in ctx.inv_handles:
            ctx.inv_handles[self.id] = self._setup(ctx)
        return ctx.inv_handles[self.id]

    def run(self, ctx, ins, form):
        return [np.asarray(o) for o in self._run(ctx, self.handle(ctx), ins, form)]


def _shared(key, make):
    """setup: one curve id per definition and context"""
    def setup(ctx):
        if key not in ctx.inv_handles:
            ctx.inv_handles[key] = make(ctx)
        return ctx.inv_handles[key]
    return setup


def _build_cases():
    cs = []
    nothing = lambda ctx: None
    for name in PRESETS:
        B = FB.spec_of(name)["B"]
        for op, run in (("mul_var", run_mul_var), ("mul_add2", run_mul_add2), ("mul_fixed", run_mul_fixed)):
            cs.append(Case("%s-%s" % (op, name), ["work.h:normalize"], "norm", ["normalize"],
                           lambda name=name, op=op: _short_pool(name, op), nothing,
                           lambda ctx, h, ins, form, name=name, B=B, run=run: run(ctx, name, B, ins, form)))
        cs.append(Case("ecdsa_verify-" + name, ["work.h:ecdsa_prep"], "prep", ["ecdsa_prep_table" if name == "secp256k1" else "ecdsa_prep"],
                       lambda name=name: _verify_pool(name), nothing,
                       lambda ctx, h, ins, form, name=name: run_verify(ctx, name, ins, form)))
        cs.append(Case("ecdsa_recover-" + name, ["work.h:recover_prep"], "prep", ["recover_prep"],
                       lambda name=name: _recover_pool(name), nothing,
                       lambda ctx, h, ins, form, name=name, B=B: run_recover(ctx, name, B, ins, form)))
        cs.append(Case("ecdsa_sign-" + name, ["work.h:sign_finish"], "prep", ["sign_finish", "normalize"],
                       lambda name=name: _sign_pool(name), nothing,
                       lambda ctx, h, ins, form, name=name, B=B: run_sign(ctx, name, B, ins, form)))
    # ecdsa_verify_base (ecdsa_base_chunk): the signed comb, the unsigned one, a user-defined domain
    for name, width in (("secp256k1", 4), ("p192", 8), ("brainpoolP256r1", 8)):
        spec = VB.spec_of(name)

        def base(ctx, spec=spec, width=width):
            cid = _shared(("vb", spec["name"]), lambda c: VB.curve_id(c, spec))(ctx)
            return ctx.define_base(cid, FB.xy_bytes(VB.keys_of(spec)[3][1], spec["B"]), width)
        cs.append(Case("ecdsa_verify_base-" + name, ["work.h:ecdsa_prep"], "prep", ["ecdsa_prep"],
                       lambda name=name: _verify_pool(name), base,
                       lambda ctx, h, ins, form: [VB.run_verify(ctx, h, ins[0], ins[1], ins[2], 0, form), np.zeros(len(ins[0]), np.uint8)]))
    spec = VB.spec_of("brainpoolP256r1")
    cs.append(Case("ecdsa_verify-brainpoolP256r1", ["work.h:ecdsa_prep"], "prep", ["ecdsa_prep"],
                   lambda: _verify_pool("brainpoolP256r1"), _shared(("vb", "brainpoolP256r1"), lambda c: VB.curve_id(c, spec)),
                   lambda ctx, h, ins, form: run_verify(ctx, h, ins, form)))
    cs.append(Case("x25519", ["mont.h:normalize"], "norm", ["x25519_normalize"], _x25519_pool, nothing,
                   lambda ctx, h, ins, form: run_x25519(ctx, ins, form)))
    for op, run in (("mul_var", run_mul_var), ("mul_add2", run_mul_add2)):
        cs.append(Case("%s-ed25519" % op, ["edwards.h:normalize"], "norm", ["ed_normalize"],
                       lambda op=op: _edwards_pool("ed25519", op), nothing,
                       lambda ctx, h, ins, form, run=run: run(ctx, "ed25519", 32, ins, form)))
    # the run-time-modulus kernels: a 256-bit domain and a 112-bit one whose order is above its prime
    for name in ("brainpoolP256r1", "secp112r1"):
        dom = _shared(("cd", name), lambda c, name=name: CR.define(c, CR.spec_of(name)))
        cs.append(Case("custom_recover-" + name, ["work.h:rt_recover_prep"], "prep", ["rt_recover_prep"],
                       lambda name=name: _rt_recover_pool(name), dom,
                       lambda ctx, h, ins, form: CR.run_recover(ctx, h, *ins, form=form)))
        cs.append(Case("custom_sign-" + name, ["work.h:rt_sign_finish"], "prep", ["rt_sign_finish", "normalize"],
                       lambda name=name: _rt_sign_pool(name), dom,
                       lambda ctx, h, ins, form: CS.run_sign(ctx, h, *ins, form=form)))
        cs.append(Case("custom_derive-" + name, ["work.h:rt_derive_finish"], "norm", ["rt_derive_finish"],
                       lambda name=name: _rt_derive_pool(name, False), dom,
                       lambda ctx, h, ins, form: CH.run_derive(ctx, h, *ins, form=form)))
        cs.append(Case("custom_derive_wire-" + name, ["work.h:rt_derive_finish"], "norm", ["rt_derive_finish"],
                       lambda name=name: _rt_derive_pool(name, True), dom,
                       lambda ctx, h, ins, form: CH.run_derive_wire(ctx, h, *ins, form=form)))
    # user-defined Edwards ids: a domain and a plain curve
    for name in ("curve1174", "e222"):
        ed = _shared(("fbe", name), lambda c, name=name: FBE.curve_id(c, FBE.spec_of(name)))
        for op, run in (("mul_var", run_mul_var), ("mul_add2", run_mul_add2)):
            cs.append(Case("%s-%s" % (op, name), ["edcustom.h:normalize"], "norm", ["edc_normalize"],
                           lambda name=name, op=op: _edwards_pool(name, op), ed,
                           lambda ctx, h, ins, form, run=run: run(ctx, h, 32, ins, form)))

        def bases(ctx, name=name, ed=ed):
            spec = FBE.spec_of(name)
            return FBE.define_bases(ctx, spec, 8, ed(ctx), which=(0, 2, 3))[1]
        cs.append(Case("mul_base-" + name, ["edcustom.h:normalize"], "norm", ["edc_normalize"],
                       lambda name=name: _edwards_base_pool(name, "mul_base"), bases,
                       lambda ctx, h, ins, form: FB.run_mul(ctx, h[3], ins[0], 32, form), setup_kernels=["edc_base_normalize"]))
        cs.append(Case("mul_base2-" + name, ["edcustom.h:normalize"], "norm", ["edc_normalize"],
                       lambda name=name: _edwards_base_pool(name, "mul_base2"), bases,
                       lambda ctx, h, ins, form: FB.run_mul2(ctx, h[0], h[2], ins[0], ins[1], 32, form)))
    for name in ("curve1174", "twisted_a4"):
        ed = _shared(("ce", name), lambda c, name=name: CE.define(c, CE.spec_of(name)))
        for from_y in (False, True):
            cs.append(Case("custom_ed_decompress-%s-%s" % ("y" if from_y else "x", name), ["edckey.h:quotient"], "norm",
                           ["edc_key_quotient"], lambda name=name, from_y=from_y: _ed_decompress_pool(name, from_y), ed,
                           lambda ctx, h, ins, form, from_y=from_y: CE.run_decompress(ctx, h, ins[0], ins[1], from_y, form)))
        cs.append(Case("custom_ed_derive-" + name, ["edckey.h:derive_finish"], "norm", ["edc_key_derive_finish"],
                       lambda name=name: _ed_derive_pool(name, False), ed,
                       lambda ctx, h, ins, form: CE.run_derive(ctx, h, ins[0], ins[1], form)))
        cs.append(Case("custom_ed_derive_wire-full-" + name, ["edckey.h:derive_finish"], "norm", ["edc_key_derive_finish"],
                       lambda name=name: _ed_derive_pool(name, "full"), ed,
                       lambda ctx, h, ins, form: CE.run_derive_wire(ctx, h, ins[0], ins[1], form)))
        cs.append(Case("custom_ed_derive_wire-comp-" + name, ["edckey.h:quotient", "edckey.h:derive_finish"], "norm",
                       ["edc_key_quotient", "edc_key_derive_finish"], lambda name=name: _ed_derive_pool(name, "comp"), ed,
                       lambda ctx, h, ins, form: CE.run_derive_wire(ctx, h, ins[0], ins[1], form)))
        cs.append(Case("custom_ed_decode_points-" + name, ["edckey.h:quotient"], "norm", ["edc_key_quotient"],
                       lambda name=name: _ed_decode_pool(name), ed,
                       lambda ctx, h, ins, form: CE.run_decode(ctx, h, ins[0], form)))
    # ECDSA on Edwards domains: the toy domain compares in affine form (eq_affine), the others by
    # Maxwell's trick after the short domains' ecdsa_prep
    for name, routines, kind, kernels in (("toy_p65521", ["edcecdsa.h:eq_affine"], "norm", ["edc_ecdsa_eq_affine", "ecdsa_prep"]),
                                          ("curve1174", ["work.h:ecdsa_prep"], "prep", ["ecdsa_prep"])):
        dom = _shared(("cee", name), lambda c, name=name: CEE.define(c, CEE.spec_of(name)))
        cs.append(Case("custom_ed_verify-" + name, routines, kind, kernels, lambda name=name: _ed_verify_pool(name), dom,
                       lambda ctx, h, ins, form: CEE.run_verify(ctx, h, *ins, bits=0, form=form)))
    for name in ("curve1174", "toy_p65521"):
        dom = _shared(("cee", name), lambda c, name=name: CEE.define(c, CEE.spec_of(name)))
        cs.append(Case("custom_ed_sign-" + name, ["edcecdsa.h:sign_norm", "work.h:rt_sign_finish"], "norm",
                       ["edc_sign_norm", "rt_sign_finish"], lambda name=name: _ed_sign_pool(name), dom,
                       lambda ctx, h, ins, form: CEE.run_sign(ctx, h, *ins, form=form)))
    for name in ("m221", "bp256_mont"):
        mo = _shared(("cm", name), lambda c, name=name: CM.define(c, CM.spec_of(name)))
        cs.append(Case("custom_mont_ladder-" + name, ["montcustom.h:normalize"], "norm", ["montc_normalize"],
                       lambda name=name: _mont_pool(name, False), mo,
                       lambda ctx, h, ins, form: CM.run_ladder(ctx, h, ins[0], ins[1], form)))
        cs.append(Case("custom_mont_derive-" + name, ["montcustom.h:normalize"], "norm", ["montc_normalize"],
                       lambda name=name: _mont_pool(name, True), mo,
                       lambda ctx, h, ins, form: CM.run_derive(ctx, h, ins[0], ins[1], form)))
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _build_cases()
CASE_IDS = [c.id for c in CASES]


def case_of(id):
    return next(c for c in CASES if c.id == id)


# ---- the guard: every routine of the headers has a row --------------------------------------------

_ROUTINE = re.compile(r"static\s+void\s+(\w+)\s*\(\s*size_t t,\s*size_t T,\s*size_t n,\s*int K\b")


def routines_in_headers():
    """"<header>:<function>" of every device routine whose parameters begin (t, T, n, K)"""
    found = []
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".h"):
            with open(os.path.join(CSRC, f)) as fh:
                found += ["%s:%s" % (f, m) for m in _ROUTINE.findall(fh.read())]
    return found


def routines_with_a_row(cases=None):
    return {r for c in (CASES if cases is None else cases) for r in c.routines}


# ---- one case in one context ----------------------------------------------------------------------

def check_case(case, ctx, ref, form, launches=None, whole=False):
    """every size of the context's K and every placement: the forced context's bytes are the K = 1
    context's and the pool's.  launches(fn) -> {kernel: count} of what fn launched on ctx, where the
    runner can tell; whole: the first of the case's kernels is launched exactly once per call (the batch
    is not cut up, so T is placement()'s); -> the number of batches run"""
    K = case.K(ctx)
    pool = case.pool()
    case.handle(ref)
    if launches and case.setup_kernels and case.id not in ctx.inv_handles:
        seen = launches(lambda: case.handle(ctx))
        assert all(seen.get(k, 0) >= 1 for k in case.setup_kernels), (case.id, seen)
    case.handle(ctx)
    warm = compose(pool, placement(1, K)[0])[0]
    case.run(ctx, warm, form), case.run(ref, warm, form)       # (the curve's own tables are built at first use)
    ran = 0
    for n in sizes_of(K):
        for rot in range(rotations_of(n, K)):
            mask, plan = placement(n, K, rot)
            ins, want = compose(pool, mask)
            what = (case.id, K, n, rot)
            if launches:
                box = []
                seen = launches(lambda: box.append(case.run(ctx, ins, form)))
                got = box[0]
                assert all(seen.get(k, 0) >= 1 for k in case.kernels), what + (seen,)
                assert not whole or seen[case.kernels[0]] == 1, what + (seen,)
                assert not [k for k in seen if k.endswith("_c") or k.endswith("_r")], what + (seen,)
            else:
                got = case.run(ctx, ins, form)
            one = case.run(ref, ins, form)
            assert len(got) == len(one) == len(want), what
            for j, (g, o, w) in enumerate(zip(got, one, want)):
                bad = np.nonzero((g != o).reshape(n, -1).any(axis=1))[0]
                assert bad.size == 0, what + ("differs from K = 1", j, bad[:10].tolist(), mask[bad[:10]].tolist())
                bad = np.nonzero((g != w).reshape(n, -1).any(axis=1))[0]
                assert bad.size == 0, what + ("differs from the model", j, bad[:10].tolist(), mask[bad[:10]].tolist())
            ran += 1
    return ran
