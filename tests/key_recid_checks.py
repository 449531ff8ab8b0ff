"""The recovery id of a signature under a known key, in one pass (ellgpu_ecdsa_recid): the
reference's recorded answers (tests/golden/key_recid.json, tools/gen_golden_key_recid.js), a
Python-integer model of the one-pass rule and the helpers the hostsim and device tests share.

The model is the rule itself over Python integers (the affine group law of
tests/fixed_base_checks.py): status 3 where r = 0, r >= n or s = 0 (mod n); status 2 where the key,
its coordinates reduced mod p, is not on the curve; R' = (e / s) G + (r / s) Q with e = int(hash) mod
n and s reduced; status 1 where R' = O or x(R') is neither r nor r + n; else status 0 and the id
(y(R') odd) | (2 if x(R') = r + n).  check_model_pinned holds it to every recorded answer of the
reference -- EC#getKeyRecoveryParam's own loop over four recoveries -- before anything relies on it.

Memory kinds as in tests/verify_base_checks.py: "host", "dev_np" (ELLGPU_MEM_DEVICE on the hostsim
build, where device memory is host memory) and "dev_torch" (device tensors, the current stream)."""
import json
import os
import random
import subprocess
import sys

import numpy as np

import fixed_base_checks as FB

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "key_recid.json")
FILL = 0xA5
PRESETS = FB.PRESETS
I = FB.I
rows = FB.rows
STATUS_OF = {"throws": 1, "offcurve": 2, "outside": 3}
_cache = {}


def curves():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
    return _cache["golden"]


def spec_of(name):
    return next(c for c in curves() if c["name"] == name)


def expected_of(want):
    """a recorded answer -> (recid, status)"""
    return (0, STATUS_OF[want]) if isinstance(want, str) else (int(want), 0)


# ---- the model ------------------------------------------------------------------------------

class Curve:
    def __init__(self, spec):
        from oracle import ec_oracle as O
        c = O.get_curve(spec["name"], precompute=False)
        assert c.p == I(spec["p"]) and c.n == I(spec["n"])
        self.name, self.B, self.p, self.n = spec["name"], spec["B"], c.p, c.n
        self.m = FB.Model(c.p, c.a, c.b)
        self.G = (c.g.x, c.g.y)
        self.bits = 8 * self.B

    def scalars(self, h, r, s):
        """(u1, u2), or None where the item is outside the engine's domain"""
        n = self.n
        if not 1 <= r < n or s % n == 0:
            return None
        w = pow(s % n, -1, n)
        return int.from_bytes(h, "big") % n * w % n, r * w % n

    def key_of(self, Q):
        """the key with its coordinates reduced, or None where that is no curve point"""
        Q = (Q[0] % self.p, Q[1] % self.p)
        return Q if self.m.on_curve(Q) else None

    def read_off(self, R, r):
        if R is None:
            return 0, 1
        if R[0] == r:
            return R[1] & 1, 0
        if R[0] == r + self.n:                       # (as integers: x < p, so r < p - n)
            return 2 | (R[1] & 1), 0
        return 0, 1

    def recid(self, h, r, s, Q):
        u = self.scalars(h, r, s)
        if u is None:
            return 0, 3
        Q = self.key_of(Q)
        if Q is None:
            return 0, 2
        return self.read_off(self.m.mul2(u[0], self.G, u[1], Q), r)

    def recid_many(self, hs, rs, ss, Q):
        """the same for a batch on one key, through Model.mul_many (held to `recid` by check_model_pinned)"""
        us = [self.scalars(h, r, s) for h, r, s in zip(hs, rs, ss)]
        out = [(0, 3)] * len(us)
        K = self.key_of(Q)
        live = [i for i, u in enumerate(us) if u is not None]
        if K is None:
            for i in live:
                out[i] = (0, 2)
            return out
        Rs = self.m.mul_many([us[i][1] for i in live], K, self.bits,
                             self.m.mul_many([us[i][0] for i in live], self.G, self.bits))
        for i, R in zip(live, Rs):
            out[i] = self.read_off(R, rs[i])
        return out


def curve_of(name):
    key = ("curve", name)
    if key not in _cache:
        _cache[key] = Curve(spec_of(name))
    return _cache[key]


def row_ints(row):
    """a fixture row -> (hash bytes, r, s, (x, y))"""
    return bytes.fromhex(row[1]), I(row[2]), I(row[3]), (I(row[4]), I(row[5]))


def check_fixture_shape(spec):
    """about 60 rows; every id, every status, both parities of the ordinary rows, three hash lengths,
    and the rows the issue names"""
    rs_ = spec["rows"]
    assert 55 <= len(rs_) <= 70
    wants = [expected_of(r[6]) for r in rs_]
    assert {w[0] for w in wants if w[1] == 0} == {0, 1, 2, 3} and {w[1] for w in wants} == {0, 1, 2, 3}
    tags = {r[0] for r in rs_}
    B, L = spec["B"], spec["long"]
    need = {"valid20", "valid%d" % B, "valid%d" % L, "flipped_s%d" % B, "ecsign_long", "small_s", "s_plus_n", "second",
            "second_top", "r_is_p_minus_n", "wrong_key", "r_plus_1", "r_minus_1", "s_plus_1", "s_minus_1", "sum_inf",
            "offcurve_y_plus_1", "offcurve_x_ge_p", "key_x_plus_p", "r_zero", "r_n", "r_n_plus_1", "s_zero", "s_n"}
    assert need <= tags, need - tags
    assert L > B and {len(r[1]) // 2 for r in rs_} == {20, B, L}
    p, n = I(spec["p"]), I(spec["n"])
    by = {r[0]: r for r in rs_}
    assert {expected_of(r[6])[0] for r in rs_ if r[0].startswith("valid")} == {0, 1}
    assert I(by["s_plus_n"][3]) >= n and I(by["r_is_p_minus_n"][2]) == p - n and by["r_is_p_minus_n"][6] == "throws"
    assert p - n - 300 < I(by["second_top"][2]) < p - n and by["second_top"][6] == 3
    assert I(by["offcurve_x_ge_p"][4]) >= p and I(by["key_x_plus_p"][4]) >= p and by["key_x_plus_p"][6] != "offcurve"
    assert (I(by["r_zero"][2]), I(by["r_n"][2]), I(by["r_n_plus_1"][2]), I(by["s_zero"][3]), I(by["s_n"][3])) == (0, n, n + 1, 0, n)
    assert all(by[t][6] == "outside" for t in ("r_zero", "r_n", "r_n_plus_1", "s_zero", "s_n"))


def check_model_pinned(spec):
    C = curve_of(spec["name"])
    for row in spec["rows"]:
        assert C.recid(*row_ints(row)) == expected_of(row[6]), (spec["name"], row[0])


# ---- batches --------------------------------------------------------------------------------

class Batch:
    """h (n, hash_len), r, s (n, B), pub (n, 2 B) uint8 and the expected recid, status (n,) uint8"""

    def __init__(self, h, r, s, pub, recid, status, tags=None):
        self.h, self.r, self.s, self.pub = (np.ascontiguousarray(a, np.uint8) for a in (h, r, s, pub))
        self.recid, self.status = np.asarray(recid, np.uint8), np.asarray(status, np.uint8)
        self.tags = tags
        self.n = self.h.shape[0]

    def take(self, idx):
        idx = np.asarray(idx)
        return Batch(self.h[idx], self.r[idx], self.s[idx], self.pub[idx], self.recid[idx], self.status[idx],
                     None if self.tags is None else [self.tags[i] for i in idx])

    def first(self, n):
        return self.take(np.arange(n))

    def tiled(self, n, seed=0):
        """n items drawn from this batch in a shuffled order (every item where n >= self.n)"""
        rng = random.Random("key-recid-tile:%d:%d" % (n, seed))
        idx = [i % self.n for i in range(n)]
        rng.shuffle(idx)
        return self.take(idx)


def _batch_of(B, items, wants, tags=None):
    return Batch(np.stack([np.frombuffer(h, np.uint8) for h, _, _, _ in items]), rows([r for _, r, _, _ in items], B),
                 rows([s for _, _, s, _ in items], B),
                 np.stack([np.frombuffer(FB.xy_bytes(Q, B), np.uint8) for _, _, _, Q in items]),
                 [w[0] for w in wants], [w[1] for w in wants], tags)


def fixture_batches(spec, shuffled=False):
    """the fixture's rows grouped by hash length (one call each), in fixture order or shuffled"""
    groups = {}
    for row in spec["rows"]:
        groups.setdefault(len(row[1]) // 2, []).append(row)
    out = []
    for hl, rs_ in sorted(groups.items()):
        if shuffled:
            rs_ = list(rs_)
            random.Random("key-recid-shuffle:%s:%d" % (spec["name"], hl)).shuffle(rs_)
        out.append(_batch_of(spec["B"], [row_ints(r) for r in rs_], [expected_of(r[6]) for r in rs_], [r[0] for r in rs_]))
    return out


def random_batch(name, n, seed=1):
    """n items over hashes of B bytes, expected values by the model.  Signatures of three keys with
    the nonces k0 + i dk; one item in eight is tampered with (r, s, the hash or the key in turn).  The
    fixture's rows of that hash length for ids 2 and 3 and for statuses 1, 2 and 3 are tiled in at
    random positions, one item in eight again where n allows it."""
    key = ("batch", name, n, seed)
    if key in _cache:
        return _cache[key]
    spec, C = spec_of(name), curve_of(name)
    B, nn, m = C.B, C.n, C.m
    rng = random.Random("key-recid:%s:%d:%d" % (name, n, seed))
    special = [r for r in spec["rows"] if len(r[1]) // 2 == B and (expected_of(r[6])[1] != 0 or expected_of(r[6])[0] >= 2)]
    rng.shuffle(special)
    # one of each id 2, 3 and status 1, 2, 3 first, so that small batches meet the conditions
    firsts, seen = [], set()
    for r in special:
        k = expected_of(r[6])
        k = ("id", k[0]) if k[1] == 0 else ("st", k[1])
        if k not in seen:
            seen.add(k)
            firsts.append(r)
    special = firsts + [r for r in special if r not in firsts]
    n_special = min(len(special) * 4, max(0, n // 8)) if n >= 16 else 0
    n_own = n - n_special
    keys = []
    for _ in range(3):
        d = rng.randrange(1, nn)
        keys.append((d, m.mul(d, C.G)))
    k, dk = rng.randrange(1, nn), rng.randrange(1, nn)
    R, S = m.mul(k, C.G), m.mul(dk, C.G)
    items = []
    for i in range(n_own):
        while R is None or R[0] % nn == 0:
            k, R = (k + dk) % nn, m.add(R, S)
        ki = i % 3
        d, Q = keys[ki]
        h = bytes(rng.getrandbits(8) for _ in range(B))
        r = R[0] % nn
        s = pow(k, -1, nn) * (int.from_bytes(h, "big") + r * d) % nn or 1
        if i % 8 == 5:
            kind = (i // 8) % 4
            bit = 1 << rng.randrange(nn.bit_length() - 1)
            if kind == 0:
                r ^= bit
            elif kind == 1:
                s ^= bit
            elif kind == 2:
                h = bytes([h[0] ^ (0x80 >> rng.randrange(8))]) + h[1:]
            else:
                ki = (ki + 1) % 3
        if s % nn == 0 or not 1 <= r < nn:
            r, s = R[0] % nn, 1                      # (keep a tampered row inside the domain: status 3 rows are tiled in)
        items.append((ki, (h, r, s, keys[ki][1])))
        k, R = (k + dk) % nn, m.add(R, S)
    wants = [None] * n_own
    for ki in range(3):
        idx = [i for i, (kk, _) in enumerate(items) if kk == ki]
        got = C.recid_many([items[i][1][0] for i in idx], [items[i][1][1] for i in idx], [items[i][1][2] for i in idx], keys[ki][1])
        for i, w in zip(idx, got):
            wants[i] = w
    all_items = [it for _, it in items]
    tags = ["own"] * n_own
    for j in range(n_special):
        row = special[j % len(special)]
        pos = rng.randrange(len(all_items) + 1)
        all_items.insert(pos, row_ints(row))
        wants.insert(pos, C.recid(*row_ints(row)))
        tags.insert(pos, row[0])
    _cache[key] = _batch_of(B, all_items, wants, tags)
    return _cache[key]


def meets_conditions(bt):
    """asserted on the expected values before any engine call: every id and every status occurs, ids 0
    and 1 make up at least 20 % of the rows each, status 0 rows are at least half"""
    ok = bt.status == 0
    return (set(bt.recid[ok].tolist()) == {0, 1, 2, 3} and set(bt.status.tolist()) == {0, 1, 2, 3}
            and all(5 * int(((bt.recid == j) & ok).sum()) >= bt.n for j in (0, 1)) and 2 * int(ok.sum()) >= bt.n)


# ---- the engine's side ----------------------------------------------------------------------

def _raw(ctx, rc):
    from elliptic_amd import _lib
    if rc != 0:
        raise _lib.EllgpuError(rc, ctx._lib.ellgpu_last_error().decode())


def run(ctx, curve, bt, mem="host"):
    """ellgpu_ecdsa_recid on a Batch -> (recid, status), written into buffers that were filled with 0xA5"""
    n = bt.n
    if mem == "dev_torch":
        import torch
        dev = [torch.from_numpy(a).cuda() for a in (bt.h, bt.r, bt.s, bt.pub)]
        out = tuple(torch.full((n,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2))
        got = ctx.ecdsa_recid(curve, *dev, out=out)
        torch.cuda.synchronize()
        assert got[0] is out[0] and got[1] is out[1]
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    rec, st = np.full(n, FILL, np.uint8), np.full(n, FILL, np.uint8)
    if mem == "host":
        got = ctx.ecdsa_recid(curve, bt.h, bt.r, bt.s, bt.pub, out=(rec, st))
        assert got[0] is rec and got[1] is st
    else:
        P = lambda a: a.ctypes.data  # noqa: E731
        _raw(ctx, ctx._lib.ellgpu_ecdsa_recid(ctx._ctx, ctx._cid(curve), n, P(bt.h), bt.h.shape[1], P(bt.r), P(bt.s),
                                              P(bt.pub), P(rec), P(st), 1, None))
    return rec, st


def check(ctx, curve, bt, mem="host"):
    """the engine's bytes are the expected ones; -> them"""
    rec, st = run(ctx, curve, bt, mem)
    bad = np.nonzero((rec != bt.recid) | (st != bt.status))[0]
    assert bad.size == 0, (curve, mem, bt.n, [(int(i), bt.tags[i] if bt.tags else None, int(rec[i]), int(st[i]),
                                               int(bt.recid[i]), int(bt.status[i])) for i in bad[:8]])
    return rec, st


def check_recover_agrees(ctx, curve, bt):
    """for every status-0 row, ecdsa_recover with the id returns the key (reduced: the fixture's
    keys with a coordinate >= p)"""
    C = curve_of(curve)
    idx = np.nonzero(bt.status == 0)[0]
    xy, st = ctx.ecdsa_recover(curve, bt.h[idx], bt.r[idx], bt.s[idx], bt.recid[idx])
    want = np.stack([np.frombuffer(FB.xy_bytes((int.from_bytes(row[:C.B].tobytes(), "big") % C.p,
                                                int.from_bytes(row[C.B:].tobytes(), "big") % C.p), C.B), np.uint8)
                     for row in bt.pub[idx]])
    assert not st.any() and xy.tobytes() == want.tobytes(), curve


def check_verify_agrees(ctx, curve, bt):
    """hashes of n's byte length on a curve whose n fills its bytes: status 0 <=> ecdsa_verify says 1,
    for the rows whose s is in [1, n) (verify refuses the others, the recovery id reduces them)"""
    C = curve_of(curve)
    assert bt.h.shape[1] == C.B and curve in ("secp256k1", "p256", "p384")
    ok = np.asarray(ctx.ecdsa_verify(curve, bt.h, bt.r, bt.s, bt.pub), np.uint8)
    s_in = np.array([1 <= int.from_bytes(row.tobytes(), "big") < C.n for row in bt.s])
    assert s_in.sum() >= bt.n // 2
    assert ((bt.status == 0)[s_in] == (ok == 1)[s_in]).all(), curve


def check_no_poison(ctx, curve, bt, mem="host"):
    """status 3 rows poison no neighbour: with those rows replaced by valid ones every other row gets the same bytes"""
    rec, st = check(ctx, curve, bt, mem)
    bad = np.nonzero(bt.status == 3)[0]
    good = np.nonzero((bt.status == 0) & (bt.recid < 2))[0]
    assert bad.size and good.size
    idx = np.arange(bt.n)
    idx[bad] = good[np.arange(bad.size) % good.size]
    rec2, st2 = check(ctx, curve, bt.take(idx), mem)
    keep = np.ones(bt.n, bool)
    keep[bad] = False
    assert rec2[keep].tobytes() == rec[keep].tobytes() and st2[keep].tobytes() == st[keep].tobytes()
    assert not st2[bad].any()


def k3_batch(name, n):
    """n items whose threads' groups of three (items t, t + T, t + 2 T, T = ceil(n / 3)) hold a status-3
    item at the first, middle and last place in turn, and some groups none"""
    bt = random_batch(name, max(n, 65))
    bad = np.nonzero(bt.status == 3)[0]
    fine = np.nonzero(bt.status != 3)[0]
    T = (n + 2) // 3
    idx = fine[np.arange(n) % fine.size]
    places = []
    for t in range(T):
        j = t % 4                                    # first, middle, last, none
        i = t + j * T
        if j < 3 and i < n:
            idx[i] = bad[t % bad.size]
            places.append(j)
    assert {0, 1, 2} <= set(places)
    return bt.take(idx)


OPTIONAL = ("ellgpu_probe_valu", "ellgpu_ctx_set_timing", "ellgpu_ctx_get_timing", "ellgpu_debug_field_op")
K3_ENV = {"ELLGPU_PREP_K": "3", "ELLGPU_NORM_K": "3"}


def run_child(code_args, env_extra, lib_path=None, timeout=600):
    """`python tests/key_recid_checks.py <args>` in a fresh child process (the overrides are read when a
    context is created, and the parent's library is initialised without them)"""
    env = dict(os.environ, **env_extra)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, HERE] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    if lib_path:
        env["KEY_RECID_HOSTSIM"] = lib_path
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in code_args], env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0 and "K3 OK" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return p.stdout


def _child_main(argv):
    """<mem> <n> <curve>...: the K = 3 batches through a context created under the overrides of K3_ENV"""
    import elliptic_amd
    assert os.environ.get("ELLGPU_PREP_K") == "3" and os.environ.get("ELLGPU_NORM_K") == "3"
    mem, n, names = argv[0], int(argv[1]), argv[2:]
    lib = None
    if mem == "dev_torch":                           # (torch finds the device first, as in the suites' fixtures)
        import torch
        assert torch.cuda.is_available()
    if os.environ.get("KEY_RECID_HOSTSIM"):          # the CPU build of the device code, which has no probes
        from elliptic_amd import _lib
        lib = _lib.load(os.environ["KEY_RECID_HOSTSIM"], optional=OPTIONAL)
    ctx = elliptic_amd.Context(0, lib_path=lib)
    try:
        for name in names:
            bt = k3_batch(name, n)
            check(ctx, name, bt, mem)
            if mem != "dev_torch":
                check(ctx, name, bt, "host")
    finally:
        ctx.close()
    print("K3 OK", mem, n, names)


if __name__ == "__main__":
    _child_main(sys.argv[1:])
