"""EdDSA verification against a fixed-base table of the signer's key (ellgpu_eddsa_verify_base): the
reference's recorded verdicts (tests/golden/eddsa_verify_base.json,
tools/gen_golden_eddsa_verify_base.js), a Python-integer model of EDDSA#verify with a Point as the
key, and the helpers the hostsim, device and N-API tests share.

The model is oracle.ec_oracle's: eddsa_verify (eddsa/index.js:52-63) on encodePoint(A), with
ed_encode_point / ed_decode_point; a ValueError of the oracle is the reference's throw (err = 1).
check_model_pinned holds it to every recorded verdict before anything else relies on it.

Every call is run with one of three memory kinds: "host" (ELLGPU_MEM_HOST), "dev_np"
(ELLGPU_MEM_DEVICE on the hostsim build, where device memory is host memory) and "dev_torch"
(ELLGPU_MEM_DEVICE on device tensors, the current stream)."""
import hashlib
import json
import os
import random

import numpy as np

from oracle import ec_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "eddsa_verify_base.json")
FILL = 0xA5
KEYS = ["G", "negG", "aG1", "aG2", "identity", "order2", "T8", "aG_T8"]
TAGS = ["valid0", "valid1", "valid47", "valid48", "valid175", "valid176", "valid300", "flip_R", "flip_S", "flip_M",
        "S_n", "S_plus_n", "S_zero", "R_undecodable", "R_x0_odd", "R_noncanon"]
LENGTHS = [0, 1, 47, 48, 111, 112, 175, 176]
_cache = {}


def golden():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
    return _cache["golden"]


def curve():
    if "curve" not in _cache:
        _cache["curve"] = O.get_curve("ed25519")
    return _cache["curve"]


def key_of(name):
    """-> (x, y, a or None) of a fixture key"""
    k = next(k for k in golden()["keys"] if k["name"] == name)
    return int(k["x"], 16), int(k["y"], 16), None if k["a"] is None else int(k["a"], 16)


def cases_of(name):
    return golden()["cases"][KEYS.index(name)]


def xy_bytes(name):
    x, y, _ = key_of(name)
    return x.to_bytes(32, "big") + y.to_bytes(32, "big")


def enc_of(name):
    """encodePoint(A)"""
    x, y, _ = key_of(name)
    return O.ed_encode_point(curve().point(x, y))


# ---- the model ------------------------------------------------------------------------------

def model(msg, sig, enc):
    """-> (ok, err) of one item"""
    try:
        return (1 if O.eddsa_verify(curve(), msg, sig, enc) else 0), 0
    except ValueError:
        return 0, 1


def model_many(msgs, sigs, enc):
    r = [model(m, s, enc) for m, s in zip(msgs, sigs)]
    return np.array([a for a, _ in r], np.uint8), np.array([b for _, b in r], np.uint8)


def recorded(c):
    """(ok, err) of a fixture row"""
    return (0, 1) if isinstance(c[3], str) else (c[3], 0)


def check_fixture_shape():
    g, c = golden(), curve()
    assert g["curve"] == "ed25519" and int(g["n"], 16) == c.n and int(g["p"], 16) == c.p and g["tags"] == TAGS
    assert [k["name"] for k in g["keys"]] == KEYS and len(g["cases"]) == len(KEYS)
    assert os.path.getsize(GOLDEN) < 100 * 1024
    p = c.p
    assert key_of("G")[:2] == c.g.normalized() and key_of("negG")[:2] == ((p - c.g.normalized()[0]) % p, c.g.normalized()[1])
    assert key_of("identity")[:2] == (0, 1) and key_of("order2")[:2] == (0, p - 1)
    for name in KEYS:
        x, y, a = key_of(name)
        assert O.ed_validate(c, x, y) and x < p and y < p
        P = c.point(x, y)
        if name in ("G", "negG", "aG1", "aG2"):
            assert c.g.mul(a).normalized() == (x, y)
        if name in ("identity", "order2", "T8"):
            assert a is None
        cs = cases_of(name)
        assert set(TAGS) <= {r[0] for r in cs} and {r[3] for r in cs if not isinstance(r[3], str)} == {0, 1}
        by = {r[0]: r for r in cs}
        assert [len(by["valid%d" % n][1]) // 2 for n in (0, 1, 47, 48, 175, 176, 300)] == [0, 1, 47, 48, 175, 176, 300]
        assert all(isinstance(by[t][3], str) and by[t][3].startswith("throw") for t in ("R_undecodable", "R_x0_odd"))
        assert all(by[t][3] == 0 for t in ("S_n", "S_plus_n"))
        assert int.from_bytes(bytes.fromhex(by["S_n"][2])[32:], "little") == c.n
        assert int.from_bytes(bytes.fromhex(by["R_noncanon"][2])[:32], "little") == p + 1
        if name in ("G", "negG", "aG1", "aG2"):
            assert by["R_noncanon"][3] == 1 and all(by["valid%d" % n][3] == 1 for n in (0, 1, 47, 48, 175, 176, 300))
        if name in ("T8", "aG_T8"):
            built = [r[3] for r in cs if r[0].startswith(("valid", "torsion_"))]
            assert set(built) == {0, 1}
            # order 8 exactly: 4 T is not the identity, 8 T is (T = the key, or the key minus a G)
            T = P if name == "T8" else P.add(c.g.mul(a).neg())
            assert T.mul(4).normalized() != (0, 1) and T.mul(8).normalized() == (0, 1)


def check_model_pinned():
    for name in KEYS:
        enc = enc_of(name)
        for r in cases_of(name):
            assert model(bytes.fromhex(r[1]), bytes.fromhex(r[2]), enc) == recorded(r), (name, r[0])


# ---- the engine's side ----------------------------------------------------------------------

def define_key(ctx, name):
    return ctx.define_ed_base("ed25519", xy_bytes(name))


def _raw(ctx, rc):
    from elliptic_amd import _lib
    if rc != 0:
        raise _lib.EllgpuError(rc, ctx._lib.ellgpu_last_error().decode())


def _P(a):
    return a.ctypes.data if a is not None else None


def pack(msgs):
    """a list of byte strings -> (flat uint8 array, never empty; n + 1 uint64 offsets)"""
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return np.frombuffer(b"".join(msgs) or b"\0", np.uint8).copy(), off


def run_verify(ctx, base, msgs, sigs, mem="host", offsets=False, want_err=True):
    """ellgpu_eddsa_verify_base on a list of byte strings and an (n, 64) uint8 array -> (ok, err), (n,)
    uint8, written into buffers that were filled with 0xA5.  offsets: the messages concatenated with
    n + 1 offsets; otherwise rows of a uniform stride (the messages must then have one length).
    want_err=False: out_err is NULL, err comes back None."""
    sigs = np.ascontiguousarray(sigs, np.uint8).reshape(-1, 64)
    n = sigs.shape[0]
    assert len(msgs) == n
    if offsets:
        flat, off = pack(msgs)
        mlen = 0
    else:
        assert len({len(m) for m in msgs}) <= 1
        mlen = len(msgs[0]) if n else 0
        flat, off = np.frombuffer(b"".join(msgs) or b"\0", np.uint8).copy(), None
    if mem == "dev_torch":
        import torch
        dm = torch.from_numpy(flat).cuda()
        if not offsets:
            dm = dm[:n * mlen].reshape(n, mlen)
        doff = torch.from_numpy(off.view(np.int64)).cuda() if offsets else None
        ds = torch.from_numpy(sigs).cuda()
        out = tuple(torch.full((n,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2 if want_err else 1))
        ctx.eddsa_verify_base(base, dm, ds, msg_off=doff, out=out)
        torch.cuda.synchronize()
        return out[0].cpu().numpy(), (out[1].cpu().numpy() if want_err else None)
    ok = np.full(n, FILL, np.uint8)
    err = np.full(n, FILL, np.uint8) if want_err else None
    if mem == "host" and want_err:
        got = ctx.eddsa_verify_base(base, list(msgs) if offsets else np.frombuffer(b"".join(msgs), np.uint8).reshape(n, mlen),
                                    sigs, out=(ok, err))
        assert got[0] is ok and got[1] is err
    else:
        _raw(ctx, ctx._lib.ellgpu_eddsa_verify_base(ctx._ctx, base, n, _P(flat), _P(off), mlen, _P(sigs), _P(ok), _P(err),
                                                    0 if mem == "host" else 1, None))
    return ok, err


def check_golden(ctx, name, base, mem):
    """every recorded case of one key through one memory kind in both message forms -- a uniform
    stride per length group, and offsets with the mixed lengths in one call: the reference's
    verdicts, the same bytes, nothing but 0 and 1; -> the bytes of the offsets form"""
    cs = cases_of(name)
    msgs = [bytes.fromhex(r[1]) for r in cs]
    sigs = np.stack([np.frombuffer(bytes.fromhex(r[2]), np.uint8) for r in cs])
    want = [recorded(r) for r in cs]
    ok, err = run_verify(ctx, base, msgs, sigs, mem, offsets=True)
    assert list(zip(ok.tolist(), err.tolist())) == want, (name, mem)
    groups = {}
    for j, m in enumerate(msgs):
        groups.setdefault(len(m), []).append(j)
    ok2, err2 = np.full_like(ok, FILL), np.full_like(err, FILL)
    for ln, idx in sorted(groups.items()):
        a, b = run_verify(ctx, base, [msgs[j] for j in idx], sigs[idx], mem, offsets=False)
        ok2[idx], err2[idx] = a, b
    assert ok2.tobytes() == ok.tobytes() and err2.tobytes() == err.tobytes(), (name, mem)
    assert set(ok.tolist()) | set(err.tolist()) <= {0, 1}
    return ok, err


# ---- random batches -------------------------------------------------------------------------

def _undecodable(rng):
    c = curve()
    while True:
        y = rng.randrange(c.p)
        try:
            c.point_from_y(y, False)
        except ValueError:
            return y.to_bytes(32, "little")


def random_batch(n, seed, key, model_rows=None):
    """n signatures under the fixture key `key`, made by the model: R = r G with r advancing by one
    addition per item, S = r + h a (a = 0 on a torsion-only key), the message lengths cycling
    through 0, 1, 47, 48, 111, 112, 175, 176.  Every third item is tampered with, cycling R, S and
    the message.  The first rows are there by construction: row 0 S = n, row 1 an undecodable R,
    row 2 the identity encoded as y = p + 1 with S = h a (valid), row 3 S = 0.
    want: the model's (ok, err) for the first model_rows items (all of them by default)."""
    rng = random.Random("eddsa-verify-base:%s:%d" % (key, seed))
    c = curve()
    nn = c.n
    x, y, a = key_of(key)
    a = a or 0
    enc = enc_of(key)
    r, dr = rng.randrange(1, nn), rng.randrange(1, nn)
    R, D = c.g.mul(r), c.g.mul(dr)
    msgs, sigs, kinds = [], [], []
    for i in range(n):
        msg = bytes(rng.getrandbits(8) for _ in range(LENGTHS[i % len(LENGTHS)]))
        Renc = O.ed_encode_point(R)
        kind = "valid"
        if i == 2:
            Renc, kind = (c.p + 1).to_bytes(32, "little"), "noncanon"
        h = int.from_bytes(hashlib.sha512(Renc + enc + msg).digest(), "little") % nn
        S = ((0 if i == 2 else r) + h * a) % nn
        if i == 0:
            S, kind = nn, "S_n"
        elif i == 1:
            Renc, kind = _undecodable(rng), "undecodable"
        elif i == 3:
            S, kind = 0, "S_zero"
        elif i > 3 and i % 3 == 0:
            kind = ("R", "S", "M")[(i // 3) % 3]
            if kind == "R":
                Renc = bytes([Renc[0] ^ (1 << rng.randrange(8))]) + Renc[1:]
            elif kind == "S":
                S ^= 1 << rng.randrange(250)
            else:
                msg = (bytes([msg[0] ^ 1]) + msg[1:]) if msg else b"\x01"
        msgs.append(msg)
        sigs.append(Renc + S.to_bytes(32, "little"))
        kinds.append(kind)
        r, R = (r + dr) % nn, R.add(D)
    m = n if model_rows is None else min(n, model_rows)
    want = model_many(msgs[:m], sigs[:m], enc)
    return {"msgs": msgs, "sigs": np.stack([np.frombuffer(s, np.uint8) for s in sigs]), "kinds": kinds, "want": want,
            "key": key, "enc": np.frombuffer(enc, np.uint8)}


def batch_meets_conditions(bt):
    """both verdicts, at least one err = 1 and the four constructed rows behaving as named -- asserted
    on the model alone, before any engine runs"""
    ok, err = bt["want"]
    rows = [(int(ok[i]), int(err[i])) for i in range(4)]
    named = key_of(bt["key"])[2] is not None and bt["key"] != "aG_T8"
    return (set(ok.tolist()) == {0, 1} and err.any() and bt["kinds"][:4] == ["S_n", "undecodable", "noncanon", "S_zero"]
            and rows[0] == (0, 0) and rows[1] == (0, 1) and rows[3][1] == 0 and (rows[2] == (1, 0) or not named)
            and {"R", "S", "M", "valid"} <= set(bt["kinds"]))


def tiled_verify(ctx, bt, n):
    """ellgpu_eddsa_verify on the first n items with encodePoint(A) repeated in pubs (host memory)"""
    pubs = np.ascontiguousarray(np.broadcast_to(bt["enc"], (n, 32)))
    ok, err = ctx.eddsa_verify(bt["msgs"][:n], bt["sigs"][:n], pubs)
    return np.asarray(ok, np.uint8), np.asarray(err, np.uint8)
