"""Checks of the wire formats on user-defined short curves (ellgpu_custom_decompress,
ellgpu_custom_decode_points, ellgpu_custom_verify_wire), shared by the CPU test
(tests/test_custom_wire_hostsim.py, the hostsim build of the device code) and the GPU test
(tests/test_custom_wire_gpu.py):

  * the reference's statuses, points, verdicts and thrown messages recorded in
    tests/golden/custom_wire.json (tools/gen_golden_custom_wire.js);
  * ShortCurve#pointFromX / BaseCurve#decodePoint restated over Python integers (Euler's
    criterion for the status, y^2 == rhs and parity for the point) for random inputs;
  * random EC#verify batches on DER signatures and SEC1 keys against ellgpu_ecdsa_verify on the
    decoded rows and against the C oracle.

Every entry point is run in one of three forms: "host" (host buffers), "dev_np" (the _dev entry
point on the hostsim build, where device memory is host memory) and "dev_torch" (the _dev entry
point on torch tensors).  Result arrays are pre-filled with 0xA5, so a byte the call leaves
unwritten shows."""
import json
import os
import random

import numpy as np

import custom_domain_checks as CD

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "custom_wire.json")
FILL = 0xA5
ERR_OF = {"Unknown point format": 1, "invalid point": 2, "Assertion failed": 3, "Signature without r or s": 4}
OFF_CURVE = 5                        # ELLGPU_STATUS_OFF_CURVE as out_err of a wire verify

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


def is_domain(spec):
    return "n" in spec


def define(ctx, spec):
    if is_domain(spec):
        return CD.define(ctx, spec)
    return ctx.define_short(I(spec["p"]), I(spec["a"]), I(spec["b"]))


def pab(spec):
    return I(spec["p"]), I(spec["a"]), I(spec["b"])


def two_adicity(p):
    s, q = 0, p - 1
    while q % 2 == 0:
        s, q = s + 1, q // 2
    return s


# ---- the three forms of every call --------------------------------------------------------

def _filled(*shapes):
    return [np.full(sh, FILL, np.uint8) for sh in shapes]


def _torch_call(fn, ins, outs):
    import torch
    di = [torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None for a in ins]
    do = [torch.from_numpy(o.copy()).cuda() if o is not None else None for o in outs]
    fn(di, do)
    torch.cuda.synchronize()
    return [o.cpu().numpy() if o is not None else None for o in do]


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _raw(ctx, rc):
    from elliptic_amd import _lib
    if rc != 0:
        raise _lib.EllgpuError(rc, ctx._lib.ellgpu_last_error().decode())


def run_decompress(ctx, cid, x, odd, form="host"):
    x = np.ascontiguousarray(x, np.uint8).reshape(-1, 32)
    odd = np.ascontiguousarray(odd, np.uint8)
    n = x.shape[0]
    xy, st = _filled((n, 64), (n,))
    if form == "host":
        ctx.custom_decompress(cid, x, odd, out=(xy, st))
    elif form == "dev_np":
        _raw(ctx, ctx._lib.ellgpu_custom_decompress_dev(ctx._ctx, cid, n, _ptr(x), _ptr(odd), _ptr(xy), _ptr(st), None))
    else:
        xy, st = _torch_call(lambda i, o: ctx.custom_decompress_dev(cid, i[0], i[1], o[0], o[1]), [x, odd], [xy, st])
    return xy, st


def run_decode(ctx, cid, enc, form="host"):
    enc = np.ascontiguousarray(enc, np.uint8)
    n, enc_len = enc.shape
    xy, st = _filled((n, 64), (n,))
    if form == "host":
        ctx.custom_decode_points(cid, enc, out=(xy, st))
    elif form == "dev_np":
        _raw(ctx, ctx._lib.ellgpu_custom_decode_points_dev(ctx._ctx, cid, n, _ptr(enc), enc_len, _ptr(xy), _ptr(st),
                                                           None))
    else:
        xy, st = _torch_call(lambda i, o: ctx.custom_decode_points_dev(cid, i[0], o[0], o[1]), [enc], [xy, st])
    return xy, st


def run_wire(ctx, cid, h, der, lens, keys, bits=0, form="host", want_err=True):
    """-> (ok, err); err is None with want_err=False (out_err = NULL)"""
    h, der, keys = (np.ascontiguousarray(a, np.uint8) for a in (h, der, keys))
    lens = np.ascontiguousarray(lens, np.uint32)
    n = h.shape[0]
    ok, err = _filled((n,), (n,))
    if form == "host":
        ctx.custom_verify_wire(cid, h, (der, lens), keys, msg_bits=bits, out=(ok, err), want_err=want_err)
    elif form == "dev_np":
        _raw(ctx, ctx._lib.ellgpu_custom_verify_wire_dev(
            ctx._ctx, cid, n, _ptr(h), h.shape[1], int(bits), _ptr(der), der.shape[1], _ptr(lens), _ptr(keys),
            keys.shape[1], _ptr(ok), _ptr(err) if want_err else None, None))
    else:
        import torch
        dl = torch.from_numpy(lens.view(np.int32).copy()).cuda()          # (the four bytes of each length)
        ok, err = _torch_call(
            lambda i, o: ctx.custom_verify_wire_dev(cid, i[0], i[1], dl, i[2], o[0], out_err=o[1], msg_bits=bits),
            [h, der, keys], [ok, err if want_err else None])
    if not want_err:
        return ok, None
    return ok, err


# ---- the reference's recorded answers -----------------------------------------------------

def _rows(items):
    return np.stack([np.frombuffer(bytes.fromhex(x), np.uint8) for x in items])


def check_decode_golden(ctx, spec, form="host", cid=None):
    """every recorded decodePoint case, one call per encoding length, and the compressed ones once
    more through pointFromX (custom_decompress); returns the number of cases checked"""
    cid = define(ctx, spec) if cid is None else cid
    pl = spec["pl"]
    assert pl == (I(spec["p"]).bit_length() + 7) // 8
    groups = {}
    for c in spec["decode"]:
        groups.setdefault(len(c["enc"]) // 2, []).append(c)
    seen = set()
    for enc_len, cs in sorted(groups.items()):
        xy, st = run_decode(ctx, cid, _rows([c["enc"] for c in cs]), form)
        for i, c in enumerate(cs):
            what = (spec["name"], c["tag"], c["enc"], int(st[i]))
            assert st[i] == c["st"], what
            assert c["st"] == 0 or ERR_OF[c["msg"]] == c["st"], what
            want = b32(I(c["x"])).tobytes() + b32(I(c["y"])).tobytes() if c["st"] == 0 else bytes(64)
            assert xy[i].tobytes() == want, what
            seen.add(c["st"])
    comp = [c for c in spec["decode"] if len(c["enc"]) // 2 == 1 + pl and c["enc"][:2] in ("02", "03")]
    x = np.stack([b32(I(c["enc"][2:])) for c in comp])
    odd = np.array([c["enc"][:2] == "03" for c in comp], np.uint8)
    xy, st = run_decompress(ctx, cid, x, odd, form)
    for i, c in enumerate(comp):
        what = (spec["name"], "pointFromX", c["enc"], int(st[i]))
        assert st[i] == c["st"], what
        want = b32(I(c["x"])).tobytes() + b32(I(c["y"])).tobytes() if c["st"] == 0 else bytes(64)
        assert xy[i].tobytes() == want, what
    # a status-1 and a no-root case on every curve: 2 where p = 3 (mod 4), 3 otherwise
    assert {0, 1, 3} <= seen and ((2 in seen) == (I(spec["p"]) % 4 == 3))
    return len(spec["decode"]) + len(comp)


def check_wire_golden(ctx, spec, form="host", cid=None):
    """every recorded EC#verify(msg, der, key) case, one call per (digest length, msgBitLength, key
    length); a thrown message is its err code with verdict 0, an off-curve uncompressed key is
    verdict 0 / err 5 whatever the reference computed with it.  Returns the number of cases."""
    cid = define(ctx, spec) if cid is None else cid
    groups = {}
    for c in spec["wire"]:
        groups.setdefault((len(c["h"]) // 2, c["bits"], len(c["key"]) // 2), []).append(c)
    errs = set()
    for (hl, bits, kl), cs in sorted(groups.items()):
        der, lens = ctx._pack_records([bytes.fromhex(c["der"]) for c in cs])
        ok, err = run_wire(ctx, cid, _rows([c["h"] for c in cs]), der, lens, _rows([c["key"] for c in cs]), bits, form)
        for i, c in enumerate(cs):
            what = (spec["name"], c["tag"], c, int(ok[i]), int(err[i]))
            if "msg" in c:
                assert c["ok"] == 0 and ok[i] == 0 and err[i] == ERR_OF[c["msg"]], what
            elif c["tag"] == "key_off_curve":
                assert ok[i] == 0 and err[i] == OFF_CURVE, what
            else:
                assert ok[i] == c["ok"] and err[i] == 0, what
            errs.add(int(err[i]))
    p = I(spec["p"])
    assert errs == ({0, 1, 3, 4, 5} | ({2} if p % 4 == 3 else set())), errs
    return len(spec["wire"])


# ---- pointFromX / decodePoint over Python integers ------------------------------------------

def model_status(p, a, b, x):
    """ShortCurve#pointFromX's outcome for x (any integer: reduced mod p as toRed does):
    (status, rhs) -- 0 when rhs = x^3 + a x + b is 0 or a quadratic residue (Euler's criterion);
    else 'invalid point' (2) where Red#sqrt is one exponentiation (p = 3 mod 4) and 'Assertion
    failed' (3) where it is Tonelli-Shanks, whose loop stops at assert(i < m) for a non-residue"""
    x %= p
    rhs = (x * x * x + a * x + b) % p
    if rhs == 0 or pow(rhs, (p - 1) // 2, p) == 1:
        return 0, rhs
    return (2 if p % 4 == 3 else 3), rhs


def check_point(p, a, b, x, odd, xy, st, what):
    """one result of custom_decompress / a compressed custom_decode_points against the model"""
    want, rhs = model_status(p, a, b, x)
    assert st == want, what + (int(st), want)
    gx = int.from_bytes(xy[:32].tobytes(), "big")
    gy = int.from_bytes(xy[32:].tobytes(), "big")
    if want:
        assert gx == 0 and gy == 0, what
    else:
        # the root is fixed by its parity (y and p - y differ in it), except y = 0
        assert gx == x % p and gy < p and gy * gy % p == rhs and (gy == 0 or (gy & 1) == int(odd)), what


def random_xs(spec, n, seed):
    """n abscissae: uniform below 2^256 (above p wherever p is shorter: reduced by the engine), with
    0, 1, p - 1, p, p + 1 and 2^256 - 1 in front where n allows; and their parities"""
    p, a, b = pab(spec)
    rnd = random.Random(seed)
    xs = [rnd.getrandbits(256) for _ in range(n)]
    edge = [0, 1, p - 1, p, p + 1, (1 << 256) - 1]
    if n >= 2 * len(edge):
        xs[:len(edge)] = edge
    odd = [rnd.randrange(2) for _ in range(n)]
    return xs, odd


def check_random_decompress(ctx, spec, n, seed, form="host", cid=None):
    """custom_decompress on n random x against the model; returns the number of status-0 items"""
    cid = define(ctx, spec) if cid is None else cid
    p, a, b = pab(spec)
    xs, odd = random_xs(spec, n, seed)
    xy, st = run_decompress(ctx, cid, np.stack([b32(x) for x in xs]), np.array(odd, np.uint8), form)
    for i in range(n):
        check_point(p, a, b, xs[i], odd[i], xy[i], st[i], (spec["name"], n, i, hex(xs[i])))
    return int((st == 0).sum())


def check_random_decode(ctx, spec, n, seed, form="host", cid=None):
    """custom_decode_points on n compressed encodings of random x below 256^PL against the model"""
    cid = define(ctx, spec) if cid is None else cid
    p, a, b = pab(spec)
    pl = spec["pl"]
    rnd = random.Random(seed)
    xs = [rnd.getrandbits(8 * pl) for _ in range(n)]
    odd = [rnd.randrange(2) for _ in range(n)]
    enc = np.stack([np.frombuffer(bytes([2 + o]) + x.to_bytes(pl, "big"), np.uint8) for x, o in zip(xs, odd)])
    xy, st = run_decode(ctx, cid, enc, form)
    for i in range(n):
        check_point(p, a, b, xs[i], odd[i], xy[i], st[i], (spec["name"], "decode", n, i, hex(xs[i])))
    return int((st == 0).sum())


# ---- random wire batches ----------------------------------------------------------------

def der_int(v):
    b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
    return b"\x02" + bytes([len(b) + (b[0] >> 7)]) + (b"\x00" if b[0] & 0x80 else b"") + b


def der_sig(r, s):
    body = der_int(r) + der_int(s)
    assert len(body) < 0x80
    return b"\x30" + bytes([len(body)]) + body


# items 5..9 of every 40 carry a fault; the rest are the signatures of CD.random_batch
KEY_PREFIX, KEY_BAD, SIG_DER, KEY_OFF, R_WIDE = 5, 6, 7, 8, 9


def wire_batch(spec, n, seed):
    """n EC#verify items on the domain, in TWO encodings of the same signatures and keys:
    "compressed" (02 / 03 keys) and "full" (04 keys, every third one hybrid 06 / 07).  Signatures
    are CD.random_batch's (about half valid, the rest with r, s, the digest or the key disturbed),
    DER-encoded here.  Items 5..9 of every 40 carry a fault with a known answer:
      5  an unknown key prefix                                        -> err 1
      6  compressed: an x without a y                                 -> err 2 (p = 3 mod 4) / 3
         full: a hybrid prefix against y's parity                     -> err 3
      7  a DER signature with a wrong tag                             -> err 4
      8  full: y + 1, a key off the curve (r, s in range)             -> err 5   (compressed: none)
      9  r + 2^256, wider than 32 bytes                               -> verdict 0, err 0
    A call takes keys of ONE length, so no single call can show every code: a compressed key cannot
    be off the curve (5) and decodes with 2 or 3 according to p alone; an uncompressed one never
    lacks a y (2).  The two encodings together show every code that exists on the curve: 1..5 where
    p = 3 (mod 4), and 1, 3, 4, 5 where p = 1 (mod 4), on which the reference never answers
    'invalid point'.
    Returns a dict: h, r, s, q (the decoded rows), and per encoding (der, lens, keys, fault-derived
    expectations: err codes and the indices whose verdict is forced to 0)."""
    p, a, b, nn, gx, gy = CD.params(spec)
    pl = spec["pl"]
    h, r, s, q, expect = CD.random_batch(spec, n, seed)
    rnd = random.Random(seed + 1)
    no_y = None
    while no_y is None:
        x = rnd.randrange(p)
        if model_status(p, a, b, x)[0]:
            no_y = x
    out = {"h": h, "r": r, "s": s, "q": q, "known": np.array([e is not None for e in expect])}
    for form in ("compressed", "full"):
        ders, keys, err, zero = [], [], np.zeros(n, np.uint8), np.zeros(n, bool)
        for i in range(n):
            ri = int.from_bytes(r[i].tobytes(), "big")
            si = int.from_bytes(s[i].tobytes(), "big")
            qx = int.from_bytes(q[i, :32].tobytes(), "big")
            qy = int.from_bytes(q[i, 32:].tobytes(), "big")
            fault = i % 40
            sig = der_sig(ri, si)
            if form == "compressed":
                key = bytes([2 + (qy & 1)]) + qx.to_bytes(pl, "big")
            else:
                tag = 6 + (qy & 1) if i % 3 == 0 else 4
                key = bytes([tag]) + qx.to_bytes(pl, "big") + qy.to_bytes(pl, "big")
            if fault == KEY_PREFIX:
                key = b"\x05" + key[1:]
                err[i] = 1
            elif fault == KEY_BAD:
                if form == "compressed":
                    key = b"\x02" + no_y.to_bytes(pl, "big")
                    err[i] = 2 if p % 4 == 3 else 3
                else:
                    key = bytes([7 - (qy & 1)]) + key[1:]
                    err[i] = 3
            elif fault == SIG_DER:
                sig = b"\x31" + sig[1:]
                err[i] = 4
            elif fault == KEY_OFF and form == "full":
                key = b"\x04" + qx.to_bytes(pl, "big") + ((qy + 1) % p).to_bytes(pl, "big")
                err[i] = OFF_CURVE
            elif fault == R_WIDE:
                sig = der_sig(ri + (1 << 256), si)
                zero[i] = True
            ders.append(sig)
            keys.append(np.frombuffer(key, np.uint8))
        stride = max(len(d) for d in ders)
        der = np.zeros((n, stride), np.uint8)
        lens = np.zeros(n, np.uint32)
        for i, d in enumerate(ders):
            der[i, :len(d)] = np.frombuffer(d, np.uint8)
            lens[i] = len(d)
        out[form] = {"der": der, "lens": lens, "keys": np.stack(keys), "err": err, "zero": zero | (err != 0)}
    return out


def wire_reference(ctx, spec, batch, cid=None):
    """the verdicts of the decoded rows: ellgpu_ecdsa_verify (raw form) and the C oracle, which must
    agree; 1 where the signature is valid by construction"""
    cid = define(ctx, spec) if cid is None else cid
    raw = ctx.ecdsa_verify(cid, batch["h"], batch["r"], batch["s"], batch["q"])
    orc = CD.oracle_verify(spec, batch["h"], batch["r"], batch["s"], batch["q"])
    assert (raw == orc).all(), np.nonzero(raw != orc)[0][:10]
    assert (raw[batch["known"]] == 1).all()
    return raw


def check_wire_batch(ctx, spec, batch, want, n, form="host", want_err=True, cid=None):
    """the first n items of `batch` in both encodings: verdicts = `want` (wire_reference) except
    where a fault forces 0, err = the fault's code.  Returns the set of err codes seen."""
    cid = define(ctx, spec) if cid is None else cid
    p = I(spec["p"])
    seen = set()
    means = []
    for enc in ("compressed", "full"):
        e = batch[enc]
        ok, err = run_wire(ctx, cid, batch["h"][:n], e["der"][:n], e["lens"][:n], e["keys"][:n], 0, form, want_err)
        exp_ok = np.where(e["zero"][:n], 0, want[:n]).astype(np.uint8)
        assert set(np.unique(ok)) <= {0, 1}
        assert (ok == exp_ok).all(), (spec["name"], enc, n, np.nonzero(ok != exp_ok)[0][:10])
        if want_err:
            assert (err == e["err"][:n]).all(), (spec["name"], enc, n, np.nonzero(err != e["err"][:n])[0][:10])
            seen |= set(int(v) for v in err)
        means.append(float(ok.mean()))
    if n >= 257:
        # conditions, so that the test cannot pass on a batch that exercises nothing
        assert all(0.3 < m < 0.7 for m in means), means
        if want_err:
            assert seen == ({0, 1, 3, 4, 5} | ({2} if p % 4 == 3 else set())), seen
    return seen
