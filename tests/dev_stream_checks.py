"""Device-memory calls in flight on several streams: the operation table, the expected values and the
schedules that tests/test_dev_streams_gpu.py runs on the device and tests/test_dev_streams_hostsim.py
runs serially on the CPU build of the device code.

A call that takes device memory (`*_dev`, or a one-form call given ELLGPU_MEM_DEVICE) returns without
synchronising and works in the scratch of its stream's lane ("Two arenas").  Everything
here issues such calls WITHOUT a host synchronisation in between, from two or three streams, and asks
for the bytes the same call gives alone on the default stream.

OPS is the one list of the device-memory operations.  An entry builds D distinct items with the
generators and Python models of the existing *_checks.py modules (no model is written here); a batch
of m items repeats them (item i is item i % D), so the model's answer for every item of every batch is
known.  Each entry holds the faulty items its check module defines.

The two drivers hand in a platform: what a device buffer, a stream and a synchronisation are.  On the
device they are torch's; on the host simulation a buffer is a numpy array behind the few attributes
the bindings read, and there is one (null) stream -- that run proves the schedules, their operands and
their expected values, and raises no claim about ordering."""
import contextlib
import json
import os
import random
import re

import numpy as np

import elliptic_amd
from elliptic_amd.engine import FIELD_BYTES
from oracle import ec_oracle as O

import custom_domain_checks as CD
import custom_ecdh_checks as CH
import custom_ed_checks as CK
import custom_ed_ecdsa_checks as CE
import custom_mont_checks as CM
import custom_recover_checks as CR
import custom_sign_checks as CS
import custom_wire_checks as CW
import eddsa_verify_base_checks as EV
import fixed_base_checks as FB
import fixed_base_ed_checks as FE
import key_recid_checks as KR
import verify_base_checks as VB

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
D = 96                                     # distinct items per operation (no multiple of a wave's 64 lanes)
SIZES_256 = (100, 3000, 20000, 65536)      # secp256k1: the row, wave, lane, small-grid and full-grid forms
SIZES_SMALL = (100, 1500, 8192)            # p384 (the wide layer) and the user-defined ids
HOSTSIM_CAP = 96
REPS = 3
PRESETS = ("secp256k1", "p256", "p384")
SHORT_DOMAINS = ("brainpoolP256r1", "secp192k1")
EDWARDS, MONT, PLAIN = "curve1174", "m221", "cof_p10007"
OFF = 7                                    # the item whose key / point is moved off the curve (y ^ 1)
COMB_MAX_BYTES = 256 << 20                 # room for ed25519's 16-bit handle tables (134 MB); the 256-bit presets build
                                           # 16-bit tables, never the 22-bit one (1.6 GB)
COMB_MAX_BYTES_8 = 2 << 20                 # ... 8-bit tables (schedule 3)

# every `_dev` symbol and every `mem`-taking entry point of the recorded binding tables is either an
# operation of OPS or listed here.  What is listed claims no scratch slot: its chunk body (engine.h) is
# one launch on the caller's buffers, so it has nothing in a lane's arena to race on.  Every call whose
# chunk body claims a slot is in OPS.
EXCLUDED = {
    "ellgpu_sig_to_der_dev": "der_chunk: one FnSigToDer launch on the caller's buffers, claims no scratch slot",
    "ellgpu_sig_from_der_dev": "der_chunk: one FnSigFromDer launch on the caller's buffers, claims no scratch slot",
    "ellgpu_encode_points_dev": "codec_chunk OP_ENCODE: one FnEncodePoint launch on the caller's buffers, claims no scratch slot",
    "ellgpu_decode_points_dev": "codec_chunk OP_DECODE: one FnDecodePoint launch on the caller's buffers, claims no scratch slot",
    "ellgpu_custom_decompress_dev": "rt_wire_chunk OP_RT_DECOMPRESS: one FnRtDecompress launch, claims no scratch slot",
    "ellgpu_custom_decode_points_dev": "rt_wire_chunk OP_RT_DECODE: one FnRtDecodePoint launch, claims no scratch slot",
    "ellgpu_custom_encode_points_dev": "rt_encode_chunk: one FnRtEncodePoint launch, claims no scratch slot",
    "ellgpu_custom_ed_encode_points_dev": "edk_encode_chunk: one encoding launch on the caller's buffers, claims no scratch slot",
}


# ---- the platforms --------------------------------------------------------------------------------

class HostBuf:
    """a device buffer of the host simulation: a numpy array behind what the bindings read of a tensor"""

    def __init__(self, a):
        import torch
        assert isinstance(a, np.ndarray) and a.flags.c_contiguous
        self._a = a
        self.shape = a.shape
        self.dtype = torch.uint8 if a.dtype == np.uint8 else torch.int64
        self.device = torch.device("cuda", 0)

    def data_ptr(self):
        return self._a.ctypes.data

    def dim(self):
        return self._a.ndim

    def numel(self):
        return self._a.size

    def is_contiguous(self):
        return True


class HostsimPlatform:
    """device memory is host memory, every stream is the null stream, calls complete when they return"""
    gpu = False
    cap = HOSTSIM_CAP
    reps = 1                                   # a repetition asks about ordering alone: nothing to ask of a serial run

    def __init__(self, lib):
        self.lib = lib

    def context(self):
        c = elliptic_amd.Context(0, lib_path=self.lib)
        c._stream = lambda: None
        return c

    def put(self, a):
        return HostBuf(np.ascontiguousarray(a).copy())

    def zeros(self, shape):
        return HostBuf(np.zeros(shape, np.uint8))

    def get(self, t):
        return t._a.copy()

    def zero(self, t):
        t._a[...] = 0

    def copy_into(self, dst, src):
        np.copyto(dst._a, src._a)

    def clone(self, t):
        return HostBuf(t._a.copy())

    def streams(self, k):
        return [None] * k

    def on(self, stream):
        return contextlib.nullcontext()

    def sync(self):
        pass


class TorchPlatform:
    gpu = True
    cap = None
    reps = REPS

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)

    def context(self):
        return elliptic_amd.Context(0)

    def put(self, a):
        if a.dtype == np.uint32:
            a = a.view(np.int32)                      # (the four bytes of each length)
        elif a.dtype == np.uint64:
            a = a.view(np.int64)
        return self.torch.from_numpy(np.ascontiguousarray(a).copy()).to(self.dev)

    def zeros(self, shape):
        return self.torch.zeros(shape, dtype=self.torch.uint8, device=self.dev)

    def get(self, t):
        return t.cpu().numpy()

    def zero(self, t):
        t.zero_()

    def copy_into(self, dst, src):
        dst.copy_(src, non_blocking=True)

    def clone(self, t):
        return t.clone()

    def streams(self, k):
        return [self.torch.cuda.Stream(device=self.dev) for _ in range(k)]

    def on(self, stream):
        return contextlib.nullcontext() if stream is None else self.torch.cuda.stream(stream)

    def sync(self):
        self.torch.cuda.synchronize()


@contextlib.contextmanager
def environ(**kv):
    """tuning overrides are read when a context is created"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Cx:
    """a context with the curve ids and handles the operations have defined on it"""

    def __init__(self, P, comb_max_bytes=None):
        self.P = P
        if P.gpu and comb_max_bytes:
            with environ(ELLGPU_COMB_MAX_BYTES=comb_max_bytes):
                self.ctx = P.context()
        else:
            self.ctx = P.context()
        self.made = {}

    def get(self, key, make):
        if key not in self.made:
            self.made[key] = make(self.ctx)
        return self.made[key]

    def close(self):
        self.ctx.close()


# ---- the operations -------------------------------------------------------------------------------

class Ragged:
    """messages of several lengths: a flat buffer and n + 1 offsets"""

    def __init__(self, msgs):
        self.msgs = list(msgs)

    def take(self, m):
        msgs = [self.msgs[i % len(self.msgs)] for i in range(m)]
        return EV.pack(msgs)


class Op:
    """one device-memory operation.  symbols: what it covers of the binding tables; sizes: the batch
    sizes it cycles through; ins: name -> (D, ...) array, Ragged or None; outs: the results' shapes
    without the item count; model: the model's answer per result, (D, ...) arrays (None: no model for
    that result); faulty: class -> index of an item of that class; prepare(cx) defines what the call
    needs on a context; call(cx, I, O) issues it on the current stream."""

    def __init__(self, name, symbols, curve, sizes, ins, outs, model, faulty, call, prepare=None):
        self.name, self.symbols, self.curve, self.sizes = name, tuple(symbols), curve, sizes
        self.ins, self.outs, self.model, self.faulty = ins, outs, model, faulty
        self.call, self.prepare = call, prepare or (lambda cx: None)
        assert len(outs) == len(model)
        for a in model:
            assert a is None or a.shape[0] == D, (name, a.shape)
        for a in ins.values():
            assert a is None or isinstance(a, Ragged) or a.shape[0] == D, name

    def operands(self, m):
        """the numpy operands of a batch of m items"""
        idx = np.arange(m) % D
        out = {}
        for k, a in self.ins.items():
            if isinstance(a, Ragged):
                out[k], out[k + "_off"] = a.take(m)
            else:
                out[k] = None if a is None else np.ascontiguousarray(a[idx])
        return out

    def model_for(self, m):
        idx = np.arange(m) % D
        return [None if a is None else a[idx] for a in self.model]

    def out_shapes(self, m):
        return [(m,) + tuple(s) for s in self.outs]


def _rows(vals, B):
    return FB.rows(vals, B)


def _off_curve(row):
    r = row.copy()
    r[-1] ^= 1
    return r


def _tile(row):
    return np.ascontiguousarray(np.broadcast_to(row, (D, row.shape[0])))


def _xy_of(P, B):
    return np.frombuffer(FB.xy_bytes(P, B), np.uint8)


def preset_ops(curve):
    B = FIELD_BYTES[curve]
    sizes = SIZES_256 if B == 32 else SIZES_SMALL
    spec, m, C = FB.spec_of(curve), FB.model_of(FB.spec_of(curve)), O.get_curve(curve)
    pts = FB.bases_of(spec)
    bt = FB.random_batch(spec, D, 31)
    assert FB.model_meets_conditions(spec, bt)
    ks, k1, k2 = bt["ints"]
    ops = []

    # k G: the scalars 0 and n give the point at infinity
    fixed = [FB.answer(R, B) for R in m.mul_many(ks, pts[0], 8 * B)]
    fxy, finf = np.stack([x for x, _ in fixed]), np.array([f for _, f in fixed], np.uint8)
    assert finf[0] == 1 and finf[1] == 1 and not finf[2:].any()
    ops.append(Op("mul_fixed_dev", ["ellgpu_mul_fixed_dev"], curve, sizes, {"k": bt["k"]}, [(2 * B,), ()], [fxy, finf],
                  {"infinity": 0}, lambda cx, I, Q: cx.ctx.mul_fixed_dev(curve, I["k"], Q[0], Q[1])))

    # k P on the fixture's base 3, one point off the curve: status 2 beside a zeroed result
    P3 = _tile(_xy_of(pts[3], B)).copy()
    P3[OFF] = _off_curve(P3[OFF])
    vxy, vinf = bt["xy"].copy(), bt["inf"].copy()
    vxy[OFF], vinf[OFF] = 0, elliptic_amd.STATUS_OFF_CURVE
    ops.append(Op("mul_var_dev", ["ellgpu_mul_var_dev"], curve, sizes, {"k": bt["k"], "p": P3}, [(2 * B,), ()], [vxy, vinf],
                  {"infinity": 0, "off_curve": OFF},
                  lambda cx, I, Q: cx.ctx.mul_var_dev(curve, I["k"], I["p"], Q[0], Q[1])))

    # k1 G + k2 (-G), with P1 = G given and with p1 = None
    P0, P2 = _tile(_xy_of(pts[0], B)), _tile(_xy_of(pts[2], B)).copy()
    P2[OFF] = _off_curve(P2[OFF])
    axy, ainf = bt["xy2"].copy(), bt["inf2"].copy()
    axy[OFF], ainf[OFF] = 0, elliptic_amd.STATUS_OFF_CURVE
    for with_p1 in (True, False):
        ops.append(Op("mul_add2_dev" + ("" if with_p1 else "[p1=None]"), ["ellgpu_mul_add2_dev"], curve, sizes,
                      {"k1": bt["k1"], "p1": P0 if with_p1 else None, "k2": bt["k2"], "p2": P2}, [(2 * B,), ()], [axy, ainf],
                      {"infinity": 0, "doubling": 1, "off_curve": OFF},
                      lambda cx, I, Q: cx.ctx.mul_add2_dev(curve, I["k1"], I["p1"], I["k2"], I["p2"], Q[0], Q[1])))

    # EC#verify by one key: u1 = 0, R = O, r = n, tampered r / s / hash, and a key off the curve
    vspec = VB.spec_of(curve)
    vb = VB.random_batch(vspec, D, 32)
    assert VB.batch_meets_conditions(vspec, vb)
    pub = _tile(vb["pub"]).copy()
    pub[OFF] = _off_curve(pub[OFF])
    assert vb["kinds"][OFF] == "valid" and vb["want"][OFF] == 1
    vok, vst = vb["want"].copy(), np.zeros(D, np.uint8)
    vok[OFF], vst[OFF] = 0, elliptic_amd.STATUS_OFF_CURVE
    vfaulty = {"u1_zero": 0, "sum_inf": 1, "r_range": 2, "off_curve": OFF}
    vfaulty.update({"flip_" + k: vb["kinds"].index(k) for k in ("r", "s", "hash")})
    ops.append(Op("ecdsa_verify_dev", ["ellgpu_ecdsa_verify_dev"], curve, sizes,
                  {"h": vb["h"], "r": vb["r"], "s": vb["s"], "pub": pub}, [(), ()], [vok, vst], vfaulty,
                  lambda cx, I, Q: cx.ctx.ecdsa_verify_dev(curve, I["h"], I["r"], I["s"], I["pub"], Q[0], out_status=Q[1])))

    # the same signatures as DER with SEC1 keys: an unknown key prefix (err 1) and a wrong DER tag (err 4)
    hs, rs, ss = vb["ints"]
    ders = [CW.der_sig(r, s) for r, s in zip(rs, ss)]
    key = b"\x04" + vb["pub"].tobytes()
    keys = [key] * D
    wok, werr = vb["want"].copy(), np.zeros(D, np.uint8)
    keys[5], wok[5], werr[5] = b"\x05" + key[1:], 0, 1
    ders[8], wok[8], werr[8] = b"\x31" + ders[8][1:], 0, 4
    der, lens = elliptic_amd.Context._pack_records(ders)
    ops.append(Op("ecdsa_verify_wire_dev", ["ellgpu_ecdsa_verify_wire_dev"], curve, sizes,
                  {"h": vb["h"], "der": der, "lens": lens, "keys": np.stack([np.frombuffer(k, np.uint8) for k in keys])},
                  [(), ()], [wok, werr], {"u1_zero": 0, "sum_inf": 1, "r_range": 2, "key_prefix": 5, "sig_der": 8},
                  lambda cx, I, Q: cx.ctx.ecdsa_verify_wire_dev(curve, I["h"], I["der"], I["lens"], I["keys"], Q[0], out_err=Q[1])))

    # EC#sign with the reference's own nonces; every fourth key is any value of the width (reduced mod n)
    rng = random.Random("dev-streams:sign:" + curve)
    sh = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(D)]
    sd = [rng.getrandbits(8 * B) if i % 4 == 3 else rng.randrange(1, C.n) for i in range(D)]
    sig = [O.ecdsa_sign_det(C, curve, int.from_bytes(h, "big"), 32, d % C.n, True) for h, d in zip(sh, sd)]
    ops.append(Op("ecdsa_sign_det_dev", ["ellgpu_ecdsa_sign_det_dev"], curve, sizes,
                  {"h": np.stack([np.frombuffer(h, np.uint8) for h in sh]), "d": _rows(sd, B)}, [(B,), (B,), (), ()],
                  [_rows([g[0] for g in sig], B), _rows([g[1] for g in sig], B), np.array([g[2] for g in sig], np.uint8),
                   np.ones(D, np.uint8)], {"key_above_n": 3},
                  lambda cx, I, Q: cx.ctx.ecdsa_sign_det_dev(curve, I["h"], I["d"], Q[0], Q[1], Q[2], Q[3], canonical=True)))

    # EC#recoverPubKey on the recovery-id batch: the id the model found where there is one, else i % 4
    kb = KR.random_batch(curve, D, 33)
    assert KR.meets_conditions(kb)
    j = np.where(kb.status == 0, kb.recid, np.arange(D) % 4).astype(np.uint8)
    rxy, rst = np.zeros((D, 2 * B), np.uint8), np.zeros(D, np.uint8)
    for i in range(D):
        r, s = int.from_bytes(kb.r[i].tobytes(), "big"), int.from_bytes(kb.s[i].tobytes(), "big")
        if r == 0 or r >= C.n:
            rst[i] = 3
            continue
        try:
            Q_ = O.ecdsa_recover(C, int.from_bytes(kb.h[i].tobytes(), "big"), r, s, int(j[i]))
        except ValueError:
            rst[i] = 2
            continue
        if Q_.inf:
            rst[i] = 1
        else:
            rxy[i] = _xy_of((Q_.x, Q_.y), B)
    assert {0, 3} <= set(rst.tolist())
    rfaulty = {"outside": int(np.nonzero(rst == 3)[0][0])}
    if (rst == 2).any():
        rfaulty["throws"] = int(np.nonzero(rst == 2)[0][0])
    ops.append(Op("ecdsa_recover_dev", ["ellgpu_ecdsa_recover_dev"], curve, sizes, {"h": kb.h, "r": kb.r, "s": kb.s, "j": j},
                  [(2 * B,), ()], [rxy, rst], rfaulty,
                  lambda cx, I, Q: cx.ctx.ecdsa_recover_dev(curve, I["h"], I["r"], I["s"], I["j"], Q[0], Q[1])))

    # ... and its recovery id in one pass: every id, the key off the curve, r and s outside the domain
    kfaulty = {t: int(np.nonzero(kb.status == v)[0][0]) for t, v in KR.STATUS_OF.items()}
    ops.append(Op("ecdsa_recid", ["ellgpu_ecdsa_recid"], curve, sizes, {"h": kb.h, "r": kb.r, "s": kb.s, "pub": kb.pub},
                  [(), ()], [kb.recid.astype(np.uint8), kb.status.astype(np.uint8)], kfaulty,
                  lambda cx, I, Q: cx.ctx.ecdsa_recid(curve, I["h"], I["r"], I["s"], I["pub"], out=(Q[0], Q[1]))))

    # pointFromX on the abscissae of k G, with one x that has no point
    good = [i for i in range(D) if not finf[i]]
    src = np.array([good[i % len(good)] for i in range(D)])
    x, odd = np.ascontiguousarray(fxy[src, :B]), np.ascontiguousarray(fxy[src, -1] & 1)
    dxy, dok = fxy[src].copy(), np.ones(D, np.uint8)
    no_y = next(v for v in range(1, 64) if CW.model_status(m.p, m.a, m.b, v)[0])
    x[4], dxy[4], dok[4] = _rows([no_y], B)[0], 0, 0
    ops.append(Op("decompress_dev", ["ellgpu_decompress_dev"], curve, sizes, {"x": x, "odd": odd}, [(2 * B,), ()], [dxy, dok],
                  {"no_point": 4}, lambda cx, I, Q: cx.ctx.decompress_dev(curve, I["x"], I["odd"], Q[0], Q[1])))

    # KeyPair#validate with the order test (n P through the variable-base ladder): a flagged infinity
    # and a point off the curve
    Fp, Vp = m.mul_many(ks, pts[0], 8 * B), m.mul_many(ks, pts[3], 8 * B)
    A = [Fp[i] for i in src]
    vxy2, flags, wst = np.stack([_xy_of(P, B) for P in A]), np.zeros(D, np.uint8), np.zeros(D, np.uint8)
    vxy2[OFF], wst[OFF] = _off_curve(vxy2[OFF]), 2
    flags[9], wst[9] = 1, 1
    assert all(m.on_curve(P) for P in A) and m.mul(C.n, A[0]) is None and m.mul(C.n, A[50]) is None
    ops.append(Op("validate_dev", ["ellgpu_validate_dev"], curve, sizes, {"xy": vxy2, "inf": flags}, [()], [wst],
                  {"flagged_infinity": 9, "off_curve": OFF},
                  lambda cx, I, Q: cx.ctx.validate_dev(curve, I["xy"], I["inf"], True, Q[0])))

    # Point#add: a doubling, P + (-P), and the point at infinity as an operand
    Bp = list(Vp)
    Bp[5], Bp[6] = A[5], m.neg(A[6])
    inf2 = np.array([1 if P is None else 0 for P in Bp], np.uint8)
    assert inf2[0] == 1 and inf2[1] == 1 and not inf2[2:].any()
    sums = [FB.answer(m.add(P, Q_), B) for P, Q_ in zip(A, Bp)]
    sinf = np.array([f for _, f in sums], np.uint8)
    assert sinf[6] == 1 and sinf.sum() == 1
    ops.append(Op("point_add_dev", ["ellgpu_point_add_dev"], curve, sizes,
                  {"xy1": np.stack([_xy_of(P, B) for P in A]), "xy2": np.stack([FB.answer(P, B)[0] for P in Bp]), "inf2": inf2},
                  [(2 * B,), ()], [np.stack([x for x, _ in sums]), sinf], {"operand_infinity": 0, "doubling": 5, "infinity": 6},
                  lambda cx, I, Q: cx.ctx.point_add_dev(curve, I["xy1"], I["xy2"], Q[0], Q[1], inf2=I["inf2"])))

    # one pass of EC#sign for supplied nonces: k = 0 and k = 1 are refused
    gd = [rng.randrange(1, C.n) for _ in range(D)]
    nonce = [rng.randrange(2, C.n - 1).to_bytes(B, "big") for _ in range(D)]
    nonce[1], nonce[2] = bytes(B), (1).to_bytes(B, "big")
    one = [O.ecdsa_sign(C, int.from_bytes(h, "big"), 32, d, k, True) for h, d, k in zip(sh, gd, nonce)]
    assert one[1] is None and one[2] is None and sum(g is None for g in one) == 2
    z = lambda i: [0 if g is None else g[i] for g in one]  # noqa: E731
    ops.append(Op("ecdsa_sign_dev", ["ellgpu_ecdsa_sign_dev"], curve, sizes,
                  {"h": np.stack([np.frombuffer(h, np.uint8) for h in sh]), "d": _rows(gd, B),
                   "k": np.stack([np.frombuffer(k, np.uint8) for k in nonce])}, [(B,), (B,), (), ()],
                  [_rows(z(0), B), _rows(z(1), B), np.array(z(2), np.uint8), np.array([g is not None for g in one], np.uint8)],
                  {"nonce_refused": 1},
                  lambda cx, I, Q: cx.ctx.ecdsa_sign_dev(curve, I["h"], I["d"], I["k"], Q[0], Q[1], Q[2], Q[3], canonical=True)))

    # fixed-base handles: k B3, k1 G + k2 (-G) and EC#verify against the key's table
    if curve != "p384":
        def prep(cx):
            # 8-bit tables, and the walked base at 16 bits where a device builds the table
            cx.get(("bases", curve), lambda ctx: [ctx.define_base(curve, FB.xy_bytes(P, B), 16 if i == 3 and cx.P.gpu else 8)
                                                  for i, P in enumerate(pts[:4])])
        ops.append(Op("mul_base", ["ellgpu_mul_base"], curve, sizes, {"k": bt["k"]}, [(2 * B,), ()], [bt["xy"], bt["inf"]],
                      {"infinity": 0}, lambda cx, I, Q: cx.ctx.mul_base(cx.made[("bases", curve)][3], I["k"], out=(Q[0], Q[1])),
                      prep))
        ops.append(Op("mul_base2", ["ellgpu_mul_base2"], curve, sizes, {"k1": bt["k1"], "k2": bt["k2"]}, [(2 * B,), ()],
                      [bt["xy2"], bt["inf2"]], {"infinity": 0, "doubling": 1},
                      lambda cx, I, Q: cx.ctx.mul_base2(cx.made[("bases", curve)][0], cx.made[("bases", curve)][2], I["k1"],
                                                        I["k2"], out=(Q[0], Q[1])), prep))

        def vprep(cx):
            cx.get(("key", curve), lambda ctx: ctx.define_base(curve, vb["pub"].tobytes(), 8))
        ops.append(Op("ecdsa_verify_base", ["ellgpu_ecdsa_verify_base"], curve, sizes, {"h": vb["h"], "r": vb["r"], "s": vb["s"]},
                      [()], [vb["want"]], {k: v for k, v in vfaulty.items() if k != "off_curve"},
                      lambda cx, I, Q: cx.ctx.ecdsa_verify_base(cx.made[("key", curve)], I["h"], I["r"], I["s"], out=(Q[0],)),
                      vprep))
    return ops


def ed25519_ops():
    c, key = O.get_curve("ed25519"), "aG1"
    eb = EV.random_batch(D, 34, key)
    assert EV.batch_meets_conditions(eb)
    ok, err = eb["want"]
    faulty = {k: eb["kinds"].index(k) for k in ("S_n", "undecodable", "noncanon", "S_zero", "R", "S", "M")}
    msgs = Ragged(eb["msgs"])
    ops = [Op("eddsa_verify_dev", ["ellgpu_eddsa_verify_dev"], "ed25519", SIZES_256,
              {"msgs": msgs, "sigs": eb["sigs"], "pubs": _tile(eb["enc"])}, [(), ()], [ok, err], faulty,
              lambda cx, I, Q: cx.ctx.eddsa_verify_dev(I["msgs"], 0, I["sigs"], I["pubs"], Q[0], Q[1], msg_off=I["msgs_off"]))]

    def kprep(cx):
        cx.get(("edkey", key), lambda ctx: EV.define_key(ctx, key))
    ops.append(Op("eddsa_verify_base", ["ellgpu_eddsa_verify_base"], "ed25519", SIZES_256, {"msgs": msgs, "sigs": eb["sigs"]},
                  [(), ()], [ok, err], faulty,
                  lambda cx, I, Q: cx.ctx.eddsa_verify_base(cx.made[("edkey", key)], I["msgs"], I["sigs"], msg_off=I["msgs_off"],
                                                            out=(Q[0], Q[1])), kprep))

    rng = random.Random("dev-streams:eddsa-sign")
    secrets = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(D)]
    m2 = [bytes(rng.getrandbits(8) for _ in range(17)) for _ in range(D)]
    made = [O.eddsa_sign(c, m, s) for m, s in zip(m2, secrets)]
    rows = lambda bs: np.stack([np.frombuffer(b, np.uint8) for b in bs])  # noqa: E731
    ops.append(Op("eddsa_sign_dev", ["ellgpu_eddsa_sign_dev"], "ed25519", SIZES_256, {"secrets": rows(secrets), "msgs": rows(m2)},
                  [(64,), (32,)], [rows([g[0] for g in made]), rows([g[1] for g in made])], {},
                  lambda cx, I, Q: cx.ctx.eddsa_sign_dev(I["secrets"], I["msgs"], 17, Q[0], Q[1])))

    # k B3 and k1 G + k2 (-G) on handles of ed25519: the identity, and the law's doubling branch
    spec = FE.spec_of("ed25519")
    fm, pts = FE.model_of(spec), FE.bases_of(spec)
    fb = FE.random_batch(spec, D, 35)
    assert FE.model_meets_conditions(spec, fb)
    ks, k1, k2 = fb["ints"]
    one = [FE.answer(spec, fm.mul(k, pts[3])) for k in ks]
    two = [FE.answer(spec, fm.mul2(a, pts[0], b, pts[2])) for a, b in zip(k1, k2)]

    def prep(cx):
        cx.get(("edbases",), lambda ctx: FE.define_bases(ctx, spec, 0, "ed25519", which=(0, 2, 3))[1])
    ops.append(Op("mul_base[ed25519]", ["ellgpu_mul_base"], "ed25519", SIZES_256, {"k": fb["k"]}, [(64,), ()],
                  [np.stack([x for x, _ in one]), np.array([f for _, f in one], np.uint8)], {"identity": 0},
                  lambda cx, I, Q: cx.ctx.mul_base(cx.made[("edbases",)][3], I["k"], out=(Q[0], Q[1])), prep))
    ops.append(Op("mul_base2[ed25519]", ["ellgpu_mul_base2"], "ed25519", SIZES_256, {"k1": fb["k1"], "k2": fb["k2"]}, [(64,), ()],
                  [np.stack([x for x, _ in two]), np.array([f for _, f in two], np.uint8)], {"identity": 0, "doubling": 1},
                  lambda cx, I, Q: cx.ctx.mul_base2(cx.made[("edbases",)][0], cx.made[("edbases",)][2], I["k1"], I["k2"],
                                                    out=(Q[0], Q[1])), prep))

    # the x25519 ladder: x = 0 ends at infinity (the derive call has no device-memory form)
    from oracle import c_oracle
    k = rows([bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(D)])
    x = rows([bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(D)])
    x[1] = 0
    wx, winf = c_oracle.mont_mul(k, x)
    assert winf[1] == 1 and not winf[2:].all()
    ops.append(Op("x25519_dev", ["ellgpu_x25519_ladder_dev"], "curve25519", SIZES_256, {"k": k, "x": x}, [(32,), ()],
                  [np.asarray(wx, np.uint8).reshape(D, 32), np.asarray(winf, np.uint8)], {"infinity": 1},
                  lambda cx, I, Q: cx.ctx.x25519_dev(I["k"], I["x"], Q[0], Q[1])))
    return ops


def short_domain_ops(name):
    key = ("short", name)

    def prep(cx):
        cx.get(key, lambda ctx: CW.define(ctx, CW.spec_of(name)))
    cid = lambda cx: cx.made[key]  # noqa: E731
    ops = []

    wspec = CW.spec_of(name)
    wb = CW.wire_batch(wspec, D, 36)
    full = wb["full"]
    ok = np.where(full["zero"], 0, CD.oracle_verify(wspec, wb["h"], wb["r"], wb["s"], wb["q"])).astype(np.uint8)
    assert set(full["err"].tolist()) >= {0, 1, 3, 4, CW.OFF_CURVE} and set(ok.tolist()) == {0, 1}
    ops.append(Op("custom_verify_wire_dev", ["ellgpu_custom_verify_wire_dev"], name, SIZES_SMALL,
                  {"h": wb["h"], "der": full["der"], "lens": full["lens"], "keys": full["keys"]}, [(), ()], [ok, full["err"]],
                  {"key_prefix": CW.KEY_PREFIX, "key_parity": CW.KEY_BAD, "sig_der": CW.SIG_DER, "off_curve": CW.KEY_OFF,
                   "r_wide": CW.R_WIDE},
                  lambda cx, I, Q: cx.ctx.custom_verify_wire_dev(cid(cx), I["h"], I["der"], I["lens"], I["keys"], Q[0], out_err=Q[1]),
                  prep))

    rb = CR.random_batch(CR.spec_of(name), D, 37)
    assert {0, 2, 3} <= set(rb["st"].tolist())
    ops.append(Op("custom_recover_dev", ["ellgpu_custom_recover_dev"], name, SIZES_SMALL,
                  {"h": rb["h"], "r": rb["r"], "s": rb["s"], "j": rb["j"]}, [(64,), ()], [rb["xy"], rb["st"]],
                  {"throws": int(np.nonzero(rb["st"] == 2)[0][0]), "outside": int(np.nonzero(rb["st"] == 3)[0][0])},
                  lambda cx, I, Q: cx.ctx.custom_recover_dev(cid(cx), I["h"], I["r"], I["s"], I["j"], Q[0], Q[1]), prep))

    sb = CS.det_batch(CS.spec_of(name), D, 38, "sha256", 32, 1)
    ops.append(Op("custom_sign_det_dev", ["ellgpu_custom_sign_det_dev"], name, SIZES_SMALL, {"h": sb["h"], "d": sb["d"]},
                  [(32,), (32,), (), ()], [sb["r"], sb["s"], sb["j"], sb["ok"]], {"key_any_value": 3},
                  lambda cx, I, Q: cx.ctx.custom_sign_det_dev(cid(cx), I["h"], I["d"], Q[0], Q[1], Q[2], Q[3], canonical=True),
                  prep))

    hb = CH.random_batch(CH.spec_of(name), D, 39)
    assert set(hb["st"].tolist()) == {0, 1, 2}
    ops.append(Op("custom_derive_dev", ["ellgpu_custom_derive_dev"], name, SIZES_SMALL, {"priv": hb["priv"], "pub": hb["pub"]},
                  [(32,), ()], [hb["x"], hb["st"]],
                  {"not_validated": int(np.nonzero(hb["st"] == 1)[0][0]), "infinity": int(np.nonzero(hb["st"] == 2)[0][0])},
                  lambda cx, I, Q: cx.ctx.custom_derive_dev(cid(cx), I["priv"], I["pub"], Q[0], Q[1]), prep))
    assert set(hb["vst"].tolist()) >= {0, 1, 2}
    ops.append(Op("custom_validate_dev", ["ellgpu_custom_validate_dev"], name, SIZES_SMALL, {"xy": hb["pub"], "inf": hb["inf"]},
                  [()], [hb["vst"]], {"flagged_infinity": 2, "not_a_point": int(np.nonzero(hb["vst"] == 2)[0][0])},
                  lambda cx, I, Q: cx.ctx.custom_validate_dev(cid(cx), I["xy"], I["inf"], True, Q[0]), prep))

    enc, wst, wx, werr = CH.wire_batch(CH.spec_of(name), hb, D, True)
    assert {0, 3} <= set(wst.tolist()) and werr[5] == 1 and werr[11] in (2, 3)
    ops.append(Op("custom_derive_wire_dev", ["ellgpu_custom_derive_wire_dev"], name, SIZES_SMALL, {"priv": hb["priv"], "enc": enc},
                  [(32,), (), ()], [wx, wst, werr], {"key_prefix": 5, "no_root": 11},
                  lambda cx, I, Q: cx.ctx.custom_derive_wire_dev(cid(cx), I["priv"], I["enc"], Q[0], Q[1], Q[2]), prep))

    ub = CS.sup_batch(CS.spec_of(name), D, 43, 32, 1)
    ops.append(Op("custom_sign_dev", ["ellgpu_custom_sign_dev"], name, SIZES_SMALL, {"h": ub["h"], "d": ub["d"], "k": ub["k"]},
                  [(32,), (32,), (), ()], [ub["r"], ub["s"], ub["j"], ub["ok"]], {"nonce_low": 0, "nonce_high": 1, "s_zero": 2},
                  lambda cx, I, Q: cx.ctx.custom_sign_dev(cid(cx), I["h"], I["d"], I["k"], Q[0], Q[1], Q[2], Q[3], canonical=True),
                  prep))
    return ops


def other_custom_ops():
    ops = []
    espec = CE.spec_of(EDWARDS)
    eb = CE.verify_batch(espec, D, 40, distinct=D)
    assert CE.verify_batch_meets_conditions(espec, eb)
    kinds = eb["kind"].tolist()

    def eprep(cx):
        cx.get(("edwards", EDWARDS), lambda ctx: CE.define(ctx, espec))
    ops.append(Op("custom_ed_verify_dev", ["ellgpu_custom_ed_verify_dev"], EDWARDS, SIZES_SMALL,
                  {"h": eb["h"], "r": eb["r"], "s": eb["s"], "q": eb["q"]}, [(), ()], [eb["ok"], eb["st"]],
                  {k: kinds.index(k) for k in CE.FAILURES},
                  lambda cx, I, Q: cx.ctx.custom_ed_verify_dev(cx.made[("edwards", EDWARDS)], I["h"], I["r"], I["s"], I["q"], Q[0],
                                                               out_status=Q[1]), eprep))

    mspec = CM.spec_of(MONT)
    mb = CM.random_batch(mspec, D, 41)
    assert CM.model_meets_conditions(mb, D)

    def mprep(cx):
        cx.get(("mont", MONT), lambda ctx: CM.define(ctx, mspec))
    ops.append(Op("custom_mont_ladder_dev", ["ellgpu_custom_mont_ladder_dev"], MONT, SIZES_SMALL, {"k": mb["k"], "x": mb["x"]},
                  [(32,), ()], [mb["ox"], mb["inf"]], {"infinity": int(np.nonzero(mb["inf"])[0][0])},
                  lambda cx, I, Q: cx.ctx.custom_mont_ladder_dev(cx.made[("mont", MONT)], I["k"], I["x"], Q[0], Q[1]), mprep))

    ed = lambda cx: cx.made[("edwards", EDWARDS)]  # noqa: E731
    db = CE.det_batch(espec, D, 44, "sha256", 32, 1, distinct=D)
    ops.append(Op("custom_ed_sign_det_dev", ["ellgpu_custom_ed_sign_det_dev"], EDWARDS, SIZES_SMALL, {"h": db["h"], "d": db["d"]},
                  [(32,), (32,), (), ()], [db["r"], db["s"], db["j"], db["ok"]], {},
                  lambda cx, I, Q: cx.ctx.custom_ed_sign_det_dev(ed(cx), I["h"], I["d"], Q[0], Q[1], Q[2], Q[3], canonical=True),
                  eprep))
    ub = CE.sup_batch(espec, D, 45, 32, 1, distinct=D)
    assert set(ub["ok"].tolist()) == {0, 1}
    ops.append(Op("custom_ed_sign_dev", ["ellgpu_custom_ed_sign_dev"], EDWARDS, SIZES_SMALL, {"h": ub["h"], "d": ub["d"], "k": ub["k"]},
                  [(32,), (32,), (), ()], [ub["r"], ub["s"], ub["j"], ub["ok"]], {"nonce_refused": int(np.nonzero(ub["ok"] == 0)[0][0])},
                  lambda cx, I, Q: cx.ctx.custom_ed_sign_dev(ed(cx), I["h"], I["d"], I["k"], Q[0], Q[1], Q[2], Q[3], canonical=True),
                  eprep))
    kb = CK.random_batch(CK.spec_of(EDWARDS), D, 46, distinct=D)
    assert CK.model_meets_conditions(kb, D)
    first = lambda a, v: int(np.nonzero(a == v)[0][0])  # noqa: E731
    for f, from_y in (("fx", False), ("fy", True)):
        ops.append(Op("custom_ed_decompress_dev[%s]" % f, ["ellgpu_custom_ed_decompress_dev"], EDWARDS, SIZES_SMALL,
                      {"v": kb["v"], "odd": kb["odd"]}, [(64,), ()], [kb[f + "_xy"], kb[f + "_st"]],
                      {"no_root": first(kb[f + "_st"] != 0, True)},
                      lambda cx, I, Q, from_y=from_y: cx.ctx.custom_ed_decompress_dev(ed(cx), I["v"], I["odd"], from_y, Q[0], Q[1]),
                      eprep))
    ops.append(Op("custom_ed_validate_dev", ["ellgpu_custom_ed_validate_dev"], EDWARDS, SIZES_SMALL, {"xy": kb["xy"]}, [()],
                  [kb["valo"]], {"identity": first(kb["val"], 1), "not_a_point": first(kb["val"], 2)},
                  lambda cx, I, Q: cx.ctx.custom_ed_validate_dev(ed(cx), I["xy"], kb["order"], Q[0]), eprep))
    ops.append(Op("custom_ed_derive_dev", ["ellgpu_custom_ed_derive_dev"], EDWARDS, SIZES_SMALL, {"k": kb["k"], "xy": kb["xy"]},
                  [(32,), ()], [kb["dx"], kb["dst"]], {"not_validated": first(kb["dst"], 1)},
                  lambda cx, I, Q: cx.ctx.custom_ed_derive_dev(ed(cx), I["k"], I["xy"], Q[0], Q[1]), eprep))
    w = kb["wire"]["comp"]
    ops.append(Op("custom_ed_derive_wire_dev", ["ellgpu_custom_ed_derive_wire_dev"], EDWARDS, SIZES_SMALL,
                  {"k": w["k"], "enc": w["enc"]}, [(32,), (), ()], [w["x"], w["st"], w["err"]], {"undecodable": first(w["st"], 3)},
                  lambda cx, I, Q: cx.ctx.custom_ed_derive_wire_dev(ed(cx), I["k"], I["enc"], Q[0], Q[1], Q[2]), eprep))
    ops.append(Op("custom_ed_decode_points_dev", ["ellgpu_custom_ed_decode_points_dev"], EDWARDS, SIZES_SMALL, {"enc": w["enc"]},
                  [(64,), ()], [None, w["err"]], {"undecodable": first(w["err"] != 0, True)},
                  lambda cx, I, Q: cx.ctx.custom_ed_decode_points_dev(ed(cx), I["enc"], Q[0], Q[1]), eprep))

    mt = lambda cx: cx.made[("mont", MONT)]  # noqa: E731
    ops.append(Op("custom_mont_validate_dev", ["ellgpu_custom_mont_validate_dev"], MONT, SIZES_SMALL, {"x": mb["x"]}, [()],
                  [mb["vst"]], {"non_residue": first(mb["vst"] != 0, True)},
                  lambda cx, I, Q: cx.ctx.custom_mont_validate_dev(mt(cx), I["x"], Q[0]), mprep))
    ops.append(Op("custom_mont_derive_dev", ["ellgpu_custom_mont_derive_dev"], MONT, SIZES_SMALL, {"k": mb["k"], "x": mb["x"]},
                  [(32,), ()], [mb["dx"], mb["dst"]], {"not_validated": first((mb["dst"] == 1) | (mb["dst"] == 3), True),
                                                       "infinity": first(mb["dst"], 2)},
                  lambda cx, I, Q: cx.ctx.custom_mont_derive_dev(mt(cx), I["k"], I["x"], Q[0], Q[1]), mprep))

    # k B3 on a handle of a plain user-defined id: the table is uploaded with the curve's constants
    pspec = FB.spec_of(PLAIN)
    assert not pspec.get("domain")
    pb = FB.random_batch(pspec, D, 42)

    def pprep(cx):
        cid = cx.get(("plain", PLAIN), lambda ctx: FB.curve_id(ctx, pspec))
        cx.get(("plainbase",), lambda ctx: ctx.define_base(cid, FB.xy_bytes(FB.bases_of(pspec)[3], 32), 8))
    ops.append(Op("mul_base[plain id]", ["ellgpu_mul_base"], PLAIN, SIZES_SMALL, {"k": pb["k"]}, [(64,), ()], [pb["xy"], pb["inf"]],
                  {"infinity": 0}, lambda cx, I, Q: cx.ctx.mul_base(cx.made[("plainbase",)], I["k"], out=(Q[0], Q[1])), pprep))
    return ops


_ops = []


def OPS():
    """the operation table (built once: the models take a while)"""
    if not _ops:
        for c in PRESETS:
            _ops.extend(preset_ops(c))
        _ops.extend(ed25519_ops())
        for name in SHORT_DOMAINS:
            _ops.extend(short_domain_ops(name))
        _ops.extend(other_custom_ops())
    return _ops


def op(name, curve):
    return next(o for o in OPS() if o.name == name and o.curve == curve)


def interleaved():
    """OPS in an order in which neighbours differ in the operation and, where possible, in the curve"""
    groups = {}
    for o in OPS():
        groups.setdefault(o.curve, []).append(o)
    lists, out = [list(v) for v in groups.values()], []
    while any(lists):
        for l in lists:
            if l:
                out.append(l.pop(0))
    for a, b in zip(out, out[1:]):
        assert (a.name, a.curve) != (b.name, b.curve)
    return out


# ---- binding-table coverage ---------------------------------------------------------------------

def device_memory_symbols():
    """every `_dev` symbol of the recorded binding tables, and every entry point of theirs whose
    prototype (include/*.h) takes a `mem` argument"""
    import glob
    names = set()
    for path in glob.glob(os.path.join(HERE, "golden", "binding_sigs*.json")):
        with open(path) as f:
            names |= set(json.load(f))
    src = ""
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        with open(path) as f:
            src += re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    mem = {n for n, args in re.findall(r"\b(ellgpu_\w+)\s*\(([^;{]*?)\)\s*;", src) if re.search(r"\bint\s+mem\b", args)}
    return {n for n in names if n.endswith("_dev")} | (mem & names)


# ---- expected values ----------------------------------------------------------------------------

class Expected:
    """for every (operation, m): the device operands, and the bytes of that call issued alone on the
    default stream with a synchronisation behind it -- computed once, shared by the schedules and
    never written again"""

    def __init__(self, P, cx, everything):
        """everything: all items against the model; otherwise 16 items and every faulty one"""
        self.P, self.cx, self.made, self.everything = P, cx, {}, everything

    def size(self, m):
        return m if self.P.cap is None else min(m, self.P.cap)

    def get(self, o, m):
        m = self.size(m)
        k = (o.name, o.curve, m)
        if k not in self.made:
            P = self.P
            I = {n: (None if a is None else P.put(a)) for n, a in o.operands(m).items()}
            Q = [P.zeros(sh) for sh in o.out_shapes(m)]
            o.prepare(self.cx)
            P.sync()
            o.call(self.cx, I, Q)
            P.sync()
            want = [P.get(q) for q in Q]
            for w in want:
                w.setflags(write=False)
            check_against_model(o, m, want, self.everything)
            self.made[k] = (I, want)
        return self.made[k]


def check_against_model(o, m, want, everything):
    """the expected bytes against the model: all items, or a sample of 16 and every faulty item"""
    model = o.model_for(m)
    idx = np.arange(m) if everything else np.unique(np.concatenate(
        [np.arange(min(16, m)), np.array([i for i in o.faulty.values() if i < m], np.int64),
         np.array([i + D * ((m - 1 - i) // D) for i in o.faulty.values() if i < m], np.int64)]))
    assert len(idx) >= min(16, m)
    compared = 0
    for r, (w, a) in enumerate(zip(want, model)):
        if a is None:
            continue
        bad = [int(i) for i in idx if w[i].tobytes() != a[i].tobytes()]
        assert not bad, "%s on %s, m = %d: result %d differs from the model at items %s (item %% %d: %s)" % (
            o.name, o.curve, m, r, bad[:8], D, [i % D for i in bad[:8]])
        compared += 1
    assert compared, (o.name, "no model")
    assert any(w.any() for w in want), "%s on %s, m = %d: the expected output is all zeros" % (o.name, o.curve, m)
    return len(idx)


# ---- the queue ------------------------------------------------------------------------------------

class Queue:
    """the calls of one repetition of a schedule: issued in order, no host synchronisation between
    them; then synchronised once, compared, and the outputs zeroed for the next repetition"""

    def __init__(self, P, exp, schedule):
        self.P, self.exp, self.schedule = P, exp, schedule
        self.calls = []                         # (op, m, stream index, cx, I, outputs, want)
        self.outs = {}

    def add(self, o, m, si, cx=None):
        m = self.exp.size(m)
        I, want = self.exp.get(o, m)
        Q = [self.P.zeros(sh) for sh in o.out_shapes(m)]
        self.calls.append((o, m, si, cx or self.exp.cx, I, Q, want))
        return self

    def prepare(self):
        for o, _, _, cx, _, _, _ in self.calls:
            o.prepare(cx)

    def run(self, streams, between=None, reps=None):
        """between: {position: function()} run on the host after the call at that position was issued"""
        P = self.P
        self.prepare()
        P.sync()
        for rep in range(reps or P.reps):
            P.sync()                            # the zeroing below is queued on the default stream
            for pos, (o, m, si, cx, I, Q, want) in enumerate(self.calls):
                with P.on(streams[si]):
                    o.call(cx, I, Q)
                if between and pos in between:
                    between[pos](rep)
            P.sync()
            self.compare(rep)
            for c in self.calls:
                for q in c[5]:
                    P.zero(q)

    def compare(self, rep):
        for pos, (o, m, si, cx, I, Q, want) in enumerate(self.calls):
            for r, (q, w) in enumerate(zip(Q, want)):
                got = self.P.get(q)
                if got.tobytes() != w.tobytes():
                    rows = np.nonzero((got != w).reshape(m, -1).any(axis=1))[0]
                    raise AssertionError(
                        "schedule %s, repetition %d, position %d: %s on %s, stream %d, m = %d: result %d differs in %d items, "
                        "the first %s" % (self.schedule, rep, pos, o.name, o.curve, si, m, r, rows.size, rows[:8].tolist()))


def _size(o, turn):
    return o.sizes[turn % len(o.sizes)]


# ---- the schedules ----------------------------------------------------------------------------------

def schedule_round_robin(P, exp, nstreams, with_host_calls=False):
    """1 (and 6 with_host_calls): the operation table round-robin over the streams; neighbours are
    different operations claiming different slot sets of the same arena.  with_host_calls: a
    host-buffer verify and a defer / collect pair in the middle of the queue."""
    q = Queue(P, exp, "%d (%d streams)" % (6 if with_host_calls else 1, nstreams))
    for pos, o in enumerate(interleaved()):
        q.add(o, _size(o, pos + nstreams), pos % nstreams)
    between = None
    if with_host_calls:
        v = op("ecdsa_verify_dev", "secp256k1")
        a = v.operands(exp.size(777))
        want = v.model_for(exp.size(777))
        d = v.operands(5)
        ctx = exp.cx.ctx
        mid = len(q.calls) // 2

        def host_verify(rep):
            ok, st = ctx.ecdsa_verify("secp256k1", a["h"], a["r"], a["s"], a["pub"], status=True)      # waits for the lanes
            assert ok.tobytes() == want[0].tobytes() and st.tobytes() == want[1].tobytes(), ("schedule 6", rep, "host verify")

        def deferred(rep):
            ctx.defer()
            ok = ctx.ecdsa_verify("secp256k1", d["h"], d["r"], d["s"], d["pub"])
            ctx.collect()
            assert ok.tobytes() == v.model_for(5)[0].tobytes(), ("schedule 6", rep, "defer / collect")
        between = {mid: host_verify, mid + 3: deferred}
    q.run(P.streams(nstreams), between)
    return len(q.calls)


def schedule_grow(P, exp, comb_max_bytes=COMB_MAX_BYTES):
    """2: on a fresh context a large verify on stream A, then a small and a large mul_add2 on stream B:
    B's arena is freed and reallocated while A is in flight.  Then the mirror image."""
    v, a = op("ecdsa_verify_dev", "secp256k1"), op("mul_add2_dev", "secp256k1")
    n = 0
    for first, second in ((v, a), (a, v)):
        cx = Cx(P, comb_max_bytes)
        try:
            q = Queue(P, exp, "2 (%s first)" % first.name)
            q.add(first, 65536, 0, cx).add(second, 256, 1, cx).add(second, 65536, 1, cx)
            q.run(P.streams(2), reps=1)         # cold state: the arenas have their sizes after one pass
            n += len(q.calls)
        finally:
            P.sync()
            cx.close()
    return n


def schedule_first_use(P, exp):
    """3: on a fresh context, with a secp256k1 verify in flight on stream A, the context's first p256
    and first ed25519 call go to stream B: their tables are built on first use"""
    cx = Cx(P, COMB_MAX_BYTES_8)
    try:
        q = Queue(P, exp, "3")
        q.add(op("ecdsa_verify_dev", "secp256k1"), 65536, 0, cx)
        q.add(op("mul_fixed_dev", "p256"), 3000, 1, cx).add(op("eddsa_verify_dev", "ed25519"), 3000, 1, cx)
        q.run(P.streams(2), reps=1)
        if P.gpu:
            assert cx.ctx.comb_bits("p256") == 8 and cx.ctx.comb_bits("secp256k1") == 8
        return len(q.calls)
    finally:
        P.sync()
        cx.close()


def schedule_release(P, exp):
    """4: mul_base on a handle on stream A; from the host, at once, release_base and define_base of
    another point at the same width, whose allocation may take the same memory.  The call in flight
    gives the released point's products, a later call on the new handle the new point's.  (Two points
    of their own: no other schedule's handle is released here.)"""
    curve = "secp256k1"
    o = op("mul_base", curve)
    spec, m = FB.spec_of(curve), exp.size(65536)
    mdl, G = FB.model_of(spec), FB.bases_of(spec)[0]
    I, _ = exp.get(o, m)
    ks = FB.random_batch(spec, D, 31)["ints"][0]
    ctx = exp.cx.ctx
    pts, want = [mdl.mul(d, G) for d in (0x5eed0001, 0x5eed0002)], []
    for Pt in pts:                              # each point's call alone on the default stream, held to the model
        h = ctx.define_base(curve, FB.xy_bytes(Pt, 32), 8)
        Q = [P.zeros(sh) for sh in o.out_shapes(m)]
        P.sync()
        ctx.mul_base(h, I["k"], out=(Q[0], Q[1]))
        P.sync()
        ctx.release_base(h)
        want.append([P.get(q) for q in Q])
        a = [FB.answer(R, 32) for R in mdl.mul_many(ks, Pt, 256)]
        idx = np.arange(m) % D
        assert want[-1][0].tobytes() == np.stack([x for x, _ in a])[idx].tobytes()
        assert want[-1][1].tobytes() == np.array([f for _, f in a], np.uint8)[idx].tobytes() and want[-1][0].any()
    assert want[0][0].tobytes() != want[1][0].tobytes()
    streams = P.streams(2)
    for rep in range(P.reps):
        h = ctx.define_base(curve, FB.xy_bytes(pts[0], 32), 8)
        Q = [P.zeros(sh) for sh in o.out_shapes(m)]
        Q2 = [P.zeros(sh) for sh in o.out_shapes(m)]
        P.sync()
        with P.on(streams[0]):
            ctx.mul_base(h, I["k"], out=(Q[0], Q[1]))
        ctx.release_base(h)
        h2 = ctx.define_base(curve, FB.xy_bytes(pts[1], 32), 8)
        with P.on(streams[1]):
            ctx.mul_base(h2, I["k"], out=(Q2[0], Q2[1]))
        P.sync()
        ctx.release_base(h2)
        what = "schedule 4, repetition %d: mul_base on %s, m = %d" % (rep, curve, m)
        for pos, (got, w) in enumerate(((Q, want[0]), (Q2, want[1]))):
            assert P.get(got[0]).tobytes() == w[0].tobytes() and P.get(got[1]).tobytes() == w[1].tobytes(), \
                what + ", position %d, stream %d: %s" % (pos, pos, ("the released handle's products", "the new handle's products")[pos])
    return 2 * P.reps


def schedule_custom_turns(P, exp):
    """5: custom_verify_wire on two short domains taking turns over two streams, an Edwards verify and
    a Montgomery ladder between them: the parameter block in constant memory changes under every call"""
    w = [op("custom_verify_wire_dev", n) for n in SHORT_DOMAINS]
    e, l = op("custom_ed_verify_dev", EDWARDS), op("custom_mont_ladder_dev", MONT)
    q = Queue(P, exp, "5")
    for pos, o in enumerate([w[0], w[1], e, w[0], l, w[1], w[0], e, w[1], l, w[0], w[1]]):
        q.add(o, _size(o, pos), pos % 2)
    q.run(P.streams(2))
    return len(q.calls)


def schedule_callers_work(P, exp, default_stream):
    """7: the operands are written by a copy queued on the call's stream immediately before it, the
    result is read by a clone queued immediately behind it; no synchronisation until the end.
    default_stream: torch's default stream, the `_pending_default` path of Context._stream."""
    cx = exp.cx
    ops_ = [op("ecdsa_verify_dev", "secp256k1"), op("mul_base", "secp256k1"), op("custom_verify_wire_dev", SHORT_DOMAINS[0])]
    stream = None if default_stream else P.streams(1)[0]
    n = 0
    for pos, o in enumerate(ops_):
        m = exp.size(o.sizes[1])
        src, want = exp.get(o, m)
        o.prepare(cx)
        for rep in range(P.reps):
            I = {k: (None if a is None else P.clone(a)) for k, a in src.items()}
            for a in I.values():
                if a is not None:
                    P.zero(a)
            Q = [P.zeros(sh) for sh in o.out_shapes(m)]
            P.sync()
            with P.on(stream):
                for k, a in src.items():
                    if a is not None:
                        P.copy_into(I[k], a)
                o.call(cx, I, Q)
                got = [P.clone(x) for x in Q]
            P.sync()
            for r, (g, w_) in enumerate(zip(got, want)):
                assert P.get(g).tobytes() == w_.tobytes(), (
                    "schedule 7 (%s stream), repetition %d, position %d: %s on %s, stream 0, m = %d: the clone of result %d "
                    "differs" % ("default" if default_stream else "side", rep, pos, o.name, o.curve, m, r))
            n += 1
    return n
