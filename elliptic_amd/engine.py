"""Host-side batch engine over the C ABI (include/ellgpu.h).

One `Context` = one MI355X + one HIP stream (one process per GPU).  Two calling
styles, matching the two halves of the C ABI:

  * host buffers (numpy uint8 arrays / bytes): `mul_fixed`, `mul_var`,
    `mul_add2`, `ecdsa_verify`, `x25519` -- synchronous, what the N-API addon
    does for the patched JS library;
  * device buffers (torch.uint8 CUDA tensors): the `*_dev` methods -- inputs and
    outputs stay resident in HBM, work is enqueued on torch's current stream
    (bench.py, multi-GPU sharding).

Both styles of one operation go through one private method that writes the C
argument list once (`_call` takes the addresses and picks ellgpu_X or
ellgpu_X_dev); operations that differ only in the symbol and the operand widths
share one host body.

All integers are fixed-width big-endian byte strings (see include/ellgpu.h).
"""
import ctypes

import numpy as np

from . import _lib

CURVES = ["secp256k1", "p192", "p224", "p256", "p384", "p521", "ed25519", "curve25519"]
CURVE_ID = {n: i for i, n in enumerate(CURVES)}
FIELD_BYTES = {"secp256k1": 32, "p192": 24, "p224": 28, "p256": 32, "p384": 48, "p521": 66,
               "ed25519": 32, "curve25519": 32}
ORDER_BYTES = dict(FIELD_BYTES)
# per-item status in the `inf` / `ok` results (include/ellgpu.h ELLGPU_STATUS_OFF_CURVE): a point
# operand is not on the curve -- outside the engine's domain, reported instead of guessed (the
# reference computes with such points, and its answer depends on the order of its own operations)
STATUS_OFF_CURVE = 2
# Context.custom_sign_det's drbg_hash (include/ellgpu.h ELLGPU_HASH_*) and its cap on candidates per item
HASH_SHA256, HASH_SHA384, HASH_SHA512 = 0, 1, 2
CUSTOM_SIGN_MAX_DRAWS = 64
# user-defined short curves (Context.define_short) are addressed by the integer id the library
# hands out; their scalars and coordinates are 32 bytes wide whatever the prime's size
CURVE_CUSTOM0 = 16
for _i in range(CURVE_CUSTOM0, CURVE_CUSTOM0 + 16):
    FIELD_BYTES[_i] = ORDER_BYTES[_i] = 32
_PLAIN = frozenset((int, bytes, type(None)))      # what Context._call passes on as it is: no buffer, or an absent one


def _u8(a, shape=None):
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _rows2d(a, what):
    """an (n, len) array of digests or encodings; what: its name and shape for the refusal"""
    a = _u8(a)
    if a.ndim != 2:
        raise ValueError(what[0] + " must be " + what[1])
    return a


_HASHES, _ENC = ("hashes", "(n, hash_len)"), ("enc", "(n, enc_len)")


def ints_to_be(values, width):
    """list of ints -> (n, width) uint8 big-endian array"""
    out = np.zeros((len(values), width), dtype=np.uint8)
    for i, v in enumerate(values):
        out[i] = np.frombuffer(int(v).to_bytes(width, "big"), dtype=np.uint8)
    return out


def be_to_ints(arr):
    arr = np.asarray(arr, dtype=np.uint8)
    return [int.from_bytes(row.tobytes(), "big") for row in arr]


class Context:
    def __init__(self, device=0, lib_path=None, devices=None):
        """device: one HIP ordinal; devices=[...]: a GROUP over several (ellgpu_group_create) --
        mul_fixed / mul_var / mul_add2 / ecdsa_verify on host buffers are then sharded over the
        devices, one host thread each, results copied straight into the caller's arrays"""
        self._lib = _lib.load(lib_path) if not hasattr(lib_path, "ellgpu_version") else lib_path
        self._ctx = ctypes.c_void_p()
        self._own = None
        self._pending_default = None
        if devices is not None:
            devs = [int(d) for d in devices]
            arr = (ctypes.c_int * len(devs))(*devs)
            rc = self._lib.ellgpu_group_create(arr, len(devs), ctypes.byref(self._ctx))
            device = devs[0] if devs else 0
        else:
            rc = self._lib.ellgpu_ctx_create(int(device), ctypes.byref(self._ctx))
        if rc != 0:
            raise _lib.EllgpuError(rc, self._lib.ellgpu_last_error().decode())
        self.device = device
        self.devices = list(devices) if devices is not None else [device]
        self._own = None                  # torch view of the context's own stream (see _stream)
        self._pending_default = None
        self._pbytes = {}                 # p.byteLength() of the user-defined short curves (custom_encode_points)
        self._ed_pbytes = {}              # ... and of the user-defined Edwards curves (custom_ed_encode_points)
        self._base_curve = {}             # curve of each define_base handle (the width of its scalars)

    def group_size(self):
        return self._lib.ellgpu_group_size(self._ctx)

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self._lib.ellgpu_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if self._pending_default is not None:              # see _stream()
            cur, self._pending_default = self._pending_default, None
            cur.wait_stream(self._own)
        if rc != 0:
            raise _lib.EllgpuError(rc, self._lib.ellgpu_last_error().decode())

    @staticmethod
    def _cid(curve):
        return CURVE_ID[curve] if isinstance(curve, str) else int(curve)

    def synchronize(self):
        self._check(self._lib.ellgpu_ctx_synchronize(self._ctx))

    # ---- the one place where a batch call is made ----------------------------------------------

    def _stream(self):
        """the current torch stream OF THIS CONTEXT'S DEVICE (not of torch's current device)"""
        import torch
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream:
            return ctypes.c_void_p(cur.cuda_stream)
        # torch's default stream is the NULL handle, which the C ABI reads as "the context's own
        # (non-blocking) stream": run there, ordered after the default stream's work so far, and
        # let the default stream wait for the call's work afterwards (_check)
        if self._own is None:
            self._own = torch.cuda.ExternalStream(self._lib.ellgpu_ctx_stream(self._ctx), device=self.device)
        self._own.wait_stream(cur)
        self._pending_default = cur
        return ctypes.c_void_p(self._own.cuda_stream)

    def _call(self, name, dev, *args):
        """ellgpu_<name>(ctx, *args) on host arrays, or with dev ellgpu_<name>_dev(ctx, *args, stream)
        on device tensors.  args are in the C prototype's order: integers (and the byte string of
        custom_ed_validate's order) pass as they are, an absent optional operand as None, every
        other one as its address.  The _dev form trusts the caller's buffers: nothing but the
        address is read of them here."""
        if dev:
            ptrs = [a if type(a) in _PLAIN else a.data_ptr() for a in args]
            rc = getattr(self._lib, "ellgpu_" + name + "_dev")(self._ctx, *ptrs, self._stream())
        else:
            ptrs = [a if type(a) in _PLAIN else a.ctypes.data for a in args]
            rc = getattr(self._lib, "ellgpu_" + name)(self._ctx, *ptrs)
        self._check(rc)

    # the argument lists, one per shape of prototype: written once for the host method and its _dev twin

    def _c_rows(self, name, dev, curve, *ops):
        """(curve, n, operands...): n is the row count of the first operand"""
        self._call(name, dev, self._cid(curve), ops[0].shape[0], *ops)

    def _c_records(self, name, dev, curve, rec, *ops):
        """(curve, n, rec, rec_len, operands...) for (n, rec_len) digests or encodings"""
        n, rec_len = rec.shape
        self._call(name, dev, self._cid(curve), n, rec, rec_len, *ops)

    def _c_verify(self, name, dev, curve, hashes, msg_bits, r, s, pub, ok, st):
        n, hash_len = hashes.shape                 # (written out: the one call bench.py times per batch)
        self._call(name, dev, self._cid(curve), n, hashes, hash_len, int(msg_bits), r, s, pub, ok, st)

    def _c_sign(self, name, dev, curve, hashes, msg_bits, priv, nonces, canonical, r, s, rec, ok):
        self._c_records(name, dev, curve, hashes, int(msg_bits), priv, nonces, 1 if canonical else 0, r, s, rec, ok)

    def _c_sign_det(self, name, dev, curve, hashes, msg_bits, priv, drbg_hash, canonical, r, s, rec, ok):
        """drbg_hash=None: ellgpu_ecdsa_sign_det, whose prototype has none (the presets sign over SHA-256)"""
        drbg = () if drbg_hash is None else (int(drbg_hash),)
        self._c_records(name, dev, curve, hashes, int(msg_bits), priv, *drbg, 1 if canonical else 0, r, s, rec, ok)

    def _c_verify_wire(self, name, dev, curve, hashes, msg_bits, der, der_len, pubs, ok, err):
        self._c_records(name, dev, curve, hashes, int(msg_bits), der, der.shape[1], der_len, pubs, pubs.shape[1], ok, err)

    def _c_derive_wire(self, name, dev, curve, priv, pubs, x, st, err):
        n, pub_len = pubs.shape
        self._call(name, dev, self._cid(curve), n, priv, pubs, pub_len, x, st, err)

    def _c_encode(self, name, dev, curve, xy, compact, enc):
        self._c_rows(name, dev, curve, xy, 1 if compact else 0, enc)

    def _c_validate(self, name, dev, curve, xy, inf, check_order, st):
        self._c_rows(name, dev, curve, xy, inf, 1 if check_order else 0, st)

    def _c_decompress(self, name, dev, curve, v, odd, from_y, xy, st):
        """from_y=None: the short curves' prototypes, which have no such flag"""
        flag = () if from_y is None else (1 if from_y else 0,)
        self._c_rows(name, dev, curve, v, odd, *flag, xy, st)

    def _c_ed_validate(self, dev, curve, xy, order, st):
        self._c_rows("custom_ed_validate", dev, curve, xy, None if order is None else int(order).to_bytes(32, "big"), st)

    def _c_eddsa_verify(self, dev, msgs, msg_off, msg_len, sigs, pubs, ok, err):
        self._call("eddsa_verify", dev, sigs.shape[0], msgs, msg_off, int(msg_len), sigs, pubs, ok, err)

    def _c_eddsa_sign(self, dev, secrets, msgs, msg_off, msg_len, sig, pub):
        self._call("eddsa_sign", dev, secrets.shape[0], secrets, msgs, msg_off, int(msg_len), sig, pub)

    @staticmethod
    def _outs(out, shapes):
        """result arrays: fresh zeroed ones, or the caller's (checked) to write into"""
        if out is None:
            return [np.zeros(sh, np.uint8) for sh in shapes]
        for o, sh in zip(out, shapes):
            assert o.dtype == np.uint8 and o.shape == sh and o.flags.c_contiguous
        return list(out)

    # ---- curve definitions ------------------------------------------------------------------------

    def _define(self, name, p, coeffs, domain=()):
        """ellgpu_curve_define_<name>: p, the coefficients reduced mod p and a domain's (n, gx, gy)
        as 32-byte integers -> (curve id, p.byteLength())"""
        p = int(p)
        vals = [p] + [int(c) % p if p else int(c) for c in coeffs] + [int(v) for v in domain]
        cid = ctypes.c_int(-1)
        fn = getattr(self._lib, "ellgpu_curve_define_" + name)
        self._check(fn(self._ctx, *[v.to_bytes(32, "big") for v in vals], ctypes.byref(cid)))
        return cid.value, (p.bit_length() + 7) // 8

    def define_short(self, p, a, b):
        """Register y^2 = x^3 + a x + b over the odd prime p < 2^256 (`new curve.short({p, a, b})`
        with parameters that are no preset, lib/elliptic/curve/short.js:11-24) and return its
        curve id: valid for mul_var / mul_add2 (both points given) / point_add and their _dev forms."""
        cid, self._pbytes[cid] = self._define("short", p, (a, b))
        return cid

    def define_short_domain(self, p, a, b, n, gx, gy):
        """Register an ECDSA domain: the curve of define_short plus its order n and generator
        G = (gx, gy) (`new elliptic.ec({curve: {type: 'short', p, a, b, n, g}})`), and return its
        curve id.  Beside what a define_short id allows, mul_fixed, mul_add2 with p1=None and
        ecdsa_verify (and their _dev forms) take it.  Raises EllgpuError (ELLGPU_E_ARG) for n even
        or < 3, G off the curve or a singular curve; n and p are not tested for primality."""
        cid, self._pbytes[cid] = self._define("short_domain", p, (a, b), (n, gx, gy))
        return cid

    def define_edwards(self, p, a, d):
        """Register a x^2 + y^2 = 1 + d x^2 y^2 over the odd prime p < 2^256 (`new curve.edwards({p, a,
        c: 1, d})` with parameters that are not ed25519's) and return its curve id (as define_short)."""
        cid, self._ed_pbytes[cid] = self._define("edwards", p, (a, d))
        return cid

    def define_edwards_domain(self, p, a, d, n, gx, gy):
        """Register an ECDSA domain on an Edwards curve: the curve of define_edwards plus its order n
        and generator G = (gx, gy) (`new elliptic.ec(new curves.PresetCurve({type: 'edwards', p, a,
        c: '1', d, n, g}))`), and return its curve id.  Beside everything a define_edwards id allows,
        custom_ed_verify, custom_ed_sign and custom_ed_sign_det (and their _dev forms) take it.
        Raises EllgpuError (ELLGPU_E_ARG) for n even or < 3, G off the curve, a coordinate of G >= p
        or G = (0, 1); n and p are not tested for primality, n * G = O is not tested."""
        cid, self._ed_pbytes[cid] = self._define("edwards_domain", p, (a, d), (n, gx, gy))
        return cid

    def define_mont(self, p, a):
        """Register the Montgomery curve b y^2 = x^3 + a x^2 + x over the odd prime p < 2^256 (`new
        curve.mont({p, a, b})` with parameters that are not curve25519's) and return its curve id.
        There is no b: no formula of the reference's x-only model reads it.  Such an id is valid for
        custom_mont_ladder / custom_mont_validate / custom_mont_derive and their _dev forms only."""
        return self._define("mont", p, (a,))[0]

    def reserve(self, curve, n):
        self._check(self._lib.ellgpu_ctx_reserve(self._ctx, self._cid(curve), int(n)))

    def comb_bits(self, curve):
        """window width of the curve's fixed-base table on this context (0 = not built yet; the
        256-bit curves default to 22, narrower when the device could not hold that table)"""
        rc = self._lib.ellgpu_ctx_comb_bits(self._ctx, self._cid(curve))
        if rc < 0:
            raise _lib.EllgpuError(rc, self._lib.ellgpu_last_error().decode())
        return rc

    def defer(self):
        """the next few-item host-buffer call on this context returns once its work is enqueued;
        its result arrays are filled by collect() (ellgpu_ctx_defer / ellgpu_ctx_collect: the
        split form behind install()'s table re-validation).  Keep the result arrays alive."""
        self._check(self._lib.ellgpu_ctx_defer(self._ctx))

    def collect(self):
        self._check(self._lib.ellgpu_ctx_collect(self._ctx))

    # ---- fixed-base tables of caller-chosen points (ellgpu_base_*) -----------

    def define_base(self, curve, xy=None, window_bits=0):
        """Build the fixed-base table of a point that is used repeatedly (BasePoint#precompute on the
        device) and return its handle for mul_base / mul_base2.  xy: x || y in the curve's coordinate
        width (bytes or a uint8 array), or None for the curve's own generator -- the handle then
        aliases the curve's own table.  window_bits: 0, 4, 8, 12, 16, 22 on secp256k1 and p256
        (0 = 16), 0 or 8 elsewhere."""
        cid = self._cid(curve)
        h = ctypes.c_int(-1)
        buf = None if xy is None else _u8(xy).reshape(-1)
        self._check(self._lib.ellgpu_base_define(self._ctx, cid, None if buf is None else buf.ctypes.data,
                                                 int(window_bits), ctypes.byref(h)))
        self._base_curve[h.value] = curve
        return h.value

    def define_ed_base(self, curve, xy=None, window_bits=0):
        """define_base for ed25519 and user-defined Edwards ids (ellgpu_ed_base_define): the handle goes
        to mul_base, mul_base2, base_info and release_base like any other; rows are 32 bytes.  xy:
        x || y, 64 bytes, or None for the curve's own generator (ed25519: an alias of the curve's
        table; an Edwards domain: a table of its G).  window_bits: 0 or 16 on ed25519; 0 (= 8), 8 or
        16 on a user-defined id."""
        cid = self._cid(curve)
        h = ctypes.c_int(-1)
        buf = None if xy is None else _u8(xy).reshape(-1)
        self._check(self._lib.ellgpu_ed_base_define(self._ctx, cid, None if buf is None else buf.ctypes.data,
                                                    int(window_bits), ctypes.byref(h)))
        self._base_curve[h.value] = curve
        return h.value

    def release_base(self, base):
        self._check(self._lib.ellgpu_base_release(self._ctx, int(base)))
        self._base_curve.pop(int(base), None)

    def base_info(self, base):
        """-> (curve id, window width in use, bytes of the table); 0 bits and 0 bytes for a generator
        alias whose curve has not built its table yet"""
        c, w, b = ctypes.c_int(-1), ctypes.c_int(0), ctypes.c_uint64(0)
        self._check(self._lib.ellgpu_base_info(self._ctx, int(base), ctypes.byref(c), ctypes.byref(w), ctypes.byref(b)))
        return c.value, w.value, b.value

    def _base_width(self, base):
        curve = self._base_curve.get(int(base))
        if curve is None:
            curve = self.base_info(base)[0]
        return FIELD_BYTES[CURVES[curve] if isinstance(curve, int) and curve < len(CURVES) else curve]

    @staticmethod
    def _is_tensor(a):
        return hasattr(a, "data_ptr")

    def _dev_operands(self, ins, in_names, out, out_names, shapes):
        """checks the device tensors of a call on a base handle before their addresses go to the
        library; shapes: of the inputs, then of the results"""
        if out is None or len(out) != len(out_names):
            raise ValueError("device tensors need out=(%s): uint8 tensors of shapes %s"
                             % (", ".join(out_names), ", ".join(str(sh) for sh in shapes[len(ins):])))
        import torch
        for t, shape, name in zip(list(ins) + list(out), shapes, list(in_names) + ["out " + o for o in out_names]):
            if not self._is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("%s: a contiguous uint8 tensor of shape %s is needed" % (name, shape))
            if t.device != torch.device(self.device):
                raise ValueError("%s is on %s, the context on %s" % (name, t.device, torch.device(self.device)))

    def _base_call(self, name, bases, ins, in_names, widths, ints, out, out_names, out_widths):
        """ellgpu_mul_base / _base2 / ecdsa_verify_base: one symbol for both kinds of memory, told
        apart by a flag before the stream -- so the call is made here, beside _call.  The C argument
        list is (ctx, bases..., n, ins[0], ints..., ins[1:]..., results..., mem, stream).  widths /
        out_widths: bytes per row of every input / result (None: the first input's own second
        dimension; 0: a vector of n bytes); a None among ints stands for that dimension too."""
        dev = self._is_tensor(ins[0])
        if dev:
            if ins[0].dim() != 2:
                raise ValueError("%s: a contiguous uint8 tensor of shape (n, width) is needed" % in_names[0])
            n, w0 = int(ins[0].shape[0]), int(ins[0].shape[1])
        else:
            first = _u8(ins[0]) if widths[0] is None else _u8(ins[0], (-1, widths[0]))
            if first.ndim != 2:
                raise ValueError("%s must be (n, width)" % in_names[0])
            n, w0 = first.shape
        shapes = [(n, w0 if w is None else w) if w != 0 else (n,) for w in list(widths) + list(out_widths)]
        if dev:
            self._dev_operands(ins, in_names, out, out_names, shapes)
            res = list(out)
        else:
            ins = [first] + [_u8(a, sh) for a, sh in zip(ins[1:], shapes[1:])]
            res = self._outs(out, shapes[len(ins):])
        addr = [a.data_ptr() if dev else a.ctypes.data for a in list(ins) + res]
        fn = getattr(self._lib, "ellgpu_" + name)
        ints = [int(w0) if v is None else v for v in ints]
        self._check(fn(self._ctx, *[int(b) for b in bases], n, addr[0], *ints, *addr[1:], 1 if dev else 0,
                       self._stream() if dev else None))
        return res

    def _mul_bases(self, name, bases, ks, out):
        B = self._base_width(bases[0])
        xy, inf = self._base_call(name, bases, ks, ["k"] * len(ks), [B] * len(ks), (), out, ("xy", "inf"), (2 * B, 0))
        return xy, inf

    def mul_base(self, base, k, out=None):
        """k * B for the base of a define_base handle -> (xy, inf).  k: (n, field_bytes), used as it
        stands.  numpy arrays go through host memory; torch device tensors (k and out=(xy, inf), both
        required then) run on the current stream and return at once."""
        return self._mul_bases("mul_base", [base], [k], out)

    def mul_base2(self, base1, base2, k1, k2, out=None):
        """k1 * B1 + k2 * B2 over the tables of two bases of one curve -> (xy, inf); operands as in mul_base"""
        return self._mul_bases("mul_base2", [base1, base2], [k1, k2], out)

    def ecdsa_verify_base(self, base, hashes, r, s, msg_bits=0, out=None):
        """EC#verify of n signatures against the key of a define_base handle (ellgpu_ecdsa_verify_base:
        both scalar multiplications walk fixed-base tables) -> ok, (n,) strictly 0 / 1: what
        ecdsa_verify gives with the handle's point repeated as the key.  hashes: (n, hash_len); r, s:
        (n, order_bytes).  The handle: define_base on a preset or on a define_short_domain id, the
        generator alias included.  numpy arrays go through host memory; torch device tensors
        (hashes, r, s and out=(ok,), required then) run on the current stream and return at once."""
        NB = self._base_width(base)               # (order_bytes == field_bytes on every short curve)
        return self._base_call("ecdsa_verify_base", [base], [hashes, r, s], ["hashes", "r", "s"], [None, NB, NB],
                               (None, int(msg_bits)), out, ("ok",), (0,))[0]

    # ---- point arithmetic: presets, and user-defined ids where the definition allows ---------------

    def mul_fixed(self, curve, k, out=None):
        """out: optional (xy, inf) uint8 arrays to write into (see mul_var)"""
        B = FIELD_BYTES[curve]
        k = _u8(k, (-1, B))
        n = k.shape[0]
        xy, inf = self._outs(out, [(n, 2 * B), (n,)])
        self._c_rows("mul_fixed", False, curve, k, xy, inf)
        return xy, inf

    def mul_fixed_dev(self, curve, k, out_xy, out_inf):
        self._c_rows("mul_fixed", True, curve, k, out_xy, out_inf)

    def mul_var(self, curve, k, xy, out=None):
        """out: optional (xy, inf) uint8 arrays to write into (reusing result buffers spares a
        large batch the page faults of freshly allocated memory)."""
        B = FIELD_BYTES[curve]
        k = _u8(k, (-1, B))
        xy = _u8(xy, (-1, 2 * B))
        n = k.shape[0]
        assert xy.shape[0] == n
        out, inf = self._outs(out, [(n, 2 * B), (n,)])
        self._c_rows("mul_var", False, curve, k, xy, out, inf)
        return out, inf

    def mul_var_dev(self, curve, k, xy, out_xy, out_inf):
        self._c_rows("mul_var", True, curve, k, xy, out_xy, out_inf)

    def mul_add2(self, curve, k1, p1, k2, p2):
        """k1*P1 + k2*P2; p1=None means P1 = G."""
        B = FIELD_BYTES[curve]
        k1 = _u8(k1, (-1, B))
        n = k1.shape[0]
        k2 = _u8(k2, (n, B))
        p2 = _u8(p2, (n, 2 * B))
        p1 = None if p1 is None else _u8(p1, (n, 2 * B))
        out, inf = self._outs(None, [(n, 2 * B), (n,)])
        self._c_rows("mul_add2", False, curve, k1, p1, k2, p2, out, inf)
        return out, inf

    def mul_add2_dev(self, curve, k1, p1, k2, p2, out_xy, out_inf):
        self._c_rows("mul_add2", True, curve, k1, p1, k2, p2, out_xy, out_inf)

    def mul_sum(self, curve, k, xy, out=None):
        """n sums of m terms, sum_i k[j, i] * P[j, i] -> (xy (n, 2 field_bytes), inf (n,)): inf 0 a
        point, 1 the sum is the point at infinity, 2 (STATUS_OFF_CURVE) a term's point is not on the
        curve; xy is zeroed wherever inf is not 0 (ellgpu_mul_sum: _wnafMulAdd on any number of
        points, the partial sums added on the device, one normalisation per sum).  curve: a short
        preset or a define_short / define_short_domain id.  k: (n, m, field_bytes), used as it
        stands (not reduced mod n); xy: (n, m, 2 field_bytes).  numpy arrays go through host memory;
        torch device tensors (k, xy and out=(xy, inf), required then) run on the current stream and
        return at once."""
        B = FIELD_BYTES[CURVES[curve] if isinstance(curve, int) and 0 <= curve < len(CURVES) else curve]
        return self._sum_call("ellgpu_mul_sum", B, curve, k, xy, out)

    def ed_mul_sum(self, curve, k, xy, out=None):
        """mul_sum on the Edwards curves (ellgpu_ed_mul_sum): curve is "ed25519" or a define_edwards /
        define_edwards_domain id, k (n, m, 32), xy (n, m, 64) -> (xy (n, 64), inf (n,)).  The partial
        sums are added on the device through the curve's unified law (torsion points and the identity
        (0, 1) are ordinary terms), one normalisation per sum.  inf: 0 a point; the identity is (0, 1)
        with inf 1 on ed25519 and inf 0 on a user-defined id, as mul_add2 writes it there; 2
        (STATUS_OFF_CURVE) a term's point is not on the curve, xy zeroed.  numpy arrays go through
        host memory; torch device tensors (k, xy and out=(xy, inf), required then) run on the current
        stream and return at once.  mul_sum keeps refusing these curves, this method the short ones."""
        return self._sum_call("ellgpu_ed_mul_sum", 32, curve, k, xy, out)

    def _sum_call(self, symbol, B, curve, k, xy, out):
        """ellgpu_mul_sum / ellgpu_ed_mul_sum: (ctx, curve, n, m, k, xy, out_xy, out_inf, mem, stream),
        one symbol for both kinds of memory"""
        dev = self._is_tensor(k)
        if not dev:
            k, xy = _u8(k), _u8(xy)
        if len(k.shape) != 3 or int(k.shape[2]) != B:
            raise ValueError("k must be (n, m, %d)" % B)
        n, m = int(k.shape[0]), int(k.shape[1])
        shapes = [(n, m, B), (n, m, 2 * B), (n, 2 * B), (n,)]
        if dev:
            self._dev_operands([k, xy], ["k", "xy"], out, ("xy", "inf"), shapes)
            res = list(out)
        else:
            if xy.shape != shapes[1]:
                raise ValueError("xy must be (n, m, %d)" % (2 * B))
            res = self._outs(out, shapes[2:])
        addr = [a.data_ptr() if dev else a.ctypes.data for a in [k, xy] + res]
        self._check(getattr(self._lib, symbol)(self._ctx, self._cid(curve), n, m, *addr, 1 if dev else 0,
                                               self._stream() if dev else None))
        return res[0], res[1]

    def point_add(self, curve, xy1, xy2, inf1=None, inf2=None):
        """Point#add per pair of affine points (infinity through the optional flags) -> (xy, inf)"""
        B = FIELD_BYTES[curve]
        xy1 = _u8(xy1, (-1, 2 * B))
        n = xy1.shape[0]
        xy2 = _u8(xy2, (n, 2 * B))
        inf1 = None if inf1 is None else _u8(inf1, (n,))
        inf2 = None if inf2 is None else _u8(inf2, (n,))
        out, inf = self._outs(None, [(n, 2 * B), (n,)])
        self._c_rows("point_add", False, curve, xy1, inf1, xy2, inf2, out, inf)
        return out, inf

    def point_add_dev(self, curve, xy1, xy2, out_xy, out_inf, inf1=None, inf2=None):
        self._c_rows("point_add", True, curve, xy1, inf1, xy2, inf2, out_xy, out_inf)

    def ecdh_derive(self, curve, priv, pub_xy):
        """KeyPair#derive per item (ec/key.js:102-107): pub.validate() then pub.mul(priv).getX()
        -> (x, status); status 0 shared secret, 1 'public point not validated', 2 the product is
        the point at infinity (getX throws in the reference).  Two launches: the curve-equation
        kernel and the variable-base ladder."""
        B = FIELD_BYTES[curve]
        pub_xy = _u8(pub_xy, (-1, 2 * B))
        n = pub_xy.shape[0]
        priv = _u8(priv, (n, B))
        st = self.validate(curve, pub_xy, check_order=False)
        xy, inf = self.mul_var(curve, priv, pub_xy)
        status = np.where(st != 0, 1, np.where(inf != 0, 2, 0)).astype(np.uint8)
        x = np.ascontiguousarray(xy[:, :B])
        x[status != 0] = 0
        return x, status

    def x25519(self, k, x):
        k = _u8(k, (-1, 32))
        x = _u8(x, (-1, 32))
        n = k.shape[0]
        out, inf = self._outs(None, [(n, 32), (n,)])
        self._call("x25519_ladder", False, n, k, x, out, inf)
        return out, inf

    def x25519_dev(self, k, x, out_x, out_inf):
        self._call("x25519_ladder", True, k.shape[0], k, x, out_x, out_inf)

    def x25519_derive(self, k, x):
        """KeyPair#derive on curve25519 per item: validate (is x an abscissa of the curve?) and the
        ladder in one call -> (out_x (n, 32), status (n,)): 0 shared secret, 1 x has no point (the
        reference throws 'Assertion failed' out of its square root), 2 the product is infinity"""
        k = _u8(k, (-1, 32))
        n = k.shape[0]
        x = _u8(x, (n, 32))
        out, st = self._outs(None, [(n, 32), (n,)])
        self._call("x25519_derive", False, n, k, x, out, st)
        return out, st

    # ---- ECDSA: the presets (widths FIELD_BYTES / ORDER_BYTES) and the user-defined domains (32 / 32)
    # share their host bodies; curve is a preset's name, or an id from define_short_domain
    # (custom_*) / define_edwards_domain (custom_ed_*)

    def _verify(self, name, B, NB, curve, hashes, r, s, pub, msg_bits, status, out):
        hashes = _rows2d(hashes, _HASHES)
        n = hashes.shape[0]
        r = _u8(r, (n, NB))                     # explicit row counts: a short array must not
        s = _u8(s, (n, NB))                     # make the library read past a buffer
        pub = _u8(pub, (n, 2 * B))
        res = self._outs(out, [(n,), (n,)] if status else [(n,)])
        self._c_verify(name, False, curve, hashes, msg_bits, r, s, pub, res[0], res[1] if status else None)
        return (res[0], res[1]) if status else res[0]

    def ecdsa_verify(self, curve, hashes, r, s, pub, msg_bits=0, status=False):
        """EC#verify per item -> ok, a mask of strictly 0 / 1.  status=True -> (ok, st): st[i] = 2
        (ELLGPU_STATUS_OFF_CURVE) where r and s are in range but pub[i] is not on the curve -- ok[i]
        is 0 there, the safe answer; the reference computes with such keys, run it on those items
        if its answer is wanted -- else 0."""
        return self._verify("ecdsa_verify", FIELD_BYTES[curve], ORDER_BYTES[curve], curve, hashes, r, s, pub, msg_bits, status, None)

    def ecdsa_verify_dev(self, curve, hashes, r, s, pub, out_ok, msg_bits=0, out_status=None):
        """out_ok: uint8 CUDA tensor (n), strictly 0 / 1; out_status (optional, same shape): 2 where
        the key is not on the curve (out_ok 0 there), else 0 -- see ecdsa_verify"""
        self._c_verify("ecdsa_verify", True, curve, hashes, msg_bits, r, s, pub, out_ok, out_status)

    def custom_ed_verify(self, curve, hashes, r, s, pub, msg_bits=0, status=False, out=None):
        """EC#verify per item on an Edwards domain id -> ok, a mask of strictly 0 / 1; hashes
        (n, 1..64), r, s (n, 32), pub (n, 64) affine.  status=True -> (ok, st): st[i] = 2 where r and
        s are in range but pub[i] is not on the curve (ok[i] is 0 there), else 0.  out= the result
        arrays to write into: (ok,) or, with status, (ok, st)"""
        return self._verify("custom_ed_verify", 32, 32, curve, hashes, r, s, pub, msg_bits, status, out)

    def custom_ed_verify_dev(self, curve, hashes, r, s, pub, out_ok, out_status=None, msg_bits=0):
        self._c_verify("custom_ed_verify", True, curve, hashes, msg_bits, r, s, pub, out_ok, out_status)

    def _sign(self, name, NB, curve, hashes, priv, nonces, canonical, msg_bits, out):
        hashes = _rows2d(hashes, _HASHES)
        n = hashes.shape[0]
        priv = _u8(priv, (n, NB))
        nonces = _u8(nonces, (n, NB))
        r, s, rec, ok = self._outs(out, [(n, NB), (n, NB), (n,), (n,)])
        self._c_sign(name, False, curve, hashes, msg_bits, priv, nonces, canonical, r, s, rec, ok)
        return r, s, rec, ok

    def _sign_det(self, name, NB, curve, hashes, priv, drbg_hash, canonical, msg_bits, out):
        hashes = _rows2d(hashes, _HASHES)
        n = hashes.shape[0]
        priv = _u8(priv, (n, NB))
        r, s, rec, ok = self._outs(out, [(n, NB), (n, NB), (n,), (n,)])
        self._c_sign_det(name, False, curve, hashes, msg_bits, priv, drbg_hash, canonical, r, s, rec, ok)
        return r, s, rec, ok

    def ecdsa_sign(self, curve, hashes, priv, nonces, canonical=False, msg_bits=0):
        """one pass of EC#sign per item for supplied nonces -> (r, s, recid, ok)"""
        return self._sign("ecdsa_sign", ORDER_BYTES[curve], curve, hashes, priv, nonces, canonical, msg_bits, None)

    def ecdsa_sign_dev(self, curve, hashes, priv, nonces, out_r, out_s, out_recid, out_ok, canonical=False,
                       msg_bits=0):
        self._c_sign("ecdsa_sign", True, curve, hashes, msg_bits, priv, nonces, canonical, out_r, out_s, out_recid, out_ok)

    def ecdsa_sign_det(self, curve, hashes, priv, canonical=False, msg_bits=0):
        """EC#sign with the reference's own (HmacDRBG, deterministic) nonces -> (r, s, recid, ok)"""
        return self._sign_det("ecdsa_sign_det", ORDER_BYTES[curve], curve, hashes, priv, None, canonical, msg_bits, None)

    def ecdsa_sign_det_dev(self, curve, hashes, priv, out_r, out_s, out_recid, out_ok, canonical=False,
                           msg_bits=0):
        self._c_sign_det("ecdsa_sign_det", True, curve, hashes, msg_bits, priv, None, canonical, out_r, out_s,
                         out_recid, out_ok)

    def custom_sign(self, curve, hashes, priv, nonces, canonical=False, msg_bits=0, out=None):
        """one pass of EC#sign per item on a domain id for supplied nonces -> (r, s, recid, ok).
        hashes (n, 1..64); priv, nonces (n, 32) big-endian: priv is reduced mod n, a nonce v stands
        for k = v >> max(0, 8 byteLength(v) - n.bitLength()) as options.k's BN does; ok = 0 (r, s,
        recid zeroed) where the reference goes on to its next nonce"""
        return self._sign("custom_sign", 32, curve, hashes, priv, nonces, canonical, msg_bits, out)

    def custom_sign_dev(self, curve, hashes, priv, nonces, out_r, out_s, out_recid, out_ok, canonical=False,
                        msg_bits=0):
        self._c_sign("custom_sign", True, curve, hashes, msg_bits, priv, nonces, canonical, out_r, out_s, out_recid, out_ok)

    def custom_sign_det(self, curve, hashes, priv, drbg_hash=HASH_SHA256, canonical=False, msg_bits=0, out=None):
        """EC#sign per item on a domain id with the reference's own HmacDRBG nonces over drbg_hash
        (HASH_SHA256 / HASH_SHA384 / HASH_SHA512: the caller's options.hash) -> (r, s, recid, ok);
        at most CUSTOM_SIGN_MAX_DRAWS candidates per item.  Unsupported where n.byteLength() < 24
        (the reference throws 'Not enough entropy')"""
        return self._sign_det("custom_sign_det", 32, curve, hashes, priv, int(drbg_hash), canonical, msg_bits, out)

    def custom_sign_det_dev(self, curve, hashes, priv, out_r, out_s, out_recid, out_ok, drbg_hash=HASH_SHA256,
                            canonical=False, msg_bits=0):
        self._c_sign_det("custom_sign_det", True, curve, hashes, msg_bits, priv, int(drbg_hash), canonical, out_r, out_s,
                         out_recid, out_ok)

    def custom_ed_sign(self, curve, hashes, priv, nonces, canonical=False, msg_bits=0, out=None):
        """one pass of EC#sign per item on an Edwards domain id for supplied nonces -> (r, s, recid,
        ok); arguments and results as custom_sign"""
        return self._sign("custom_ed_sign", 32, curve, hashes, priv, nonces, canonical, msg_bits, out)

    def custom_ed_sign_dev(self, curve, hashes, priv, nonces, out_r, out_s, out_recid, out_ok, canonical=False,
                           msg_bits=0):
        self._c_sign("custom_ed_sign", True, curve, hashes, msg_bits, priv, nonces, canonical, out_r, out_s, out_recid,
                     out_ok)

    def custom_ed_sign_det(self, curve, hashes, priv, drbg_hash=HASH_SHA256, canonical=False, msg_bits=0, out=None):
        """EC#sign per item on an Edwards domain id with the reference's own HmacDRBG nonces over
        drbg_hash -> (r, s, recid, ok); arguments and results as custom_sign_det"""
        return self._sign_det("custom_ed_sign_det", 32, curve, hashes, priv, int(drbg_hash), canonical, msg_bits, out)

    def custom_ed_sign_det_dev(self, curve, hashes, priv, out_r, out_s, out_recid, out_ok, drbg_hash=HASH_SHA256,
                               canonical=False, msg_bits=0):
        self._c_sign_det("custom_ed_sign_det", True, curve, hashes, msg_bits, priv, int(drbg_hash), canonical, out_r,
                         out_s, out_recid, out_ok)

    def _recover(self, name, B, NB, curve, hashes, r, s, recid, out):
        hashes = _rows2d(hashes, _HASHES)
        n = hashes.shape[0]
        r = _u8(r, (n, NB))
        s = _u8(s, (n, NB))
        recid = _u8(recid, (n,))
        xy, st = self._outs(out, [(n, 2 * B), (n,)])
        self._c_records(name, False, curve, hashes, r, s, recid, xy, st)
        return xy, st

    def ecdsa_recover(self, curve, hashes, r, s, recid):
        """EC#recoverPubKey per item -> (xy (n, 2B), status (n,)): 0 point, 1 infinity,
        2 the reference throws, 3 outside the engine's domain (r = 0 or r >= n)"""
        return self._recover("ecdsa_recover", FIELD_BYTES[curve], ORDER_BYTES[curve], curve, hashes, r, s, recid, None)

    def ecdsa_recover_dev(self, curve, hashes, r, s, recid, out_xy, out_status):
        self._c_records("ecdsa_recover", True, curve, hashes, r, s, recid, out_xy, out_status)

    def ecdsa_recid(self, curve, hashes, r, s, pub_xy, out=None):
        """EC#getKeyRecoveryParam per item, in one pass (ellgpu_ecdsa_recid: one double-scalar product,
        no square root) -> (recid (n,), status (n,)): status 0 with the id 0 .. 3 the reference
        returns, 1 the reference throws (no id recovers the key), 2 the key is not on the curve, 3
        outside the engine's domain (r = 0, r >= n or s = 0 mod n: run the reference on those);
        recid is 0 wherever status is not.  curve: one of the six short presets.  hashes:
        (n, hash_len), NOT truncated to the order's bit length (as in ecdsa_recover); r, s:
        (n, order_bytes), s is reduced mod n; pub_xy: (n, 2 field_bytes).  numpy arrays go through
        host memory; torch device tensors (all four and out=(recid, status), required then) run on
        the current stream and return at once."""
        name = CURVES[curve] if isinstance(curve, int) and 0 <= curve < len(CURVES) else curve
        B, NB = FIELD_BYTES[name], ORDER_BYTES[name]
        # (_base_call's leading integers are handles there; here the one integer is the curve id)
        recid, st = self._base_call("ecdsa_recid", [self._cid(curve)], [hashes, r, s, pub_xy],
                                    ["hashes", "r", "s", "pub_xy"], [None, NB, NB, 2 * B], (None,), out,
                                    ("recid", "status"), (0, 0))
        return recid, st

    def custom_recover(self, curve, hashes, r, s, recid, out=None):
        """EC#recoverPubKey per item on a domain id -> (xy, status): 0 point, 1 infinity, 2 the
        reference throws, 3 r = 0 or r >= n (handed to the reference).  hashes (n, 1..64) are NOT
        truncated to the order's bit length (the reference does not either): e = BN(hash) mod n"""
        return self._recover("custom_recover", 32, 32, curve, hashes, r, s, recid, out)

    def custom_recover_dev(self, curve, hashes, r, s, recid, out_xy, out_status):
        self._c_records("custom_recover", True, curve, hashes, r, s, recid, out_xy, out_status)

    # ---- wire formats: DER signatures, SEC1 keys ----------------------------------------------------

    @staticmethod
    def _pack_records(items, stride=None):
        """list of byte strings -> ((n, stride) uint8 array, (n,) uint32 lengths)"""
        n = len(items)
        stride = max([stride or 1] + [len(x) for x in items])
        buf = np.zeros((n, stride), np.uint8)
        lens = np.zeros(n, np.uint32)
        for i, x in enumerate(items):
            buf[i, :len(x)] = np.frombuffer(bytes(x), np.uint8)
            lens[i] = len(x)
        return buf, lens

    def sig_from_der(self, curve, sigs):
        """Signature#_importDER per item (sigs: list of byte strings) -> (r, s, status);
        status 0 parsed, 1 malformed ('Signature without r or s'), 2 wider than n"""
        NB = ORDER_BYTES[curve]
        der, lens = self._pack_records(sigs)
        n = len(sigs)
        r, s, st = self._outs(None, [(n, NB), (n, NB), (n,)])
        self._call("sig_from_der", False, self._cid(curve), n, der, der.shape[1], lens, r, s, st)
        return r, s, st

    def sig_to_der(self, curve, r, s):
        """Signature#toDER per (r, s) -> list of byte strings"""
        NB = ORDER_BYTES[curve]
        r = _u8(r, (-1, NB))
        n = r.shape[0]
        s = _u8(s, (n, NB))
        stride = 2 * NB + 9
        out = np.zeros((n, stride), np.uint8)
        lens = np.zeros(n, np.uint32)
        self._call("sig_to_der", False, self._cid(curve), n, r, s, out, stride, lens)
        return [out[i, :lens[i]].tobytes() for i in range(n)]

    def _verify_wire(self, name, curve, hashes, sigs, pubs, msg_bits, out, want_err):
        hashes = _rows2d(hashes, _HASHES)
        n = hashes.shape[0]
        pubs = _u8(pubs)
        if isinstance(sigs, tuple):                   # already packed: ((n, stride) uint8, (n,) uint32)
            der, lens = _u8(sigs[0]), np.ascontiguousarray(sigs[1], np.uint32)
        else:
            der, lens = self._pack_records(sigs)
        if pubs.ndim != 2 or pubs.shape[0] != n or der.shape[0] != n or lens.shape[0] != n:
            raise ValueError("pubs must be (n, pub_len), sigs n byte strings (or packed records + lengths)")
        ok, err = self._outs(out, [(n,), (n,)])
        self._c_verify_wire(name, False, curve, hashes, msg_bits, der, lens, pubs, ok, err if want_err else None)
        return ok, (err if want_err else None)

    def ecdsa_verify_wire(self, curve, hashes, sigs, pubs, msg_bits=0):
        """EC#verify(msg, DER signature, encoded key) per item.  sigs: list of byte strings (or
        the packed pair _pack_records returns);
        pubs: (n, pub_len) SEC1 encodings -> (ok, err); err 1..3 = decodePoint's status for the
        key, 4 = 'Signature without r or s'"""
        return self._verify_wire("ecdsa_verify_wire", curve, hashes, sigs, pubs, msg_bits, None, True)

    def ecdsa_verify_wire_dev(self, curve, hashes, der, der_len, pubs, out_ok, out_err=None, msg_bits=0):
        self._c_verify_wire("ecdsa_verify_wire", True, curve, hashes, msg_bits, der, der_len, pubs, out_ok, out_err)

    def custom_verify_wire(self, curve, hashes, sigs, pubs, msg_bits=0, out=None, want_err=True):
        """EC#verify(msg, DER signature, encoded key) per item on a domain id; arguments and
        (ok, err) as ecdsa_verify_wire.  want_err=False passes no err array -> (ok, None)"""
        return self._verify_wire("custom_verify_wire", curve, hashes, sigs, pubs, msg_bits, out, want_err)

    def custom_verify_wire_dev(self, curve, hashes, der, der_len, pubs, out_ok, out_err=None, msg_bits=0):
        self._c_verify_wire("custom_verify_wire", True, curve, hashes, msg_bits, der, der_len, pubs, out_ok, out_err)

    # ---- points: decompress, decode, encode, validate -- presets (width FIELD_BYTES), user-defined
    # short curves (custom_*: an id from define_short / define_short_domain) and Edwards curves
    # (custom_ed_*: an id from define_edwards); a user-defined coordinate is 32 bytes, a SEC1
    # coordinate p.byteLength() bytes

    def _decompress(self, name, B, curve, v, odd, from_y, out):
        v = _u8(v, (-1, B))
        n = v.shape[0]
        odd = _u8(odd, (n,))
        xy, st = self._outs(out, [(n, 2 * B), (n,)])
        self._c_decompress(name, False, curve, v, odd, from_y, xy, st)
        return xy, st

    def decompress(self, curve, v, odd):
        """pointFromX (short curves, v = x) / pointFromY (ed25519, v = y) -> (xy, ok)"""
        return self._decompress("decompress", FIELD_BYTES[curve], curve, v, odd, None, None)

    def decompress_dev(self, curve, v, odd, out_xy, out_ok):
        self._c_decompress("decompress", True, curve, v, odd, None, out_xy, out_ok)

    def custom_decompress(self, curve, x, odd, out=None):
        """ShortCurve#pointFromX per item -> (xy, status); status 0 point, 2 'invalid point'
        (p = 3 mod 4), 3 'Assertion failed' (p = 1 mod 4: bn.js's Tonelli-Shanks loop)"""
        return self._decompress("custom_decompress", 32, curve, x, odd, None, out)

    def custom_decompress_dev(self, curve, x, odd, out_xy, out_status):
        self._c_decompress("custom_decompress", True, curve, x, odd, None, out_xy, out_status)

    def custom_ed_decompress(self, curve, v, odd, from_y=False, out=None):
        """EdwardsCurve#pointFromX (from_y=False) or #pointFromY per item on a define_edwards id ->
        (xy, status): 0 a point, 2 'invalid point', 3 'Assertion failed' (a non-residue where
        p = 1 mod 4).  odd (n,) is the reference's boolean.  A zero denominator gives a zero square
        (redInvm(0) = 0): pointFromX then returns (x, 0) with status 0; pointFromY with x^2 = 0
        returns (0, y) for an even request and 'invalid point' for an odd one"""
        return self._decompress("custom_ed_decompress", 32, curve, v, odd, bool(from_y), out)

    def custom_ed_decompress_dev(self, curve, v, odd, from_y, out_xy, out_status):
        self._c_decompress("custom_ed_decompress", True, curve, v, odd, bool(from_y), out_xy, out_status)

    def _decode_points(self, name, B, curve, enc, out):
        enc = _rows2d(enc, _ENC)
        n = enc.shape[0]
        xy, st = self._outs(out, [(n, 2 * B), (n,)])
        self._c_records(name, False, curve, enc, xy, st)
        return xy, st

    def decode_points(self, curve, enc):
        """decodePoint per row of `enc` (n, enc_len) -> (xy, status); status 0 point,
        1 'Unknown point format', 2 'invalid point', 3 'Assertion failed' (hybrid parity)"""
        return self._decode_points("decode_points", FIELD_BYTES[curve], curve, enc, None)

    def decode_points_dev(self, curve, enc, out_xy, out_status):
        self._c_records("decode_points", True, curve, enc, out_xy, out_status)

    def custom_decode_points(self, curve, enc, out=None):
        """BaseCurve#decodePoint per row of `enc` (n, enc_len) -> (xy, status) as decode_points;
        a compressed x without a y is 3 where p = 1 (mod 4)"""
        return self._decode_points("custom_decode_points", 32, curve, enc, out)

    def custom_decode_points_dev(self, curve, enc, out_xy, out_status):
        self._c_records("custom_decode_points", True, curve, enc, out_xy, out_status)

    def custom_ed_decode_points(self, curve, enc, out=None):
        """BaseCurve#decodePoint per row of `enc` (n, enc_len) on a define_edwards id -> (xy, status)
        as custom_decode_points; 04 / 06 / 07 points are not tested against the curve"""
        return self._decode_points("custom_ed_decode_points", 32, curve, enc, out)

    def custom_ed_decode_points_dev(self, curve, enc, out_xy, out_status):
        self._c_records("custom_ed_decode_points", True, curve, enc, out_xy, out_status)

    def encode_points(self, curve, xy, compact=False):
        """BasePoint#encode / EDDSA#encodePoint per affine point -> (n, enc_len) bytes"""
        B = FIELD_BYTES[curve]
        xy = _u8(xy, (-1, 2 * B))
        n = xy.shape[0]
        enc_len = 32 if curve == "ed25519" else (1 + B if compact else 1 + 2 * B)
        out = np.zeros((n, enc_len), np.uint8)
        self._c_encode("encode_points", False, curve, xy, compact, out)
        return out

    def encode_points_dev(self, curve, xy, compact, out_enc):
        self._c_encode("encode_points", True, curve, xy, compact, out_enc)

    def _custom_encode(self, name, pbytes, curve, xy, compact, out):
        xy = _u8(xy, (-1, 64))
        n = xy.shape[0]
        pl = pbytes.get(self._cid(curve))
        if pl is None:
            # not a curve of this kind defined on this context (a preset, an unknown id, the other
            # kind): the library's own refusal, asked for with no items so that no width has to be guessed
            self._call(name, False, self._cid(curve), 0, None, 0, None)
            raise ValueError("%s: curve %r was not defined on this context" % (name, curve))
        enc, = self._outs(out, [(n, 1 + pl if compact else 1 + 2 * pl)])
        self._c_encode(name, False, curve, xy, compact, enc)
        return enc

    def custom_encode_points(self, curve, xy, compact=False, out=None):
        """BasePoint#encode per item at the curve's own width -> (n, 1 + PL) for compact, else
        (n, 1 + 2 PL), PL = coord_bytes(curve); coordinates are reduced mod p first"""
        return self._custom_encode("custom_encode_points", self._pbytes, curve, xy, compact, out)

    def custom_encode_points_dev(self, curve, xy, compact, out_enc):
        """the _dev form: like every _dev call it trusts the caller's buffers -- out_enc must hold
        n rows of 1 + PL (compact) or 1 + 2 PL bytes, PL = p.byteLength() of the curve"""
        self._c_encode("custom_encode_points", True, curve, xy, compact, out_enc)

    def custom_ed_encode_points(self, curve, xy, compact=False, out=None):
        """BasePoint#encode per item at the curve's own width -> (n, 1 + PL) for compact, else
        (n, 1 + 2 PL), PL = p.byteLength() as recorded by define_edwards"""
        return self._custom_encode("custom_ed_encode_points", self._ed_pbytes, curve, xy, compact, out)

    def custom_ed_encode_points_dev(self, curve, xy, compact, out_enc):
        """out_enc must hold n rows of 1 + PL (compact) or 1 + 2 PL bytes"""
        self._c_encode("custom_ed_encode_points", True, curve, xy, compact, out_enc)

    def _validate(self, name, B, curve, xy, inf, check_order, out):
        xy = _u8(xy, (-1, 2 * B))
        n = xy.shape[0]
        inf = _u8(inf, (n,)) if inf is not None else None
        st, = self._outs(out, [(n,)])
        self._c_validate(name, False, curve, xy, inf, check_order, st)
        return st

    def validate(self, curve, xy, inf=None, check_order=True):
        """KeyPair#validate per item -> status (0 ok, 1 'Invalid public key', 2 'Public key is
        not a point', 3 'Public key * N != O')"""
        return self._validate("validate", FIELD_BYTES[curve], curve, xy, inf, check_order, None)

    def validate_dev(self, curve, xy, inf, check_order, out_status):
        self._c_validate("validate", True, curve, xy, inf, check_order, out_status)

    def custom_validate(self, curve, xy, inf=None, check_order=True, out=None):
        """KeyPair#validate per item -> status: 0 ok, 1 'Invalid public key' (inf[i] set), 2 'Public
        key is not a point', 3 'Public key * N != O' (check_order: needs a domain id)"""
        return self._validate("custom_validate", 32, curve, xy, inf, check_order, out)

    def custom_validate_dev(self, curve, xy, inf, check_order, out_status):
        self._c_validate("custom_validate", True, curve, xy, inf, check_order, out_status)

    def custom_ed_validate(self, curve, xy, order=None, out=None):
        """KeyPair#validate per item -> status: 0 ok, 1 'Invalid public key' (the point is (0, 1)),
        2 'Public key is not a point', 3 'Public key * N != O'.  order: the integer N (an Edwards
        definition carries none), or None to skip the order test"""
        xy = _u8(xy, (-1, 64))
        st, = self._outs(out, [(xy.shape[0],)])
        self._c_ed_validate(False, curve, xy, order, st)
        return st

    def custom_ed_validate_dev(self, curve, xy, order, out_status):
        """order is an integer or None here too: it travels as a parameter, not as a device buffer"""
        self._c_ed_validate(True, curve, xy, order, out_status)

    # ---- ECDH on user-defined curves: short (custom_*), Edwards (custom_ed_*), Montgomery (custom_mont_*,
    # an id from define_mont: x-only, the peer is 32 bytes) ------------------------------------------

    def _derive(self, name, pub_bytes, curve, priv, pub, out):
        priv = _u8(priv, (-1, 32))
        n = priv.shape[0]
        pub = _u8(pub, (n, pub_bytes))
        x, st = self._outs(out, [(n, 32), (n,)])
        self._c_rows(name, False, curve, priv, pub, x, st)
        return x, st

    def custom_derive(self, curve, priv, pub_xy, out=None):
        """KeyPair#derive per item on a domain id or a plain define_short id -> (x, status): 0 x is
        pub.mul(priv).getX(), 1 'public point not validated', 2 the product is the point at
        infinity.  priv (n, 32) is used as it stands (not reduced mod n); pub_xy (n, 64), each
        coordinate reduced mod p"""
        return self._derive("custom_derive", 64, curve, priv, pub_xy, out)

    def custom_derive_dev(self, curve, priv, pub_xy, out_x, out_status):
        self._c_rows("custom_derive", True, curve, priv, pub_xy, out_x, out_status)

    def custom_ed_derive(self, curve, priv, pub_xy, out=None):
        """KeyPair#derive per item on a define_edwards id -> (x, status): 0 x is
        pub.mul(priv).getX(), 1 'public point not validated', 2 the product has Z = 0 (incomplete
        addition laws only).  priv (n, 32) is used as it stands; priv = 0 or the peer (0, 1) gives
        status 0 with x = 0"""
        return self._derive("custom_ed_derive", 64, curve, priv, pub_xy, out)

    def custom_ed_derive_dev(self, curve, priv, pub_xy, out_x, out_status):
        self._c_rows("custom_ed_derive", True, curve, priv, pub_xy, out_x, out_status)

    def custom_mont_derive(self, curve, priv, pub_x, out=None):
        """KeyPair#derive per item on a define_mont id -> (x, status): 0 x is pub.mul(priv).getX(),
        1 'public point not validated', 3 'Assertion failed' (validate threw), 2 Z = 0 (the reference
        returns 0).  Validation is tested first; priv (n, 32) is used as it stands; x is zeroed
        unless the status is 0"""
        return self._derive("custom_mont_derive", 32, curve, priv, pub_x, out)

    def custom_mont_derive_dev(self, curve, priv, pub_x, out_x, out_status):
        self._c_rows("custom_mont_derive", True, curve, priv, pub_x, out_x, out_status)

    def custom_mont_ladder(self, curve, k, x, out=None):
        """Point#mul(k) + getX() per item on a define_mont id -> (x, inf): k (n, 32) as it stands
        (neither reduced nor clamped), x (n, 32) reduced mod p; inf = 1 where Z = 0 (the reference's
        getX() returns 0 there), with x zeroed -- the contract of x25519()"""
        return self._derive("custom_mont_ladder", 32, curve, k, x, out)        # (the same operand shapes)

    def custom_mont_ladder_dev(self, curve, k, x, out_x, out_inf):
        self._c_rows("custom_mont_ladder", True, curve, k, x, out_x, out_inf)

    def custom_mont_validate(self, curve, x, out=None):
        """MontCurve#validate per item -> status: 0 true, 1 false (a non-residue, p = 3 mod 4),
        3 'Assertion failed' (a non-residue, p = 1 mod 4: bn.js's Tonelli-Shanks loop throws)"""
        x = _u8(x, (-1, 32))
        st, = self._outs(out, [(x.shape[0],)])
        self._c_rows("custom_mont_validate", False, curve, x, st)
        return st

    def custom_mont_validate_dev(self, curve, x, out_status):
        self._c_rows("custom_mont_validate", True, curve, x, out_status)

    def _derive_wire(self, name, curve, priv, pubs, out, want_err):
        priv = _u8(priv, (-1, 32))
        n = priv.shape[0]
        pubs = _u8(pubs)
        if pubs.ndim != 2 or pubs.shape[0] != n:
            raise ValueError("pubs must be (n, pub_len)")
        if want_err:
            x, st, err = self._outs(out, [(n, 32), (n,), (n,)])
        else:
            (x, st), err = self._outs(out, [(n, 32), (n,)]), None
        self._c_derive_wire(name, False, curve, priv, pubs, x, st, err)
        return x, st, err

    def custom_derive_wire(self, curve, priv, pubs, out=None, want_err=True):
        """KeyPair#derive with the peer keys as SEC1 encodings, rows of `pubs` (n, pub_len) ->
        (x, status, err): status as custom_derive plus 3 = the key did not decode; err the
        statuses of custom_decode_points.  want_err=False passes no err array -> (x, status, None);
        out= is then (x, status)"""
        return self._derive_wire("custom_derive_wire", curve, priv, pubs, out, want_err)

    def custom_derive_wire_dev(self, curve, priv, pubs, out_x, out_status, out_err=None):
        self._c_derive_wire("custom_derive_wire", True, curve, priv, pubs, out_x, out_status, out_err)

    def custom_ed_derive_wire(self, curve, priv, pubs, out=None, want_err=True):
        """custom_ed_derive with the peer keys as SEC1 encodings, rows of `pubs` (n, pub_len) ->
        (x, status, err): status 3 = the key did not decode; err the statuses of
        custom_ed_decode_points.  want_err=False passes no err array -> (x, status, None)"""
        return self._derive_wire("custom_ed_derive_wire", curve, priv, pubs, out, want_err)

    def custom_ed_derive_wire_dev(self, curve, priv, pubs, out_x, out_status, out_err=None):
        self._c_derive_wire("custom_ed_derive_wire", True, curve, priv, pubs, out_x, out_status, out_err)

    # ---- ed25519 EdDSA ------------------------------------------------------------------------------

    @staticmethod
    def _messages(msgs, n):
        """the messages of an EdDSA call -> (bytes, offsets or None, msg_len): an (n, len) array as it
        is, a list of byte strings joined with its n + 1 offsets; never an empty buffer.  The call is
        synchronous in its inputs (a deferred call has staged them when it returns), so the arrays
        need to live no longer than the caller's frame"""
        if isinstance(msgs, np.ndarray) and msgs.ndim == 2:
            m = np.ascontiguousarray(msgs, np.uint8)
            if m.shape[0] != n:
                raise ValueError("msgs has %d rows for %d signatures" % (m.shape[0], n))
            return (m if m.size else np.zeros(1, np.uint8)), None, m.shape[1]
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in msgs])
        return np.frombuffer(b"".join(bytes(x) for x in msgs) or b"\0", dtype=np.uint8), off, 0

    def eddsa_verify(self, msgs, sigs, pubs):
        """ed25519 EdDSA verify.  msgs: list of bytes objects (any lengths) or an (n, len)
        uint8 array; sigs (n, 64), pubs (n, 32) in wire encoding.  -> (ok, err) uint8 arrays"""
        sigs = _u8(sigs, (-1, 64))
        n = sigs.shape[0]
        pubs = _u8(pubs, (n, 32))
        ok, err = self._outs(None, [(n,), (n,)])
        self._c_eddsa_verify(False, *self._messages(msgs, n), sigs, pubs, ok, err)
        return ok, err

    def eddsa_verify_dev(self, msgs, msg_len, sigs, pubs, out_ok, out_err=None, msg_off=None):
        self._c_eddsa_verify(True, msgs, msg_off, msg_len, sigs, pubs, out_ok, out_err)

    def eddsa_verify_base(self, base, msgs, sigs, msg_off=None, out=None):
        """EDDSA#verify(msg, sig, A) of n signatures against the key A of a define_ed_base handle on
        ed25519 (ellgpu_eddsa_verify_base: h walks the key's table, S the curve's own) -> (ok, err):
        what eddsa_verify gives with encodePoint(A) repeated as the key.  The handle:
        define_ed_base("ed25519", xy), the generator alias included.  numpy: msgs as for eddsa_verify
        (a list of bytes objects or an (n, len) array), sigs (n, 64), through host memory.  torch
        device tensors run on the current stream and return at once: msgs (n, len) uint8, or a flat
        uint8 tensor with msg_off a device tensor of n + 1 64-bit offsets; out=(ok,) or (ok, err),
        (n,) uint8, is required then (with out=(ok,) the second result is None)."""
        fn = self._lib.ellgpu_eddsa_verify_base
        if not self._is_tensor(sigs):
            if msg_off is not None:
                raise ValueError("msg_off goes with device tensors: host messages are a list of bytes objects or an (n, len) array")
            sigs = _u8(sigs, (-1, 64))
            n = sigs.shape[0]
            ok, err = self._outs(out, [(n,), (n,)])
            m, off, msg_len = self._messages(msgs, n)
            self._check(fn(self._ctx, int(base), n, m.ctypes.data, None if off is None else off.ctypes.data, int(msg_len),
                           sigs.ctypes.data, ok.ctypes.data, err.ctypes.data, 0, None))
            return ok, err
        import torch
        if sigs.dim() != 2 or sigs.shape[1] != 64:
            raise ValueError("sigs: a contiguous uint8 tensor of shape (n, 64) is needed")
        n = int(sigs.shape[0])
        if out is None or len(out) not in (1, 2):
            raise ValueError("device tensors need out=(ok,) or out=(ok, err): uint8 tensors of shape (%d,)" % n)
        here = torch.device(self.device)
        ops = [(sigs, (n, 64), torch.uint8, "sigs")] + [(o, (n,), torch.uint8, "out " + nm) for o, nm in zip(out, ("ok", "err"))]
        if msg_off is None:
            if not self._is_tensor(msgs) or msgs.dim() != 2:
                raise ValueError("msgs: a contiguous uint8 tensor of shape (n, len) is needed (or a flat one with msg_off)")
            ops.append((msgs, (n, int(msgs.shape[1])), torch.uint8, "msgs"))
        else:
            if not self._is_tensor(msgs) or msgs.dim() != 1:
                raise ValueError("msgs: with msg_off a flat contiguous uint8 tensor is needed")
            ops.append((msgs, tuple(msgs.shape), torch.uint8, "msgs"))
            if not self._is_tensor(msg_off) or msg_off.dtype not in (torch.int64, torch.uint64):
                raise ValueError("msg_off: a contiguous tensor of %d 64-bit offsets is needed" % (n + 1))
            ops.append((msg_off, (n + 1,), msg_off.dtype, "msg_off"))
        for t, shape, dtype, name in ops:
            if not self._is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("%s: a contiguous %s tensor of shape %s is needed" % (name, str(dtype).replace("torch.", ""), shape))
            if t.device != here:
                raise ValueError("%s is on %s, the context on %s" % (name, t.device, here))
        msg_len = 0 if msg_off is not None else int(msgs.shape[1])
        self._check(fn(self._ctx, int(base), n, msgs.data_ptr() if msgs.numel() else None,
                       None if msg_off is None else msg_off.data_ptr(), msg_len, sigs.data_ptr(), out[0].data_ptr(),
                       out[1].data_ptr() if len(out) == 2 else None, 1, self._stream()))
        return out[0], (out[1] if len(out) == 2 else None)

    def eddsa_sign(self, msgs, secrets):
        """ed25519 EdDSA sign from 32-byte secrets (EDDSA#sign with keyFromSecret).  msgs as for
        eddsa_verify.  -> (sig (n, 64), pub (n, 32)) uint8 arrays"""
        secrets = _u8(secrets, (-1, 32))
        n = secrets.shape[0]
        sig, pub = self._outs(None, [(n, 64), (n, 32)])
        self._c_eddsa_sign(False, secrets, *self._messages(msgs, n), sig, pub)
        return sig, pub

    def eddsa_sign_dev(self, secrets, msgs, msg_len, out_sig, out_pub=None, msg_off=None):
        self._c_eddsa_sign(True, secrets, msgs, msg_off, msg_len, out_sig, out_pub)

    # ---- instrumentation ----------------------------------------------------------------------------

    def set_timing(self, on=True):
        self._check(self._lib.ellgpu_ctx_set_timing(self._ctx, 1 if on else 0))

    def get_timing(self):
        """-> {kernel name: (launches, total_ms)} since set_timing(True)"""
        buf = ctypes.create_string_buffer(8192)
        rc = self._lib.ellgpu_ctx_get_timing(self._ctx, buf, 8192)
        if rc < 0:
            self._check(rc)
        out = {}
        for line in buf.value.decode().splitlines():
            name, cnt, ms = line.split()
            out[name] = (int(cnt), float(ms))
        return out

    def probe_valu(self, kind, blocks, iters):
        ms = ctypes.c_double()
        ops = ctypes.c_double()
        self._check(self._lib.ellgpu_probe_valu(self._ctx, kind, blocks, iters, ctypes.byref(ms),
                                                ctypes.byref(ops)))
        return ms.value, ops.value
