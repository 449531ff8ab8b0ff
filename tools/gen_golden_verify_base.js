'use strict';
// Golden vectors for ECDSA verification against a fixed-base table of the signer's key --
// ellgpu_ecdsa_verify_base: every verdict is the reference's own `ec.verify(hash, {r, s}, key)`.
// Runs only where the reference is present (see tools/ref_loader.js); all randomness is SHA-256
// counter mode over a fixed seed and the signatures are made here from seeded nonces, so a rerun
// reproduces tests/golden/verify_base.json byte for byte.
//
//   node tools/gen_golden_verify_base.js [outdir]
//
// Curves: the six presets; as user-defined DOMAINS brainpoolP256r1, secp192k1, secp224k1 (n > p) and
// `cof_p10007` with the parameters tests/golden/fixed_base.json records for it (order 2 q over p =
// 10007, n = q = 4993: floor(p / n) = 2, so JPoint#eqXToP's later candidates r + n < p are common).
//
// Per curve:
//   B        bytes per coordinate, r and s at the C ABI (32 on user-defined ids)
//   p, a, b, n, g   the parameters (user-defined curves; n alone on a preset)
//   keys     [d, x, y] hex, five of them: d = 1 (G itself), n - 1 (-G), 2, and two from the PRNG
//   cases    per key, rows [tag, hash, msg_bits, r, s, verdict]; hash, r, s hex (r, s without leading
//            zeros), msg_bits = options.msgBitLength (0: none), verdict 1 / 0.  Tags:
//     valid20 valid32 valid64   a signature over a hash of that many bytes (_truncateToN's shift)
//     msgbits   a signature made and verified with msgBitLength = n.bitLength() + 5 over 20 bytes
//     high_s    (r, n - s) of valid32
//     flip_r flip_s flip_h   one bit of valid32's r / s / hash flipped
//     r_zero s_zero r_n s_n   out of range
//     r_nm1     r = n - 1 with an arbitrary s
//     u1_zero   a valid signature over a hash with e = n, so e = 0 (mod n) and u1 = 0
//     sum_inf   e = -r d (mod n): u1 G + u2 Q = O, the answer is false
//     x_ge_n    (curves with floor(p / n) >= 1 and n well below p: cof_p10007) a valid signature
//               whose R has x(R) >= n: accepted through eqXToP's second candidate r + n
//     r_ge_p    (n > p: secp224k1) an r in [p, n), which eqXToP reduces mod p first.  An ACCEPTED
//               case of this kind needs x(R) = r - p < n - p ~ 2^113 for an R = k G with k known --
//               a discrete logarithm once the key is fixed -- so this one is a rejection; likewise no
//               R with x(R) >= n can be found on the presets, brainpoolP256r1 or secp192k1.
// The generator refuses to write a fixture in which a tag is missing for a key or in which a key
// does not see both verdicts.

var fs = require('fs');
var path = require('path');
var crypto = require('crypto');
var ref = require('./ref_loader').load();
var elliptic = ref.elliptic;
var BN = ref.BN;
var hash = ref.hash;

var OUT = process.argv[2] || path.join(__dirname, '..', 'tests', 'golden');

function Prng(seed) { this.seed = seed; this.ctr = 0; }
Prng.prototype.bytes = function(n) {
  var out = [];
  while (out.length < n) {
    var h = crypto.createHash('sha256').update(this.seed + ':' + (this.ctr++)).digest();
    for (var i = 0; i < h.length && out.length < n; i++) out.push(h[i]);
  }
  return Buffer.from(out);
};
Prng.prototype.bits = function(b) { return new BN(this.bytes(Math.ceil(b / 8))).maskn(b); };
Prng.prototype.below = function(n) {            // uniform-ish in [1, n)
  for (;;) {
    var k = this.bits(n.bitLength()).umod(n);
    if (!k.isZero()) return k;
  }
};

var PRESETS = [['secp256k1', 32], ['p192', 24], ['p224', 28], ['p256', 32], ['p384', 48], ['p521', 66]];
var USER = [
  { name: 'brainpoolP256r1',
    p: 'a9fb57dba1eea9bc3e660a909d838d726e3bf623d52620282013481d1f6e5377',
    a: '7d5a0975fc2c3057eef67530417affe7fb8055c126dc5c6ce94a4b44f330b5d9',
    b: '26dc5c6ce94a4b44f330b5d9bbd77cbf958416295cf7e1ce6bccdc18ff8c07b6',
    g: ['8bd2aeb9cb7e57cb2c4b482ffc81b7afb9de27e1e3bd23c23a4453bd9ace3262',
      '547ef835c3dac4fd97f8461a14611dc9c27745132ded8e545c1d54c72f046997'],
    n: 'a9fb57dba1eea9bc3e660a909d838d718c397aa3b561a6f7901e0e82974856a7' },
  { name: 'secp192k1', p: 'fffffffffffffffffffffffffffffffffffffffeffffee37', a: '0', b: '3',
    g: ['db4ff10ec057e9ae26b07d0280b7f4341da5d1b1eae06c7d', '9b2f2f6d9c5628a7844163d015be86344082aa88d95e2f9d'],
    n: 'fffffffffffffffffffffffe26f2fc170f69466a74defd8d' },
  { name: 'secp224k1', p: 'fffffffffffffffffffffffffffffffffffffffffffffffeffffe56d', a: '0', b: '5',
    g: ['a1455b334df099df30fc28a169a467e9e47075a90f7e650eb6b7a45c',
      '7e089fed7fba344282cafbd6f7e319f7c0b0bd59e2ca4bdb556d61a5'],
    n: '010000000000000000000000000001dce8d2ec6184caf0a971769fb1f7' },
];
// cof_p10007 as tests/golden/fixed_base.json has it: bases[0] is its G, n the order q of G
(function() {
  var fb = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'fixed_base.json'), 'utf8'));
  var c = fb.filter(function(e) { return e.name === 'cof_p10007'; })[0];
  USER.push({ name: c.name, p: c.p, a: c.a, b: c.b, g: [c.bases[0][0], c.bases[0][1]], n: c.n });
})();

var BASE_TAGS = ['valid20', 'valid32', 'valid64', 'msgbits', 'high_s', 'flip_r', 'flip_s', 'flip_h', 'r_zero', 's_zero',
  'r_n', 's_n', 'r_nm1', 'u1_zero', 'sum_inf'];

function gen(name, B, ec, extra) {
  var curve = ec.curve, G = ec.g, n = ec.n, p = curve.p;
  var rng = new Prng('ellgpu-golden-v1:verify-base:' + name);
  var nbits = n.bitLength();
  var o = { name: name, B: B };
  Object.keys(extra || {}).forEach(function(f) { o[f] = extra[f]; });
  o.n = n.toString(16);
  var ds = [new BN(1), n.subn(1), new BN(2), rng.below(n), rng.below(n)];
  var want = BASE_TAGS.slice();
  var cof = p.div(n).cmpn(1) >= 0 && p.sub(n).bitLength() > p.bitLength() - 8;     // n well below p
  if (cof) want.push('x_ge_n');
  if (n.cmp(p) > 0) want.push('r_ge_p');
  o.keys = [];
  o.cases = [];
  ds.forEach(function(d) {
    var Q = G.mul(d);
    var key = ec.keyFromPublic({ x: Q.getX().toString(16), y: Q.getY().toString(16) }, 'hex');
    o.keys.push([d.toString(16), Q.getX().toString(16, 2 * B), Q.getY().toString(16, 2 * B)]);
    var rows = [];
    function rec(tag, h, bits, r, s) {
      var ok = ec.verify(h, { r: r.toString(16), s: s.toString(16) }, key, undefined, bits ? { msgBitLength: bits } : undefined);
      rows.push([tag, h.toString('hex'), bits || 0, r.toString(16), s.toString(16), ok ? 1 : 0]);
      return ok;
    }
    // (r, s) over h with the nonce k: EC#sign's equations (ec/index.js:159-171)
    function signWith(k, h, bits) {
      var e = ec._truncateToN(h, false, bits || undefined);
      var R = G.mul(k);
      if (R.isInfinity()) return null;
      var r = R.getX().umod(n);
      var s = k.invm(n).mul(e.add(d.mul(r))).umod(n);
      if (r.isZero() || s.isZero()) return null;
      return { r: r, s: s, R: R };
    }
    function sign(h, bits, accept) {
      for (var t = 0; t < 4096; t++) {
        var sig = signWith(rng.below(n), h, bits);
        if (sig && (!accept || accept(sig))) return sig;
      }
      throw new Error(name + ': no nonce found');
    }
    // a hash of B bytes that _truncateToN brings to e exactly (e < 2^nbits)
    function hashOf(e) { return Buffer.from(e.ushln(8 * B - nbits).toArray('be', B)); }
    var h20 = rng.bytes(20), h32 = rng.bytes(32), h64 = rng.bytes(64);
    var s20 = sign(h20, 0), s32 = sign(h32, 0), s64 = sign(h64, 0);
    if (!rec('valid20', h20, 0, s20.r, s20.s) || !rec('valid32', h32, 0, s32.r, s32.s) || !rec('valid64', h64, 0, s64.r, s64.s))
      throw new Error(name + ': a signature made here is not valid');
    var hm = rng.bytes(20), sm = sign(hm, nbits + 5);
    if (!rec('msgbits', hm, nbits + 5, sm.r, sm.s)) throw new Error(name + ': msgbits signature is not valid');
    if (!rec('high_s', h32, 0, s32.r, n.sub(s32.s))) throw new Error(name + ': the high-s twin is not valid');
    var bit = rng.bits(16).toNumber();
    rec('flip_r', h32, 0, s32.r.xor(new BN(1).ushln(bit % (nbits - 1))), s32.s);
    rec('flip_s', h32, 0, s32.r, s32.s.xor(new BN(1).ushln((bit >> 3) % (nbits - 1))));
    var hf = Buffer.from(h32);
    hf[0] ^= 0x80 >> (bit & 7);                        // one of the hash's top eight bits: inside every truncation
    rec('flip_h', hf, 0, s32.r, s32.s);
    rec('r_zero', h32, 0, new BN(0), s32.s);
    rec('s_zero', h32, 0, s32.r, new BN(0));
    rec('r_n', h32, 0, n, s32.s);
    rec('s_n', h32, 0, s32.r, n);
    rec('r_nm1', h32, 0, n.subn(1), rng.below(n));
    // e = n: _truncateToN subtracts n once, so e = 0 and u1 = 0; s = r d / k
    var hz = hashOf(n), sz = sign(hz, 0);
    if (!ec._truncateToN(hz).isZero()) throw new Error(name + ': e is not 0 (mod n)');
    if (!rec('u1_zero', hz, 0, sz.r, sz.s)) throw new Error(name + ': the u1 = 0 signature is not valid');
    // e = -r d (mod n): u1 G + u2 Q = (e + r d) / s G = O
    var r0 = rng.below(n), s0 = rng.below(n);
    var e0 = n.sub(r0.mul(d).umod(n)).umod(n);
    var hi = hashOf(e0);
    if (ec._truncateToN(hi).cmp(e0) !== 0) throw new Error(name + ': e is not -r d');
    if (rec('sum_inf', hi, 0, r0, s0)) throw new Error(name + ': R = O was accepted');
    if (cof) {
      var hx = rng.bytes(32);
      var sx = sign(hx, 0, function(sig) { return sig.R.getX().cmp(n) >= 0; });
      if (!rec('x_ge_n', hx, 0, sx.r, sx.s)) throw new Error(name + ': x(R) >= n was not accepted');
    }
    if (n.cmp(p) > 0) {
      var rp = p.add(rng.below(n.sub(p)));
      rec('r_ge_p', h32, 0, rp, s32.s);
    }
    // every category, both verdicts
    want.forEach(function(tag) {
      if (!rows.some(function(c) { return c[0] === tag; })) throw new Error(name + ': no case ' + tag + ' for key ' + d.toString(16));
    });
    [0, 1].forEach(function(v) {
      if (!rows.some(function(c) { return c[5] === v; })) throw new Error(name + ': verdict ' + v + ' never occurs for key ' + d.toString(16));
    });
    o.cases.push(rows);
  });
  o.tags = want;
  return o;
}

var out = [];
PRESETS.forEach(function(nb) { out.push(gen(nb[0], nb[1], new elliptic.ec(nb[0]))); });
USER.forEach(function(s) {
  var pc = new elliptic.curves.PresetCurve({ type: 'short', prime: null, p: s.p, a: s.a, b: s.b, n: s.n, hash: hash.sha256,
    gRed: false, g: s.g });
  out.push(gen(s.name, 32, new elliptic.ec(pc), { p: s.p, a: s.a, b: s.b, g: s.g }));
});
['secp224k1', 'cof_p10007'].forEach(function(nm) {
  var c = out.filter(function(e) { return e.name === nm; })[0];
  var tag = nm === 'cof_p10007' ? 'x_ge_n' : 'r_ge_p';
  if (c.tags.indexOf(tag) < 0) throw new Error(nm + ': ' + tag + ' is not among its categories');
});

var file = path.join(OUT, 'verify_base.json');
fs.writeFileSync(file, JSON.stringify(out).replace(/("name"|"keys"|"cases"|"tags"):/g, '\n$1:').replace(/\],\[/g, '],\n[') + '\n');
out.forEach(function(c) {
  var all = [].concat.apply([], c.cases);
  console.log(c.name + ': ' + c.keys.length + ' keys x ' + c.cases[0].length + ' cases, ' +
    all.filter(function(r) { return r[5]; }).length + ' accepted of ' + all.length);
});
console.log('wrote ' + file + ' (' + fs.statSync(file).size + ' bytes)');
