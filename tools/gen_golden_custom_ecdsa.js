'use strict';
// Golden vectors for ECDSA on USER-DEFINED domains (`new elliptic.ec(new PresetCurve({type:
// 'short', p, a, b, n, g}))` with parameters that are no preset): EC#verify's verdicts, k*G and
// mulAdd with G, all from the reference itself.  Runs only where the reference is present (see
// tools/ref_loader.js); all randomness is SHA-256 counter mode over a fixed seed and the
// signatures are the reference's deterministic (RFC 6979) ones, so a rerun reproduces
// tests/golden/custom_ecdsa.json byte for byte.
//
//   node tools/gen_golden_custom_ecdsa.js [outdir]
//
// Curves: brainpoolP256r1 and secp192k1 (as in custom_short.json), secp112r1 (a 112-bit n
// above p), secp224k1 (n > p by about 2^113: JPoint#eqXToP reduces r mod p, so r = x + p is
// ACCEPTED) and w25519_like with its prime-order subgroup (cofactor 8: eqXToP's later candidates).
//
// Verify cases (`verify`): h = digest hex, bits = options.msgBitLength (0: none), r, s, q = key,
// ok = the reference's verdict, tag = what the case exercises.  `mulg`: k -> k*G; `muladd`:
// k1*G + k2*Q (Point#mulAdd).

var fs = require('fs');
var path = require('path');
var crypto = require('crypto');
var ref = require('./ref_loader').load();
var elliptic = ref.elliptic;
var BN = ref.BN;
var hash = ref.breq(19);

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

function hex32(bn) { return bn.toString(16, 64); }
function aff(p) {
  if (p.isInfinity()) return { inf: true };
  if (p.z !== undefined) p = p.toP();
  return { x: hex32(p.getX()), y: hex32(p.getY()) };
}

// Wei25519 (curve25519 in short Weierstrass form, group order 8n).  custom_short.json's w25519_like
// spells a with two more digits -- a different curve, whose order is not 8n -- so this one takes
// the 64-digit a.
var W25519 = { p: '7fffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffed',
  a: '2aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa984914a144',
  b: '7b425ed097b425ed097b425ed097b425ed097b425ed097b4260b5e9c7710c864' };

var CURVES = [
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
  { name: 'secp112r1', p: 'db7c2abf62e35e668076bead208b', a: 'db7c2abf62e35e668076bead2088',
    b: '659ef8ba043916eede8911702b22', g: ['09487239995a5ee76b55f9c2f098', 'a89ce5af8724c0a23e0e0ff77500'],
    n: 'db7c2abf62e35e7628dfac6561c5' },
  { name: 'secp224k1', p: 'fffffffffffffffffffffffffffffffffffffffffffffffeffffe56d', a: '0', b: '5',
    g: ['a1455b334df099df30fc28a169a467e9e47075a90f7e650eb6b7a45c',
      '7e089fed7fba344282cafbd6f7e319f7c0b0bd59e2ca4bdb556d61a5'],
    n: '010000000000000000000000000001dce8d2ec6184caf0a971769fb1f7' },
  { name: 'w25519_like', p: W25519.p, a: W25519.a, b: W25519.b,
    n: new BN(1).ushln(252).add(new BN('27742317777372353535851937790883648493', 10)).toString(16) },
];

function build(spec) {
  var g = spec.g;
  if (!g) {
    // 8 * (the first point with a small x): a generator of the order-n subgroup
    var c = new elliptic.curve.short({ p: spec.p, a: spec.a, b: spec.b });
    var P;
    for (var x = 1; ; x++) {
      try { P = c.pointFromX(new BN(x), false); } catch (e) { continue; }
      P = P.mul(new BN(8));
      if (!P.isInfinity()) break;
    }
    g = [P.getX().toString(16), P.getY().toString(16)];
  }
  var pc = new elliptic.curves.PresetCurve({ type: 'short', prime: null, p: spec.p, a: spec.a, b: spec.b,
    n: spec.n, hash: hash.sha256, gRed: false, g: g });
  return new elliptic.ec(pc);
}

function gen(spec) {
  var ec = build(spec);
  var curve = ec.curve, G = ec.g, n = ec.n, p = curve.p;
  var rng = new Prng('ellgpu-golden-v1:custom-ecdsa:' + spec.name);
  var verify = [], mulg = [], muladd = [];
  function pt(P) { return { x: hex32(P.getX()), y: hex32(P.getY()) }; }
  function rec(tag, h, bits, r, s, Q) {
    var q = pt(Q);
    var opts = bits ? { msgBitLength: bits } : undefined;
    var key = ec.keyFromPublic({ x: q.x, y: q.y }, 'hex');
    var ok = ec.verify(h, { r: r.toString(16), s: s.toString(16) }, key, undefined, opts);
    verify.push({ tag: tag, h: h.toString('hex'), bits: bits || 0, r: hex32(r), s: hex32(s), q: q, ok: ok ? 1 : 0 });
  }
  function keypair() { return ec.keyFromPrivate(rng.below(n)); }
  // the reference's own sign; where it cannot sign (HmacDRBG wants 192 bits of key: secp112r1),
  // the same equations with a nonce from the seeded stream
  function sign(kp, h, bits) {
    try {
      return kp.sign(h, bits ? { msgBitLength: bits } : undefined);
    } catch (e) {
      if (!/entropy/.test(e.message)) throw e;
      var m = ec._truncateToN(h, false, bits || undefined);
      for (;;) {
        var k = rng.below(n);
        var r = G.mul(k).getX().umod(n);
        var s = k.invm(n).mul(m.add(kp.getPrivate().mul(r))).umod(n);
        if (!r.isZero() && !s.isZero()) return { r: r, s: s };
      }
    }
  }
  function signed(tag, len, bits) {
    var kp = keypair();
    var h = rng.bytes(len);
    var sig = sign(kp, h, bits);
    rec(tag, h, bits, sig.r, sig.s, kp.getPublic());
    return { kp: kp, h: h, sig: sig };
  }
  var i;
  // valid signatures, digests of 20 / 32 / 48 / 64 bytes
  [20, 32, 48, 64].forEach(function(len) {
    for (i = 0; i < 3; i++) signed('valid', len, 0);
  });
  var base = signed('valid', 32, 0);
  // msgBitLength: signed with the same option where the reference can sign (its nonce wants the
  // truncated digest within n's bytes), else base's signature over the new digest (a rejection)
  [[64, 512], [64, 300], [32, 256], [32, 160], [20, 100], [8, 8], [64, 100]].forEach(function(lb) {
    try {
      signed('msgbits', lb[0], lb[1]);
    } catch (e) {
      rec('msgbits', rng.bytes(lb[0]), lb[1], base.sig.r, base.sig.s, base.kp.getPublic());
    }
  });
  var other = keypair();
  rec('wrong_msg', rng.bytes(32), 0, base.sig.r, base.sig.s, base.kp.getPublic());
  rec('wrong_key', base.h, 0, base.sig.r, base.sig.s, other.getPublic());
  rec('msgbits_mismatch', base.h, 200, base.sig.r, base.sig.s, base.kp.getPublic());
  // r or s out of range
  var bad = [new BN(0), n.clone(), n.addn(1), new BN(1).ushln(256).subn(1)];
  bad.forEach(function(v) {
    rec('r_range', base.h, 0, v, base.sig.s, base.kp.getPublic());
    rec('s_range', base.h, 0, base.sig.r, v, base.kp.getPublic());
  });
  rec('r_one', base.h, 0, new BN(1), base.sig.s, base.kp.getPublic());
  rec('s_n_minus_1', base.h, 0, base.sig.r, n.subn(1), base.kp.getPublic());
  // off-curve keys (the reference's answer, whatever it computes)
  var Q0 = base.kp.getPublic();
  var offs = [curve.point(Q0.getX(), Q0.getY().addn(1)), curve.point(new BN(1), new BN(1))];
  offs.forEach(function(Qo) { rec('off_curve', base.h, 0, base.sig.r, base.sig.s, Qo); });
  // u1 G + u2 Q = O: Q = -(e / r) G
  for (i = 0; i < 3; i++) {
    var h0 = rng.bytes(32);
    var e0 = ec._truncateToN(h0);
    var r0 = rng.below(n), s0 = rng.below(n);
    var c0 = e0.mul(r0.invm(n)).umod(n);
    if (c0.isZero()) continue;
    rec('sum_infinity', h0, 0, r0, s0, G.mul(c0).neg());
  }
  // x(R) >= n with r = x mod n: Q = r^-1 (s R - e G), so that u1 G + u2 Q = R
  var found = 0;
  for (i = 0; i < 64 && found < 4; i++) {
    var R = G.mul(rng.below(n));
    if (R.getX().cmp(n) < 0) continue;
    var r1 = R.getX().umod(n);
    if (r1.isZero()) continue;
    var h1 = rng.bytes(32), e1 = ec._truncateToN(h1), s1 = rng.below(n);
    var Q1 = R.mul(s1).add(G.mul(e1).neg()).mul(r1.invm(n));
    rec('x_ge_n', h1, 0, r1, s1, Q1);
    found++;
  }
  // n > p: r = x(R) + p for an R with a small x -- r.toRed(red) in eqXToP reduces r mod p
  if (n.cmp(p) > 0) {
    var cnt = 0;
    for (var x = 1; cnt < 3 && x < 1000; x++) {
      var Rs;
      try { Rs = curve.pointFromX(new BN(x), x & 1); } catch (e) { continue; }
      if (!Rs.mul(n).isInfinity()) continue;
      var r2 = Rs.getX().add(p);
      if (r2.cmp(n) >= 0) continue;
      var h2 = rng.bytes(32), e2 = ec._truncateToN(h2), s2 = rng.below(n);
      var Q2 = Rs.mul(s2).add(G.mul(e2).neg()).mul(r2.invm(n));
      rec('r_is_x_plus_p', h2, 0, r2, s2, Q2);
      rec('r_is_x', h2, 0, Rs.getX(), s2, Q2);
      cnt++;
    }
  }
  // k * G
  var ks = [new BN(0), new BN(1), new BN(2), new BN(255), new BN(256), n.subn(1), n.clone(), n.addn(1),
    new BN(1).ushln(255), new BN(1).ushln(256).subn(1)];
  for (i = 0; i < 10; i++) ks.push(rng.bits(256));
  ks.forEach(function(k) { mulg.push({ k: hex32(k), r: aff(G.mul(k)) }); });
  // k1 G + k2 Q
  var pairs = [[new BN(0), new BN(5)], [new BN(3), new BN(0)], [n.subn(1), new BN(1)], [n.clone(), n.clone()]];
  for (i = 0; i < 8; i++) pairs.push([rng.bits(256), rng.bits(256)]);
  pairs.forEach(function(kk, j) {
    var Q = j === 2 ? G : keypair().getPublic();
    muladd.push({ k1: hex32(kk[0]), k2: hex32(kk[1]), q: pt(Q), r: aff(G.mulAdd(kk[0], Q, kk[1])) });
  });
  return { name: spec.name, p: hex32(p), a: hex32(curve.a.fromRed()), b: hex32(curve.b.fromRed()), n: hex32(n),
    g: pt(G), verify: verify, mulg: mulg, muladd: muladd };
}

var out = CURVES.map(gen);
var file = path.join(OUT, 'custom_ecdsa.json');
fs.writeFileSync(file, JSON.stringify(out, null, 1) + '\n');
out.forEach(function(c) {
  var acc = c.verify.filter(function(v) { return v.ok; }).length;
  console.log(c.name + ': ' + c.verify.length + ' verify cases (' + acc + ' accepted), ' + c.mulg.length +
    ' k*G, ' + c.muladd.length + ' mulAdd');
});
console.log('wrote ' + file);
