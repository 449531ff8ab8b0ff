'use strict';
// Golden vectors for the WIRE FORMATS on user-defined short curves: BaseCurve#decodePoint /
// ShortCurve#pointFromX on SEC1 encodings whose coordinates are p.byteLength() bytes, and
// EC#verify(msg, derSignature, encodedKey) on user-defined domains -- every status, point, verdict
// and thrown message from the reference itself.  Runs only where the reference is present (see
// tools/ref_loader.js); all randomness is SHA-256 counter mode over a fixed seed and the
// signatures are the reference's deterministic (RFC 6979) ones, so a rerun reproduces
// tests/golden/custom_wire.json byte for byte.
//
//   node tools/gen_golden_custom_wire.js [outdir]
//
// Curves: the five domains of custom_ecdsa.json (brainpoolP256r1, secp192k1, secp112r1: p = 3 mod
// 4; secp224k1, w25519_like: p = 1 mod 4 with p - 1 = q 2^2), NIST P-224's parameters as a
// user-defined domain (p - 1 = q 2^96: the deep Tonelli-Shanks schedule of Red#sqrt), and two
// plain curves y^2 = x^3 + 2x + 3 (decode only) over primes with p - 1 = q 2^3 and q 2^32.
//
// `decode`: enc = the encoding (hex) -> st (0 point, 1 'Unknown point format', 2 'invalid point',
// 3 'Assertion failed') with x, y (64 hex digits) or msg = the message thrown.
// `wire`: h = digest, bits = options.msgBitLength (0: none), der, key (hex) -> ok = the verdict,
// or msg = the message EC#verify throws (ok = 0).  tag = what the case exercises.

var fs = require('fs');
var path = require('path');
var crypto = require('crypto');
var ref = require('./ref_loader').load();
var elliptic = ref.elliptic;
var BN = ref.BN;
var Signature = ref.Signature;
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
function hex(arr) { return Buffer.from(arr).toString('hex'); }

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
  // NIST P-224 (FIPS 186-4 D.1.2.2) given as a user-defined curve: the generic Mont context
  { name: 'p224_user', p: 'ffffffffffffffffffffffffffffffff000000000000000000000001',
    a: 'fffffffffffffffffffffffffffffffefffffffffffffffffffffffe',
    b: 'b4050a850c04b3abf54132565044b0b7d7bfd8ba270b39432355ffb4',
    g: ['b70e0cbd6bb4bf7f321390b94a03c1d356c21122343280d6115c1d21',
      'bd376388b5f723fb4c22dfe6cd4375a05a07476444d5819985007e34'],
    n: 'ffffffffffffffffffffffffffff16a2e0b8f03e13dd29455c5c2a3d' },
  // decode only
  { name: 'plain_s3', p: 'ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffee09', a: '2', b: '3' },
  { name: 'plain_s32', p: 'ffffffffffffffffffffffffffffffffffffffffffffffffffffffd500000001', a: '2', b: '3' },
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

var STATUS = { 'Unknown point format': 1, 'invalid point': 2, 'Assertion failed': 3 };

function genDecode(curve, rng) {
  var p = curve.p, PL = p.byteLength();
  var out = [];
  function rec(tag, enc) {
    var c = { tag: tag, enc: hex(enc) };
    try {
      var P = curve.decodePoint(enc);
      c.st = 0;
      c.x = hex32(P.getX());
      c.y = hex32(P.getY());
    } catch (e) {
      if (!(e.message in STATUS)) throw e;
      c.st = STATUS[e.message];
      c.msg = e.message;
    }
    out.push(c);
  }
  function coord(v) { return v.toArray('be', PL); }
  function hasY(x) {
    try { curve.pointFromX(x, false); return true; } catch (e) { return false; }
  }
  function randomX(want) {
    for (;;) {
      var x = rng.below(p);
      if (hasY(x) === want) return x;
    }
  }
  var i;
  // points of the curve under every prefix; the hybrid prefixes with and against y's parity
  for (i = 0; i < 2; i++) {
    var P = curve.pointFromX(randomX(true), i & 1);
    var X = coord(P.getX()), Y = coord(P.getY());
    var odd = P.getY().isOdd() ? 1 : 0;
    rec('compressed', [2 + odd].concat(X));
    rec('compressed_other_y', [3 - odd].concat(X));
    rec('uncompressed', [4].concat(X, Y));
    rec('hybrid', [6 + odd].concat(X, Y));
    rec('hybrid_parity', [7 - odd].concat(X, Y));
    if (i === 0) {
      // unknown prefixes at both lengths, known prefixes at the other's length, wrong lengths
      [0, 5, 8].forEach(function(t) {
        rec('prefix', [t].concat(X));
        rec('prefix', [t].concat(X, Y));
      });
      rec('length', [4].concat(X));
      rec('length', [2].concat(X, Y));
      rec('length', [2 + odd].concat(X.slice(1)));
      rec('length', [2 + odd].concat([0], X));
      rec('length', [4].concat(X, Y.slice(1)));
      rec('length', [4].concat(X, Y, [0]));
      rec('length', [6 + odd].concat(X, Y, [odd]));
      rec('length', [2]);
      rec('length', [4]);
    }
  }
  // compressed x without a y
  for (i = 0; i < 2; i++) {
    var xn = coord(randomX(false));
    rec('no_y', [2 + (i & 1)].concat(xn));
  }
  // uncompressed encodings are not tested against the curve equation
  rec('off_curve', [4].concat(coord(rng.below(p)), coord(rng.below(p))));
  rec('off_curve_hybrid', [6].concat(coord(rng.below(p)), coord(rng.below(p).iuor(new BN(1)).isubn(1))));
  // x = 0, x = p - 1 (rhs = 0 where a = 2, b = 3: x^3 + 2x + 3 = (x + 1)(x^2 - x + 3)), x = 1
  rec('x_zero', [2].concat(coord(new BN(0))));
  rec('x_zero', [3].concat(coord(new BN(0))));
  rec('x_p_minus_1', [2].concat(coord(p.subn(1))));
  rec('x_p_minus_1', [3].concat(coord(p.subn(1))));
  rec('x_one', [3].concat(coord(new BN(1))));
  rec('origin', [4].concat(coord(new BN(0)), coord(new BN(0))));
  // coordinates >= p, where PL bytes hold them: reduced like toRed
  var top = new BN(1).ushln(8 * PL);
  for (i = 0; i < 6; i++) {
    var xb = p.addn(i);
    if (xb.cmp(top) >= 0) break;
    rec('x_ge_p', [2 + (i & 1)].concat(coord(xb)));
    if (i === 1 && p.addn(2).cmp(top) < 0) rec('xy_ge_p', [4].concat(coord(xb), coord(p.addn(2))));
  }
  if (top.subn(1).cmp(p) > 0) {
    rec('x_all_ones', [2].concat(coord(top.subn(1))));
    rec('xy_all_ones', [7].concat(coord(top.subn(1)), coord(top.subn(1))));
  }
  return out;
}

function genWire(spec, ec, rng) {
  var curve = ec.curve, G = ec.g, n = ec.n, p = curve.p;
  var out = [];
  function rec(tag, h, bits, der, key) {
    var c = { tag: tag, h: h.toString('hex'), bits: bits || 0, der: hex(der), key: hex(key) };
    try {
      c.ok = ec.verify(h, c.der, c.key, 'hex', bits ? { msgBitLength: bits } : undefined) ? 1 : 0;
    } catch (e) {
      c.ok = 0;
      c.msg = e.message;
    }
    out.push(c);
  }
  function keypair() { return ec.keyFromPrivate(rng.below(n)); }
  // the reference's own sign; where it cannot sign (HmacDRBG wants 192 bits of key, and a digest
  // that msgBitLength leaves wider than n does not fit its nonce: secp112r1), the same equations
  // with a nonce from the seeded stream
  function sign(kp, h, bits) {
    try {
      return kp.sign(h, bits ? { msgBitLength: bits } : undefined);
    } catch (e) {
      if (!/entropy|byte array longer/.test(e.message)) throw e;
      var m = ec._truncateToN(h, false, bits || undefined);
      for (;;) {
        var k = rng.below(n);
        var r = G.mul(k).getX().umod(n);
        var s = k.invm(n).mul(m.add(kp.getPrivate().mul(r))).umod(n);
        if (!r.isZero() && !s.isZero()) return { r: r, s: s };
      }
    }
  }
  function der(r, s) { return new Signature({ r: r, s: s }).toDER(); }
  function enc(P, form) {
    if (form === 'hybrid') {
      var e = P.encode('array', false);
      e[0] = P.getY().isOdd() ? 7 : 6;
      return e;
    }
    return P.encode('array', form === 'compressed');
  }
  function signed(tag, len, bits, form) {
    var kp = keypair();
    var h = rng.bytes(len);
    var sig = sign(kp, h, bits);
    rec(tag, h, bits, der(sig.r, sig.s), enc(kp.getPublic(), form));
    return { kp: kp, h: h, r: sig.r, s: sig.s };
  }
  var i;
  for (i = 0; i < 2; i++) signed('valid_compressed', 32, 0, 'compressed');
  signed('valid_uncompressed', 32, 0, 'uncompressed');
  signed('valid_hybrid', 32, 0, 'hybrid');
  signed('valid_sha1', 20, 0, 'compressed');
  signed('valid_sha512', 64, 0, 'compressed');
  if (spec.name === 'secp112r1') {
    // a 20-byte digest over a 112-bit n, without and with msgBitLength
    signed('digest20', 20, 0, 'compressed');
    signed('digest20_msgbits', 20, 100, 'compressed');
    signed('digest20_msgbits', 20, 160, 'uncompressed');
  }
  var base = signed('valid_compressed', 32, 0, 'compressed');
  var Q = base.kp.getPublic();
  var key = enc(Q, 'compressed'), good = der(base.r, base.s);
  var other = keypair().getPublic();
  // one of r, s, the digest, the key disturbed
  rec('wrong_r', base.h, 0, der(base.r.addn(1).umod(n), base.s), key);
  rec('wrong_s', base.h, 0, der(base.r, base.s.addn(1).umod(n)), key);
  rec('wrong_digest', rng.bytes(32), 0, good, key);
  rec('wrong_key', base.h, 0, good, enc(other, 'compressed'));
  rec('wrong_key_sign', base.h, 0, good, enc(Q.neg(), 'compressed'));
  rec('msgbits_mismatch', base.h, 200, good, key);
  // keys the decoder refuses (thrown before the signature is looked at) -- with a good and a bad DER
  var xn;
  for (;;) {
    xn = rng.below(p);
    try { curve.pointFromX(xn, false); } catch (e) { break; }
  }
  var PL = p.byteLength();
  var noY = [2].concat(xn.toArray('be', PL));
  var hyb = enc(Q, 'hybrid');
  hyb[0] ^= 1;
  rec('key_no_y', base.h, 0, good, noY);
  rec('key_no_y_bad_der', base.h, 0, [0x31].concat(good.slice(1)), noY);
  rec('key_hybrid_parity', base.h, 0, good, hyb);
  rec('key_prefix', base.h, 0, good, [5].concat(key.slice(1)));
  rec('key_prefix_bad_der', base.h, 0, [], [5].concat(key.slice(1)));
  rec('key_length', base.h, 0, good, key.concat([0]));
  // an uncompressed key off the curve: the reference computes with it (recorded as it answers)
  rec('key_off_curve', base.h, 0, good, [4].concat(Q.getX().toArray('be', PL), Q.getY().addn(1).umod(p).toArray('be', PL)));
  rec('key_off_curve', base.h, 0, good, [4].concat(new BN(1).toArray('be', PL), new BN(1).toArray('be', PL)));
  // malformed DER: every `return false` of Signature#_importDER and getLength
  var rA = base.r.toArray(), sA = base.s.toArray();
  if (rA[0] & 0x80) rA = [0].concat(rA);
  if (sA[0] & 0x80) sA = [0].concat(sA);
  function seq(body, lenBytes) { return [0x30].concat(lenBytes || [body.length], body); }
  function int_(v, lenBytes) { return [2].concat(lenBytes || [v.length], v); }
  var body = int_(rA).concat(int_(sA));
  rec('der_empty', base.h, 0, [], key);
  rec('der_tag', base.h, 0, [0x31].concat(good.slice(1)), key);
  rec('der_len_indefinite', base.h, 0, seq(body, [0x80]), key);
  rec('der_len_5_octets', base.h, 0, seq(body, [0x85, 0, 0, 0, 0, body.length]), key);
  rec('der_len_zero_octet', base.h, 0, seq(body, [0x82, 0, body.length]), key);
  rec('der_len_not_minimal', base.h, 0, seq(body, [0x81, body.length]), key);
  rec('der_len_short', base.h, 0, seq(body, [body.length - 1]), key);
  rec('der_len_long', base.h, 0, seq(body, [body.length + 1]), key);
  rec('der_trailing', base.h, 0, good.concat([0]), key);
  rec('der_truncated', base.h, 0, good.slice(0, good.length - 1), key);
  rec('der_r_tag', base.h, 0, seq([3].concat([rA.length], rA, int_(sA))), key);
  rec('der_r_len_long_form', base.h, 0, seq(int_(rA, [0x81, rA.length]).concat(int_(sA))), key);
  rec('der_r_negative', base.h, 0, seq(int_([0x80].concat(rA.slice(1))).concat(int_(sA))), key);
  rec('der_r_overruns', base.h, 0, seq(int_(rA, [rA.length + sA.length + 4]).concat(int_(sA))), key);
  rec('der_s_tag', base.h, 0, seq(int_(rA).concat([4], [sA.length], sA)), key);
  rec('der_s_len', base.h, 0, seq(int_(rA).concat(int_(sA, [sA.length - 1]))), key);
  rec('der_s_len_indefinite', base.h, 0, seq(int_(rA).concat(int_(sA, [0x80]))), key);
  rec('der_s_negative', base.h, 0, seq(int_(rA).concat(int_([0xff].concat(sA.slice(1))))), key);
  rec('der_r_zero_padded', base.h, 0, seq(int_([0, 0x7f].concat(rA.slice(1))).concat(int_(sA))), key);
  rec('der_s_zero_padded', base.h, 0, seq(int_(rA).concat(int_([0, 0x01].concat(sA)))), key);
  rec('der_r_zero', base.h, 0, seq(int_([0]).concat(int_(sA))), key);
  rec('der_s_zero', base.h, 0, seq(int_(rA).concat(int_([0]))), key);
  rec('der_r_empty', base.h, 0, seq(int_([]).concat(int_(sA))), key);
  rec('der_missing_s', base.h, 0, seq(int_(rA)), key);
  // r or s out of range: n, n + 1, 2^256 - 1, and wider than 32 bytes
  var wide = [n.clone(), n.addn(1), new BN(1).ushln(256).subn(1), new BN(1).ushln(256).add(base.r),
    new BN(1).ushln(263)];
  wide.forEach(function(v) {
    rec('r_range', base.h, 0, der(v, base.s), key);
    rec('s_range', base.h, 0, der(base.r, v), key);
  });
  rec('r_one', base.h, 0, der(new BN(1), base.s), key);
  rec('s_n_minus_1', base.h, 0, der(base.r, n.subn(1)), key);
  // n > p: an r in [p, n) -- r.toRed(red) in JPoint#eqXToP reduces r mod p, so r = x(R) + p is accepted
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
      rec('r_is_x_plus_p', h2, 0, der(r2, s2), enc(Q2, cnt & 1 ? 'hybrid' : 'compressed'));
      rec('r_is_x', h2, 0, der(Rs.getX(), s2), enc(Q2, 'compressed'));
      cnt++;
    }
  }
  return out;
}

function gen(spec) {
  var rng = new Prng('ellgpu-golden-v1:custom-wire:' + spec.name);
  var ec = spec.n ? build(spec) : null;
  var curve = ec ? ec.curve : new elliptic.curve.short({ p: spec.p, a: spec.a, b: spec.b });
  var o = { name: spec.name, p: hex32(curve.p), a: hex32(curve.a.fromRed()), b: hex32(curve.b.fromRed()),
    pl: curve.p.byteLength() };
  if (ec) {
    o.n = hex32(ec.n);
    o.g = { x: hex32(ec.g.getX()), y: hex32(ec.g.getY()) };
  }
  o.decode = genDecode(curve, rng);
  if (ec) o.wire = genWire(spec, ec, rng);
  return o;
}

// the P-224 parameters above are the reference's own preset's
(function() {
  var c = elliptic.curves.p224, s = CURVES[5];
  if (c.curve.p.toString(16) !== s.p || c.n.toString(16) !== s.n || c.g.getX().toString(16) !== s.g[0])
    throw new Error('p224_user does not match the p224 preset');
})();

var out = CURVES.map(gen);
var file = path.join(OUT, 'custom_wire.json');
fs.writeFileSync(file, JSON.stringify(out).replace(/\{"tag"/g, '\n{"tag"').replace(/\],"wire"/g, '\n],"wire"') + '\n');
out.forEach(function(c) {
  var st = [0, 0, 0, 0];
  c.decode.forEach(function(d) { st[d.st]++; });
  var w = c.wire || [];
  console.log(c.name + ': ' + c.decode.length + ' decode cases (status 0/1/2/3: ' + st.join('/') + '), ' + w.length +
    ' wire cases (' + w.filter(function(v) { return v.ok; }).length + ' accepted, ' +
    w.filter(function(v) { return v.msg; }).length + ' thrown)');
});
console.log('wrote ' + file);
