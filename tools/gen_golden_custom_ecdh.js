'use strict';
// Golden vectors for the key side on user-defined short-curve domains -- ellgpu_custom_derive,
// _custom_derive_wire, _custom_validate, _custom_encode_points: every shared secret, status, thrown
// message and encoding from the reference itself.  Runs only where the reference is present (see
// tools/ref_loader.js); all randomness is SHA-256 counter mode over a fixed seed, so a rerun
// reproduces tests/golden/custom_ecdh.json byte for byte.
//
//   node tools/gen_golden_custom_ecdh.js [outdir]
//
// Domains: the six of custom_recover.json -- brainpoolP256r1, secp192k1, secp112r1 (p = 3 mod 4),
// secp224k1 (n > p, p = 5 mod 8), w25519_like (cofactor 8, p = 5 mod 8), p224_user (p - 1 = q 2^96).
//
// `derive`: priv, x, y (64 hex digits; x, y may be >= p) -> st 0 with out (64 hex digits) = what
//   KeyPair#derive returns, 1 with msg 'public point not validated', 2 = the product is the point at
//   infinity, with msg = what getX throws.  Cases tagged `pair` went through KeyPair#derive of the
//   reference's own key pairs, both directions; every other priv is fed to Point#mul as it stands
//   (KeyPair would reduce it mod n first), behind the same pub.validate() test.
// `derive_wire`: priv, enc (hex) -> the same with st 3 = keyFromPublic throws (msg), and err = the
//   status of ellgpu_custom_decode_points: 0, 1 'Unknown point format', 2 'invalid point',
//   3 'Assertion failed'.
// `validate`: x, y, inf -> st = KeyPair#validate's reason (0 result true, 1 'Invalid public key',
//   2 'Public key is not a point', 3 'Public key * N != O'), st0 = the same without the third test.
// `encode`: x, y -> full = encode('hex', false), compact = encode('hex', true).
// tag = what the case exercises.

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

// the domains of custom_recover.json, read back from that fixture (parameters are data)
var DOMAINS = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'tests', 'golden', 'custom_recover.json'), 'utf8'))
  .map(function(c) { return { name: c.name, p: c.p, a: c.a, b: c.b, n: c.n, g: [c.g.x, c.g.y] }; });

function build(spec) {
  var pc = new elliptic.curves.PresetCurve({ type: 'short', prime: null, p: spec.p, a: spec.a, b: spec.b,
    n: spec.n, hash: hash.sha256, gRed: false, g: spec.g });
  return new elliptic.ec(pc);
}

var TOP = new BN(1).ushln(256);
var DECODE_ERR = { 'Unknown point format': 1, 'invalid point': 2, 'Assertion failed': 3 };
var REASON = { 'Invalid public key': 1, 'Public key is not a point': 2, 'Public key * N != O': 3 };

function orderOf(P) {                          // of a point whose order divides 8
  var o = 1;
  for (var Q = P; !Q.isInfinity(); Q = Q.dbl()) o *= 2;
  return o;
}

function gen(spec) {
  var rng = new Prng('ellgpu-golden-v1:custom-ecdh:' + spec.name);
  var ec = build(spec);
  var curve = ec.curve, G = ec.g, n = ec.n, p = curve.p;
  var PL = p.byteLength();
  var o = { name: spec.name, p: hex32(p), a: hex32(curve.a.fromRed()), b: hex32(curve.b.fromRed()), n: hex32(n),
    g: { x: hex32(G.getX()), y: hex32(G.getY()) }, pl: PL, derive: [], derive_wire: [], validate: [], encode: [] };

  // the tail of KeyPair#derive for a priv that is used as it stands
  function tail(c, pub, priv) {
    if (!pub.validate()) {
      c.st = 1;
      c.msg = 'public point not validated';
      return;
    }
    var R = pub.mul(priv);
    if (R.isInfinity()) {
      c.st = 2;
      try { R.getX(); throw new Error('getX of infinity did not throw'); } catch (e) { c.msg = String(e.message).slice(0, 60); }
    } else {
      c.st = 0;
      c.out = hex32(R.getX());
    }
  }
  function derive(tag, priv, x, y) {
    var c = { tag: tag, priv: hex32(priv), x: hex32(x), y: hex32(y) };
    tail(c, curve.point(x.clone(), y.clone()), priv.clone());
    o.derive.push(c);
    return c;
  }
  function wire(tag, priv, enc) {
    var c = { tag: tag, priv: hex32(priv), enc: Buffer.from(enc).toString('hex') };
    var pub = null;
    try {
      pub = ec.keyFromPublic(Buffer.from(enc)).getPublic();
      c.err = 0;
    } catch (e) {
      if (!(e.message in DECODE_ERR)) throw e;
      c.st = 3;
      c.err = DECODE_ERR[e.message];
      c.msg = e.message;
    }
    if (pub) tail(c, pub, priv.clone());
    o.derive_wire.push(c);
    return c;
  }
  function validate(tag, x, y, inf) {
    var c = { tag: tag, x: hex32(x), y: hex32(y), inf: inf ? 1 : 0 };
    var pub = inf ? curve.point(null, null) : curve.point(x.clone(), y.clone());
    var kp = ec.keyFromPublic(G);               // (keyFromPublic cannot take the point at infinity)
    kp.pub = pub;
    var v = kp.validate();
    c.st = v.result ? 0 : REASON[v.reason];
    c.st0 = pub.isInfinity() ? 1 : (pub.validate() ? 0 : 2);
    if (c.st === undefined) throw new Error('reason ' + v.reason);
    o.validate.push(c);
    return c;
  }
  function encode(tag, x, y) {
    var P = curve.point(x.clone(), y.clone());
    o.encode.push({ tag: tag, x: hex32(x), y: hex32(y), full: P.encode('hex', false), compact: P.encode('hex', true) });
  }
  function enc(P, prefix) {                      // a SEC1 encoding with a prefix of the caller's choosing
    var xb = P.getX().toArray('be', PL), yb = P.getY().toArray('be', PL);
    return prefix === 2 || prefix === 3 ? [prefix].concat(xb) : [prefix].concat(xb, yb);
  }
  function fits(v) { return v.cmp(TOP) < 0; }

  var i, keys = [];
  for (i = 0; i < 4; i++) keys.push(ec.keyFromPrivate(rng.below(n)));
  // the reference's own key pairs, both directions
  for (i = 0; i < 4; i++) {
    var A = keys[i], B = keys[(i + 1) % 4];
    var s1 = A.derive(B.getPublic()), s2 = B.derive(A.getPublic());
    if (s1.cmp(s2) !== 0) throw new Error('ECDH asymmetry in the reference');
    var c1 = derive('pair', A.getPrivate(), B.getPublic().getX(), B.getPublic().getY());
    var c2 = derive('pair', B.getPrivate(), A.getPublic().getX(), A.getPublic().getY());
    if (c1.out !== hex32(s1) || c2.out !== hex32(s1)) throw new Error('derive tail differs from KeyPair#derive');
  }
  var Q = keys[0].getPublic(), Q2 = keys[1].getPublic(), d = keys[2].getPrivate();
  // priv as Point#mul sees it
  [['priv_1', new BN(1)], ['priv_2', new BN(2)], ['priv_n_minus_1', n.subn(1)], ['priv_n', n.clone()],
    ['priv_n_plus_1', n.addn(1)], ['priv_0', new BN(0)], ['priv_all_ones', TOP.subn(1)], ['priv_2n', n.muln(2)],
    ['priv_random_256', rng.bits(256)]].forEach(function(t) {
    if (fits(t[1])) {
      derive(t[0], t[1], Q.getX(), Q.getY());
      derive(t[0], t[1], G.getX(), G.getY());
    }
  });
  // off-curve peers
  derive('off_curve_y', d, Q.getX(), Q.getY().addn(1).umod(p));
  derive('off_curve_x', d, Q.getX().addn(1).umod(p), Q.getY());
  derive('off_curve_zero', d, new BN(0), new BN(0));
  derive('off_curve_swapped', d, Q.getY(), Q.getX());
  derive('off_curve_random', d, rng.below(p), rng.below(p));
  // a coordinate + p where it still fits 32 bytes
  if (fits(Q.getX().add(p))) derive('x_plus_p', d, Q.getX().add(p), Q.getY());
  if (fits(Q.getY().add(p))) derive('y_plus_p', d, Q.getX(), Q.getY().add(p));
  if (fits(Q.getX().add(p)) && fits(Q.getY().add(p))) derive('xy_plus_p', d, Q.getX().add(p), Q.getY().add(p));
  if (fits(Q.getX().add(p).add(p))) derive('x_plus_2p', d, Q.getX().add(p).add(p), Q.getY());
  if (fits(p)) derive('x_is_p', d, p.clone(), new BN(1));
  derive('all_ones', d, TOP.subn(1), TOP.subn(1));

  // validate: subgroup points, infinity, off-curve points
  for (i = 0; i < 4; i++) validate('subgroup', keys[i].getPublic().getX(), keys[i].getPublic().getY(), false);
  validate('generator', G.getX(), G.getY(), false);
  validate('infinity', new BN(0), new BN(0), true);
  validate('infinity_over_a_point', Q.getX(), Q.getY(), true);
  validate('infinity_over_off_curve', Q.getX(), Q.getY().addn(1).umod(p), true);
  validate('off_curve_y', Q.getX(), Q.getY().addn(1).umod(p), false);
  validate('off_curve_zero', new BN(0), new BN(0), false);
  validate('off_curve_random', rng.below(p), rng.below(p), false);
  if (fits(Q.getX().add(p))) validate('x_plus_p', Q.getX().add(p), Q.getY(), false);
  if (fits(Q.getY().add(p))) validate('y_plus_p', Q.getX(), Q.getY().add(p), false);
  validate('negated', Q.getX(), Q.neg().getY(), false);

  // points outside the subgroup (a cofactor curve only): orders 2, 4, 8 and 8 n
  var h = curve.p.div(n).toNumber() + 1;       // Hasse: the cofactor of these domains is 1 or 8
  if (h >= 8) {
    var low = {}, big = null;
    for (var x = 1; !(low[2] && low[4] && low[8] && big); x++) {
      var P;
      try { P = curve.pointFromX(new BN(x), (x & 1) === 1); } catch (e) { continue; }
      var T = P.mul(n);
      if (T.isInfinity()) continue;
      var ord = orderOf(T);
      if (ord === 8 && !big) big = P;
      for (var R = T; !R.isInfinity(); R = R.dbl()) {
        var ro = orderOf(R);
        if (!low[ro]) low[ro] = R;
      }
    }
    if (!low[2].getY().isZero()) throw new Error('the point of order 2 has y != 0');
    [2, 4, 8].forEach(function(ord) {
      var L = low[ord];
      validate('order_' + ord, L.getX(), L.getY(), false);
      derive('order_' + ord + '_times_order', new BN(ord), L.getX(), L.getY());
      derive('order_' + ord + '_times_multiple', new BN(ord * 5), L.getX(), L.getY());
      derive('order_' + ord + '_times_1', new BN(1), L.getX(), L.getY());
      derive('order_' + ord + '_times_3', new BN(3), L.getX(), L.getY());
      derive('order_' + ord + '_times_n', n.clone(), L.getX(), L.getY());
      derive('order_' + ord + '_times_random', d, L.getX(), L.getY());
      derive('order_' + ord + '_times_all_ones', TOP.subn(1), L.getX(), L.getY());
      wire('order_' + ord + '_compressed', d, enc(L, 2 + (L.getY().isOdd() ? 1 : 0)));
    });
    validate('order_8n', big.getX(), big.getY(), false);
    derive('order_8n_times_n', n.clone(), big.getX(), big.getY());
    derive('order_8n_times_8n', n.muln(8), big.getX(), big.getY());
    derive('order_8n_times_random', d, big.getX(), big.getY());
  }

  // SEC1: every prefix, the wrong ones, and the lengths
  for (i = 0; i < 2; i++) {
    var K = keys[i].getPublic(), dk = keys[3 - i].getPrivate();
    var odd = K.getY().isOdd();
    wire('compressed', dk, enc(K, odd ? 3 : 2));
    wire('compressed_other_parity', dk, enc(K, odd ? 2 : 3));
    wire('uncompressed', dk, enc(K, 4));
    wire('hybrid', dk, enc(K, odd ? 7 : 6));
    wire('hybrid_contradicting_y', dk, enc(K, odd ? 6 : 7));
    wire('prefix_00', dk, enc(K, 0));
    wire('prefix_05', dk, enc(K, 5));
    wire('prefix_08', dk, enc(K, 8));
    wire('prefix_04_on_short', dk, [4].concat(K.getX().toArray('be', PL)));
    wire('prefix_02_on_long', dk, [2].concat(K.getX().toArray('be', PL), K.getY().toArray('be', PL)));
    var bad = enc(K, 4);
    bad[bad.length - 1] ^= 1;
    wire('uncompressed_off_curve', dk, bad);
    var hy = enc(K, odd ? 6 : 7);
    hy[hy.length - 1] ^= 1;                     // the prefix now agrees with y's last bit, y is wrong
    wire('hybrid_off_curve', dk, hy);
    wire('wrong_length_short', dk, enc(K, 4).slice(0, 2 * PL));
    wire('wrong_length_long', dk, enc(K, 4).concat([0]));
    wire('wrong_length_compressed_short', dk, enc(K, 2).slice(0, PL));
    wire('wrong_length_one', dk, [4]);
    wire('priv_0', new BN(0), enc(K, 4));
    wire('priv_n', n.clone(), enc(K, odd ? 3 : 2));
    wire('priv_all_ones', TOP.subn(1), enc(K, 4));
  }
  // a compressed x without a root, and coordinates >= p where PL bytes hold them
  for (i = 0, x = 2; i < 3; x++) {
    var xb = new BN(x);
    var ok = true;
    try { curve.pointFromX(xb, false); } catch (e) { ok = false; }
    if (ok) continue;
    wire('compressed_no_root', d, [2 + (i & 1)].concat(xb.toArray('be', PL)));
    i++;
  }
  if (Q.getX().add(p).byteLength() <= PL) {
    wire('compressed_x_plus_p', d, [Q.getY().isOdd() ? 3 : 2].concat(Q.getX().add(p).toArray('be', PL)));
    if (Q.getY().add(p).byteLength() <= PL)
      wire('uncompressed_xy_plus_p', d, [4].concat(Q.getX().add(p).toArray('be', PL), Q.getY().add(p).toArray('be', PL)));
  }
  wire('compressed_all_ones', d, [2].concat(new BN(1).ushln(8 * PL).subn(1).toArray('be', PL)));
  wire('uncompressed_all_ones', d, [4].concat(new BN(1).ushln(8 * PL).subn(1).toArray('be', PL),
    new BN(1).ushln(8 * PL).subn(1).toArray('be', PL)));
  wire('uncompressed_zero', d, [4].concat(new BN(0).toArray('be', 2 * PL)));

  // encode: subgroup points, coordinates with leading zero bytes, coordinates >= p
  for (i = 0; i < 4; i++) encode('subgroup', keys[i].getPublic().getX(), keys[i].getPublic().getY());
  for (i = 0, x = 1; i < 2; x++) {
    var S = G.mul(new BN(x));
    if (S.getX().byteLength() < PL || S.getY().byteLength() < PL) {
      encode('leading_zero_byte', S.getX(), S.getY());
      i++;
    }
    if (x > 4000) break;
  }
  encode('small_coordinates', new BN(1), new BN(2));
  encode('small_coordinates_odd', new BN(0x0102), new BN(3));
  encode('zero', new BN(0), new BN(0));
  if (fits(Q.getX().add(p))) encode('x_plus_p', Q.getX().add(p), Q.getY());
  if (fits(Q.getY().add(p))) encode('y_plus_p', Q2.getX(), Q2.getY().add(p));
  encode('all_ones', TOP.subn(1), TOP.subn(1));
  encode('p_minus_1', p.subn(1), p.subn(2));
  return o;
}

var out = DOMAINS.map(gen);
var file = path.join(OUT, 'custom_ecdh.json');
fs.writeFileSync(file, JSON.stringify(out).replace(/\{"tag"/g, '\n{"tag"') + '\n');
out.forEach(function(c) {
  function hist(rows, key) {
    var h = {};
    rows.forEach(function(r) { h[r[key]] = (h[r[key]] || 0) + 1; });
    return JSON.stringify(h);
  }
  console.log(c.name + ': derive ' + c.derive.length + ' (st ' + hist(c.derive, 'st') + '), wire ' + c.derive_wire.length +
    ' (st ' + hist(c.derive_wire, 'st') + ', err ' + hist(c.derive_wire, 'err') + '), validate ' + c.validate.length +
    ' (st ' + hist(c.validate, 'st') + '), encode ' + c.encode.length);
});
console.log('wrote ' + file + ' (' + fs.statSync(file).size + ' bytes)');
