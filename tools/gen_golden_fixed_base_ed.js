'use strict';
// Golden vectors for the fixed-base tables of caller-chosen points on Edwards curves --
// ellgpu_ed_base_define, then ellgpu_mul_base and ellgpu_mul_base2 on its handles: every answer is
// the reference's own `P.precompute(); P.mul(k)`, or `B1.mulAdd(k1, B2, k2)` with both operands
// precomputed.  Runs only where the reference is present (see tools/ref_loader.js); all randomness
// is SHA-256 counter mode over a fixed seed (the PRNG of tools/gen_golden_fixed_base.js), so a rerun
// reproduces tests/golden/fixed_base_ed.json byte for byte.
//
//   node tools/gen_golden_fixed_base_ed.js [outdir]
//
// Curves (`kind`): ed25519, the preset; Curve1174 as a user-defined domain; E-222 as a plain
// user-defined id; ed25519's parameters written out by hand, as a domain.  a is a square and d is not
// on all four (checked below), so the addition law is complete and every answer is a curve point.
//
// Per curve:
//   p, a, d, n, g   the parameters, n = the order of g
//   bases    [x, y] hex: G, 2 G, -G, one point from the PRNG, the identity (0, 1), (0, p - 1) of
//            order 2, and a point (x, 0) of order 4 (every one of these curves has cofactor 4 or 8)
//   k        the scalars, 64 hex digits: 0, 1, 2, n - 1, n, n + 1, 2^256 - 1, values with leading zero
//            bytes, 2^15, 2^15 + 1, 2^16 - 1, 2^16 and their twins around bits 7/8, and 24 random ones
//   mul      per base, per scalar: the answer's digest
//   pairs    [i1, i2, k1, k2, digest] for k1 * bases[i1] + k2 * bases[i2]: random ones, k1 B1 = -k2 B2
//            (the answer is the identity), B1 = B2 with k1 = k2 = one window digit, B2 = -B1 with
//            k1 = d and k2 = d + e 2^16, k1 = 0, k2 = 0, both 0, and two with bases of small order
// A digest is the first 8 bytes of SHA-256(inf || x || y) as in fixed_base.json, with the identity
// written as inf = 1 beside (0, 1): what ellgpu_mul_base writes on ed25519 (a user-defined id gets
// inf = 0 beside the same coordinates; tests/fixed_base_ed_checks.py knows).

var fs = require('fs');
var path = require('path');
var crypto = require('crypto');
var ref = require('./ref_loader').load();
var elliptic = ref.elliptic;
var BN = ref.BN;

var OUT = process.argv[2] || path.join(__dirname, '..', 'tests', 'golden');
var B = 32;

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

var P1174 = new BN(1).ushln(251).subn(9);
var P25519 = new BN(1).ushln(255).subn(19);
var ED = elliptic.curves.ed25519.curve;
var USER = [
  { name: 'curve1174', kind: 'domain', p: P1174, a: new BN(1), d: P1174.subn(1174),
    n: new BN(1).ushln(249).sub(new BN('11332719920821432534773113288178349711', 10)),
    gx: new BN('1582619097725911541954547006453739763381091388846394833492296309729998839514', 10),
    gy: new BN('3037538013604154504764115728651437646519513534305223422754827055689195992590', 10) },
  { name: 'e222', kind: 'plain', p: new BN(1).ushln(222).subn(117), a: new BN(1), d: new BN(160102),
    n: new BN('1684996666696914987166688442938726735569737456760058294185521417407', 10),
    gx: new BN('2705691079882681090389589001251962954446177367541711474502428610129', 10), gy: new BN(28) },
  { name: 'ed25519_by_hand', kind: 'domain', p: P25519, a: P25519.subn(1), aconf: '-1', d: ED.d.fromRed(), n: ED.n.clone(),
    gx: ED.g.getX(), gy: ED.g.getY() },
];

function hex(bn) { return bn.toString(16, 2 * B); }
function digest(P) {
  var buf = Buffer.alloc(1 + 2 * B);
  if (P.isInfinity()) buf[0] = 1;
  Buffer.from(P.getX().toArray('be', B)).copy(buf, 1);
  Buffer.from(P.getY().toArray('be', B)).copy(buf, 1 + B);
  return crypto.createHash('sha256').update(buf).digest('hex').slice(0, 16);
}

function gen(name, kind, curve, G, n) {
  var rng = new Prng('ellgpu-golden-v1:fixed-base-ed:' + name);
  var p = curve.p, red = curve.red;
  var a = curve.a.fromRed(), d = curve.d.fromRed();
  var euler = function(v) { return v.toRed(red).redPow(p.subn(1).shrn(1)).fromRed().cmpn(1) === 0; };
  if (!euler(a) || euler(d)) throw new Error(name + ': the addition law is not complete');
  var o = { name: name, kind: kind, B: B, p: hex(p), a: hex(a), d: hex(d), n: hex(n), g: [hex(G.getX()), hex(G.getY())] };
  if (!G.mul(n).isInfinity()) throw new Error(name + ': n G is not the identity');
  var H = G.mul(rng.bits(248).umod(n.subn(2)).addn(2));
  // order 4: a x^2 = 1 at y = 0
  var x4 = a.toRed(red).redInvm().redSqrt().fromRed();
  var T4 = curve.point(x4, new BN(0));
  var T2 = curve.point(new BN(0), p.subn(1));
  var ID = curve.point(new BN(0), new BN(1));
  if (!curve.validate(T4) || T4.dbl().isInfinity() || !T4.dbl().dbl().isInfinity()) throw new Error(name + ': T4 is not of order 4');
  if (!curve.validate(T2) || T2.isInfinity() || !T2.dbl().isInfinity()) throw new Error(name + ': T2 is not of order 2');
  var pts = [G, G.dbl(), G.neg(), H, ID, T2, T4].map(function(P) { return curve.point(P.getX(), P.getY()); });
  o.bases = pts.map(function(P) { return [hex(P.getX()), hex(P.getY())]; });
  var TOP = new BN(1).ushln(8 * B);
  var ks = [new BN(0), new BN(1), new BN(2), n.subn(1), n, n.addn(1), TOP.subn(1)];
  [8, 64, 128].forEach(function(b) { ks.push(rng.bits(b).setn(b - 1, 1)); });
  [[15, 16], [7, 8]].forEach(function(lh) {
    var lo = new BN(1).ushln(lh[0]), hi = new BN(1).ushln(lh[1]);
    ks.push(lo, lo.addn(1), hi.subn(1), hi);
  });
  for (var i = 0; i < 24; i++) ks.push(rng.bits(8 * B));
  o.k = ks.map(hex);
  pts.forEach(function(P) { P.precompute(8 * B + 1); });
  o.mul = pts.map(function(P) { return ks.map(function(k) { return digest(P.mul(k.clone())); }); });
  var pairs = [];
  function pair(i1, i2, k1, k2) {
    pairs.push([i1, i2, hex(k1), hex(k2), digest(pts[i1].mulAdd(k1.clone(), pts[i2], k2.clone()))]);
  }
  for (i = 0; i < 4; i++) pair(i & 1 ? 3 : 0, i & 1 ? 1 : 3, rng.bits(8 * B), rng.bits(8 * B));
  var t = rng.bits(64).umod(n.subn(1)).addn(1);
  pair(0, 1, t.muln(2), n.sub(t));                     // 2t G + (n - t) 2G = the identity
  [5, 200].forEach(function(dg) { pair(0, 0, new BN(dg), new BN(dg)); });
  [[7, 3], [255, 1], [1, 40000]].forEach(function(de) {
    pair(0, 2, new BN(de[0]), new BN(de[0]).add(new BN(de[1]).ushln(16)));
  });
  pair(0, 3, new BN(0), rng.bits(8 * B));
  pair(0, 3, rng.bits(8 * B), new BN(0));
  pair(0, 3, new BN(0), new BN(0));
  pair(4, 6, rng.bits(8 * B), rng.bits(8 * B));
  pair(5, 3, rng.bits(8 * B), rng.bits(8 * B));
  o.pairs = pairs;
  if (pairs[4][4] !== digest(ID)) throw new Error(name + ': the cancelling pair is not the identity');
  return o;
}

var out = [gen('ed25519', 'preset', ED, ED.g, ED.n)];
USER.forEach(function(s) {
  var c = new elliptic.curve.edwards({ p: s.p.toString(16), a: s.aconf || s.a.toString(16), c: '1', d: s.d.toString(16),
    n: s.n.toString(16), g: [s.gx.toString(16), s.gy.toString(16)] });
  out.push(gen(s.name, s.kind, c, c.g, c.n));
});

var file = path.join(OUT, 'fixed_base_ed.json');
fs.writeFileSync(file, JSON.stringify(out).replace(/("name"|"bases"|"k"|"mul"|"pairs"):/g, '\n$1:').replace(/\],\[/g, '],\n[') + '\n');
out.forEach(function(c) { console.log(c.name + ': ' + c.k.length + ' scalars x ' + c.bases.length + ' bases, ' + c.pairs.length + ' pairs'); });
console.log('wrote ' + file + ' (' + fs.statSync(file).size + ' bytes)');
