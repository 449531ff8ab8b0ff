'use strict';
// Golden vectors for the fixed-base tables of caller-chosen points -- ellgpu_base_define,
// ellgpu_mul_base, ellgpu_mul_base2: every answer is the reference's own `P.precompute(); P.mul(k)`,
// or `B1.mulAdd(k1, B2, k2)` with both operands precomputed.  Runs only where the reference is
// present (see tools/ref_loader.js); all randomness is SHA-256 counter mode over a fixed seed, so a
// rerun reproduces tests/golden/fixed_base.json byte for byte.
//
//   node tools/gen_golden_fixed_base.js [outdir]
//
// Curves: the six presets; brainpoolP256r1 as a user-defined domain; secp192k1 as a plain
// user-defined id (its G is one more base given by coordinates); `cof_p10007`, a curve of order 2 q
// over p = 10007 found by search here, whose point of order 2 is a base the engine must refuse (2 T
// = O sits inside the table) and whose points of order q are bases it must accept.
//
// Per curve:
//   B        bytes per coordinate and scalar at the C ABI (32 on user-defined ids)
//   p, a, b, n, g   the parameters (user-defined curves), n = the order of the bases
//   bases    [x, y] hex: G by coordinates, 2 G, -G, one point from the PRNG
//   refused  (cof_p10007) [x, y] of the bases whose table would hold the point at infinity
//   k        the scalars, hex of B bytes: 0, 1, 2, n - 1, n, n + 1, 2^(8B) - 1 (all-ones: the signed
//            recoding's carry runs through every window and into the extra one), values with leading
//            zero bytes, 2^15, 2^15 + 1, 2^16 - 1, 2^16 and the same around bits 3/4, 7/8, 11/12, 21/22,
//            and 24 random ones
//   mul      per base, per scalar: the answer's digest
//   pairs    [i1, i2, k1, k2, digest] for k1 * bases[i1] + k2 * bases[i2]: random ones, k1 B1 = -k2 B2
//            (the answer is O), B1 = B2 with k1 = k2 = one window digit (the doubling branch of the
//            addition), B2 = -B1 with k1 = d and k2 = d + e 2^16 (the accumulator is O in the middle
//            of the second walk and additions start again from it), k1 = 0, k2 = 0, both 0
// A digest is the first 8 bytes of SHA-256(inf || x || y), inf one byte (1 at infinity, x and y zero
// then), x and y of B bytes each: what ellgpu_mul_base writes for the item.  Full coordinates of
// ~2 300 answers up to 132 bytes each would be four times the size allowed for this file; the
// Python-integer model of tests/fixed_base_checks.py is pinned to these digests and gives the
// coordinates themselves.

var fs = require('fs');
var path = require('path');
var crypto = require('crypto');
var ref = require('./ref_loader').load();
var elliptic = ref.elliptic;
var BN = ref.BN;

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

// ---- the cofactor curve: y^2 = x^3 + x + b over 10007 with order 2 q, by search in plain numbers
function powmod(a, e, p) { var r = 1; a %= p; while (e) { if (e & 1) r = r * a % p; a = a * a % p; e >>= 1; } return r; }
function isPrime(v) { if (v < 2) return false; for (var d = 2; d * d <= v; d++) if (v % d === 0) return false; return true; }
function findCofactorCurve() {
  var p = 10007;
  for (var b = 1; b < p; b++) {
    if ((4 + 27 * b * b) % p === 0) continue;
    var N = 1, root = -1;
    for (var x = 0; x < p; x++) {
      var rhs = ((x * x % p) * x + x + b) % p;
      if (rhs === 0) { N += 1; if (root < 0) root = x; } else if (powmod(rhs, (p - 1) / 2, p) === 1) N += 2;
    }
    if (root >= 0 && N % 2 === 0 && N % 4 !== 0 && isPrime(N / 2) && N / 2 > 255) return { p: p, b: b, q: N / 2, root: root };
  }
  throw new Error('no cofactor curve found');
}

var PRESETS = [['secp256k1', 32], ['p192', 24], ['p224', 28], ['p256', 32], ['p384', 48], ['p521', 66]];
var USER = [
  { name: 'brainpoolP256r1', domain: true,
    p: 'a9fb57dba1eea9bc3e660a909d838d726e3bf623d52620282013481d1f6e5377',
    a: '7d5a0975fc2c3057eef67530417affe7fb8055c126dc5c6ce94a4b44f330b5d9',
    b: '26dc5c6ce94a4b44f330b5d9bbd77cbf958416295cf7e1ce6bccdc18ff8c07b6',
    g: ['8bd2aeb9cb7e57cb2c4b482ffc81b7afb9de27e1e3bd23c23a4453bd9ace3262',
      '547ef835c3dac4fd97f8461a14611dc9c27745132ded8e545c1d54c72f046997'],
    n: 'a9fb57dba1eea9bc3e660a909d838d718c397aa3b561a6f7901e0e82974856a7' },
  { name: 'secp192k1', domain: false, p: 'fffffffffffffffffffffffffffffffffffffffeffffee37', a: '0', b: '3',
    g: ['db4ff10ec057e9ae26b07d0280b7f4341da5d1b1eae06c7d', '9b2f2f6d9c5628a7844163d015be86344082aa88d95e2f9d'],
    n: 'fffffffffffffffffffffffe26f2fc170f69466a74defd8d' },
];

function digest(P, B) {
  var inf = P.isInfinity();
  var buf = Buffer.alloc(1 + 2 * B);
  if (inf) buf[0] = 1;
  else {
    Buffer.from(P.getX().toArray('be', B)).copy(buf, 1);
    Buffer.from(P.getY().toArray('be', B)).copy(buf, 1 + B);
  }
  return crypto.createHash('sha256').update(buf).digest('hex').slice(0, 16);
}

function gen(name, B, curve, G, n, extra) {
  var rng = new Prng('ellgpu-golden-v1:fixed-base:' + name);
  var hex = function(bn) { return bn.toString(16, 2 * B); };
  var o = { name: name, B: B };
  Object.keys(extra || {}).forEach(function(f) { o[f] = extra[f]; });
  o.n = n.toString(16);
  // a point from the PRNG: a multiple of G (so that it has G's order on the cofactor curve too)
  var H = G.mul(rng.bits(8 * B - 8).umod(n.subn(2)).addn(2));
  var pts = [G, G.dbl(), G.neg(), H].map(function(P) { return curve.point(P.getX(), P.getY()); });
  o.bases = pts.map(function(P) { return [hex(P.getX()), hex(P.getY())]; });
  var TOP = new BN(1).ushln(8 * B);
  var ks = [new BN(0), new BN(1), new BN(2), n.subn(1), n, n.addn(1), TOP.subn(1)];
  [8, 64, 4 * B].forEach(function(b) { ks.push(rng.bits(b).setn(b - 1, 1)); });
  [[15, 16], [3, 4], [7, 8], [11, 12], [21, 22]].forEach(function(lh) {
    var lo = new BN(1).ushln(lh[0]), hi = new BN(1).ushln(lh[1]);
    ks.push(lo, lo.addn(1), hi.subn(1), hi);
  });
  for (var i = 0; i < 24; i++) ks.push(rng.bits(8 * B));
  o.k = ks.map(hex);
  pts.forEach(function(P) { P.precompute(8 * B + 1); });
  o.mul = pts.map(function(P) { return ks.map(function(k) { return digest(P.mul(k.clone()), B); }); });
  var pairs = [];
  function pair(i1, i2, k1, k2) {
    pairs.push([i1, i2, hex(k1), hex(k2), digest(pts[i1].mulAdd(k1.clone(), pts[i2], k2.clone()), B)]);
  }
  for (i = 0; i < 4; i++) pair(i & 1 ? 3 : 0, i & 1 ? 1 : 3, rng.bits(8 * B), rng.bits(8 * B));
  var t = rng.bits(64).umod(n.subn(1)).addn(1);
  pair(0, 1, t.muln(2), n.sub(t));                     // 2t G + (n - t) 2G = O
  [5, 200].forEach(function(d) { pair(0, 0, new BN(d), new BN(d)); });          // the doubling branch
  [[7, 3], [255, 1], [1, 40000]].forEach(function(de) {                         // O in the middle of the second walk
    pair(0, 2, new BN(de[0]), new BN(de[0]).add(new BN(de[1]).ushln(16)));
  });
  pair(0, 3, new BN(0), rng.bits(8 * B));
  pair(0, 3, rng.bits(8 * B), new BN(0));
  pair(0, 3, new BN(0), new BN(0));
  o.pairs = pairs;
  if (pairs[4][4] !== digest(curve.point(null, null), B)) throw new Error(name + ': the cancelling pair is not O');
  return o;
}

var out = [];
PRESETS.forEach(function(nb) {
  var c = new elliptic.ec(nb[0]).curve;
  out.push(gen(nb[0], nb[1], c, c.g, c.n));
});
USER.forEach(function(s) {
  var c = new elliptic.curve.short({ p: s.p, a: s.a, b: s.b, n: s.n, g: s.g });
  out.push(gen(s.name, 32, c, c.g, c.n, { domain: s.domain, p: s.p, a: s.a, b: s.b, g: s.g }));
});
(function() {
  var f = findCofactorCurve();
  var c = new elliptic.curve.short({ p: f.p.toString(16), a: '1', b: f.b.toString(16) });
  var rng = new Prng('ellgpu-golden-v1:fixed-base:cof_p10007:G');
  var G = null;
  while (!G || G.isInfinity()) {
    try { G = c.pointFromX(rng.bits(16).umod(new BN(f.p)), false).dbl(); } catch (e) { G = null; }
  }
  var q = new BN(f.q);
  if (!G.mul(q).isInfinity()) throw new Error('G is not of order q');
  var T = c.point(new BN(f.root), new BN(0));
  if (!c.validate(T) || !T.dbl().isInfinity()) throw new Error('T is not of order 2');
  var o = gen('cof_p10007', 32, c, G, q, { domain: false, p: f.p.toString(16), a: '1', b: f.b.toString(16), order: (2 * f.q).toString(16) });
  o.refused = [[T.getX().toString(16, 64), T.getY().toString(16, 64)]];
  var TG = T.add(G);                                  // order 2 q: no entry d 2^(8w) (T + G) with d < 256 < q is O
  o.accepted_2q = [TG.getX().toString(16, 64), TG.getY().toString(16, 64)];
  out.push(o);
})();

var file = path.join(OUT, 'fixed_base.json');
fs.writeFileSync(file, JSON.stringify(out).replace(/("name"|"bases"|"k"|"mul"|"pairs"|"refused"):/g, '\n$1:').replace(/\],\[/g, '],\n[') + '\n');
out.forEach(function(c) { console.log(c.name + ': ' + c.k.length + ' scalars x ' + c.bases.length + ' bases, ' + c.pairs.length + ' pairs'); });
console.log('wrote ' + file + ' (' + fs.statSync(file).size + ' bytes)');
