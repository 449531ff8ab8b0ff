'use strict';
// Golden vectors for sums of many k * P terms -- ellgpu_mul_sum: every answer is the reference's own
// `points.map(mul).reduce(add)`, the terms multiplied one by one with Point#mul and added in order
// with Point#add.  The generator asserts that it equals curve._wnafMulAdd(1, points, coeffs, m)
// wherever m is even (an odd len throws there) and, on secp256k1, curve._endoWnafMulAdd(points,
// coeffs) for every m.  Runs only where the reference is present (see tools/ref_loader.js); all
// randomness is SHA-256 counter mode over a fixed seed, so a rerun reproduces
// tests/golden/mul_sum.json byte for byte.
//
//   node tools/gen_golden_mul_sum.js [outdir]
//
// Curves: the six presets; brainpoolP256r1 as a user-defined domain; secp192k1 as a plain
// user-defined id.
//
// Per curve:
//   B        bytes per coordinate and scalar at the C ABI (32 on user-defined ids)
//   p, a, b, n, g   the parameters (user-defined curves); n on every curve
//   pts      [x, y] hex of 2 B digits each: the pool the terms draw their points from -- multiples
//            of G from the PRNG, each followed by its negative; then the same points with p added to
//            a coordinate where 2^(8B) > p leaves room; last, points that are NOT on the curve
//            (y + 1), used by the `off` rows only
//   rows     [tag, [[k, point index], ...], digest]: one sum each
//            m<M>         M random terms, M in 1, 2, 3, 4, 5, 7, 8, 16, 33
//            edge<i>      the scalars 0, 1, n - 1, n, n + 1, 2^(8B) - 1: scalar i in both slots of a
//                         pair and in the lone last term of three
//            zeros        every scalar 0: O
//            twice_pair   the same (k, P) in both slots of one pair (the ladder's doubling branch)
//            twice_fold   the same two pairs twice: the partial sums are equal (the fold's doubling branch)
//            cancel_pair  (k, P) and (k, -P) in one pair, then more terms
//            cancel_fold  two pairs that cancel each other, then more pairs: O in the middle of the
//                         fold, which goes on adding
//            total_o      a sum of seven terms that is O in total
//            wide         terms whose coordinates are >= p (where the pool has such points)
//   off      [tag, [[k, point index], ...]]: sums with one term that is not on the curve -- first,
//            last, and as the lone last term of an odd m; inputs only, the expected answer is the
//            engine's status 2
// A digest is the first 8 bytes of SHA-256(inf || x || y), inf one byte (1 at infinity, x and y zero
// then), x and y of B bytes each: what ellgpu_mul_sum writes for the sum.  The Python-integer model
// of tests/mul_sum_checks.py is pinned to these digests and gives the coordinates themselves.

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
var MS = [1, 2, 3, 4, 5, 7, 8, 16, 33];
var NPTS = 12;          // points from the PRNG; the pool holds each and its negative

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
  var rng = new Prng('ellgpu-golden-v1:mul-sum:' + name);
  var hex = function(bn) { return bn.toString(16, 2 * B); };
  var o = { name: name, B: B };
  Object.keys(extra || {}).forEach(function(f) { o[f] = extra[f]; });
  o.n = n.toString(16);
  var TOP = new BN(1).ushln(8 * B);
  var p = curve.p;
  // the pool: coords[i] = [x, y] as written to the fixture, pts[i] = the reference's point (null off the curve)
  var coords = [], pts = [];
  for (var i = 0; i < NPTS; i++) {
    var P = G.mul(rng.bits(8 * B - 8).umod(n.subn(2)).addn(2));
    [P, P.neg()].forEach(function(Q) {
      coords.push([Q.getX(), Q.getY()]);
      pts.push(curve.point(Q.getX(), Q.getY()));
    });
  }
  var wide = [];
  for (i = 0; i < 2 * NPTS && wide.length < 4; i++) {
    var x = coords[i][0], y = coords[i][1];
    var fx = x.add(p).cmp(TOP) < 0, fy = y.add(p).cmp(TOP) < 0;
    if (!fx && !fy) continue;
    var c = [fx ? x.add(p) : x, fy && (wide.length & 1 || !fx) ? y.add(p) : y];
    var Q = curve.point(c[0], c[1]);                  // reduces, as the engine does
    if (!Q.eq(pts[i])) throw new Error(name + ': the reference does not reduce a wide coordinate');
    wide.push(coords.length);
    coords.push(c);
    pts.push(Q);
  }
  var offs = [];
  for (i = 0; i < 3; i++) {
    var yy = coords[i][1].addn(1).umod(p);
    if (curve.validate(curve.point(coords[i][0], yy))) throw new Error(name + ': y + 1 is on the curve');
    offs.push(coords.length);
    coords.push([coords[i][0], yy]);
    pts.push(null);
  }
  o.pts = coords.map(function(c) { return [hex(c[0]), hex(c[1])]; });

  var rows = [];
  function answer(terms) {
    var ps = terms.map(function(t) { return pts[t[1]]; });
    var ks = terms.map(function(t) { return t[0].clone(); });
    var want = ps.map(function(P, j) { return P.mul(ks[j].clone()); }).reduce(function(a, b) { return a.add(b); });
    if (terms.length % 2 === 0) {
      var w = curve._wnafMulAdd(1, ps, ks.map(function(k) { return k.clone(); }), terms.length);
      if (!w.eq(want)) throw new Error(name + ': _wnafMulAdd differs from the sum of the products');
    }
    if (curve.endo) {
      var e = curve._endoWnafMulAdd(ps, ks.map(function(k) { return k.clone(); }));
      if (!e.eq(want)) throw new Error(name + ': _endoWnafMulAdd differs from the sum of the products');
    }
    return want;
  }
  function row(tag, terms) {
    var want = answer(terms);
    rows.push([tag, terms.map(function(t) { return [hex(t[0]), t[1]]; }), digest(want, B)]);
    return want;
  }
  function rk() { return rng.bits(8 * B); }
  function rp() { return rng.bytes(1)[0] % (2 * NPTS); }
  function rt() { return [rk(), rp()]; }
  function many(m) { var t = []; for (var j = 0; j < m; j++) t.push(rt()); return t; }

  MS.forEach(function(m) { row('m' + m, many(m)); });
  [new BN(0), new BN(1), n.subn(1), n, n.addn(1), TOP.subn(1)].forEach(function(k, j) {
    row('edge' + j, [[k, rp()], [k, rp()], [k, rp()]]);
  });
  var O = curve.point(null, null);
  var z = row('zeros', [[new BN(0), 0], [new BN(0), 3], [new BN(0), 5], [new BN(0), 8], [new BN(0), 2]]);
  if (!z.isInfinity()) throw new Error(name + ': zeros is not O');
  var t1 = rt(), t2 = rt(), t3 = rt();
  row('twice_pair', [t1, t1, t2]);
  row('twice_fold', [t1, t2, t1, t2]);
  row('twice_fold8', [t1, t2, t3, t3, t1, t2, t3, t3]);
  var neg = function(t) { return [t[0], t[1] ^ 1]; };     // the pool holds P at 2 i and -P at 2 i + 1
  row('cancel_pair', [t1, neg(t1), t2, t3]);
  row('cancel_pair_alone', [t2, neg(t2)]);
  row('cancel_fold', [t1, t2, neg(t1), neg(t2), t3, rt(), rt()]);
  row('cancel_fold8', [t1, t2, t3, t1, neg(t1), neg(t2), neg(t3), neg(t1), rt()]);
  // O in total: six random terms and the negative of their sum as 1 * (-S), S taken into the pool
  var six = many(6);
  var S = answer(six);
  coords.push([S.getX(), S.neg().getY()]);
  pts.push(S.neg());
  o.pts.push([hex(S.getX()), hex(S.neg().getY())]);
  var tot = row('total_o', six.concat([[new BN(1), pts.length - 1]]));
  if (!tot.isInfinity()) throw new Error(name + ': total_o is not O');
  if (wide.length) {
    row('wide', wide.map(function(w) { return [rk(), w]; }).concat([rt()]));
    row('wide_pair', [[rk(), wide[0]], [rk(), wide[wide.length - 1]]]);
  }
  o.rows = rows;

  var off = [];
  function offrow(tag, terms) { off.push([tag, terms.map(function(t) { return [hex(t[0]), t[1]]; })]); }
  offrow('first', [[rk(), offs[0]]].concat(many(4)));
  offrow('last', many(3).concat([[rk(), offs[1]]]));
  offrow('lone', many(4).concat([[rk(), offs[2]]]));
  offrow('middle', many(8).concat([[rk(), offs[0]]], many(8)));
  offrow('only', [[rk(), offs[1]]]);
  offrow('zero_scalar', [rt(), [new BN(0), offs[2]]]);
  o.off = off;
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

var file = path.join(OUT, 'mul_sum.json');
fs.writeFileSync(file, JSON.stringify(out).replace(/("name"|"pts"|"rows"|"off"):/g, '\n$1:').replace(/\]\],\["/g, ']],\n["') + '\n');
out.forEach(function(c) {
  var terms = c.rows.reduce(function(a, r) { return a + r[1].length; }, 0);
  console.log(c.name + ': ' + c.pts.length + ' points, ' + c.rows.length + ' sums of ' + terms + ' terms, ' + c.off.length + ' off-curve sums');
});
console.log('wrote ' + file + ' (' + fs.statSync(file).size + ' bytes)');
