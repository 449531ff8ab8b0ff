'use strict';
// Golden vectors for sums of many k * P terms on Edwards curves -- ellgpu_ed_mul_sum: every answer is
// the reference's own `points.map(mul).reduce(add)`, the terms multiplied one by one with Point#mul
// and added in order with Point#add.  The generator asserts that it equals
// curve._wnafMulAdd(1, points, coeffs, m) wherever m is even (an odd len throws there; the points
// precomputed, see `precomputed` below).  Runs only where the reference is present (see
// tools/ref_loader.js); all randomness is SHA-256 counter mode over a fixed seed, so a rerun
// reproduces tests/golden/ed_mul_sum.json byte for byte.
//
//   node tools/gen_golden_ed_mul_sum.js [outdir]
//
// Curves (`kind`), those of tests/golden/fixed_base_ed.json: ed25519, the preset; Curve1174 as a
// user-defined domain; E-222 as a plain user-defined id; ed25519's parameters written out by hand, as
// a domain.  a is a square and d is not on all four (checked below): the addition law is complete.
//
// Per curve:
//   p, a, d, n, g   the parameters, n = the order of g
//   pts      [x, y] hex of 64 digits each: the pool the terms draw their points from -- multiples of
//            G from the PRNG, each followed by its negative (-x, y); the identity (0, 1); (0, p - 1) of
//            order 2; on ed25519 and ed25519_by_hand a point of order 8; the first points again with p
//            added to a coordinate (every one of these primes leaves room in 32 bytes); last, points
//            that are NOT on the curve (x, y + 1), used by the `off` rows only
//   rows     [tag, [[k, point index], ...], digest]: one sum each
//            m<M>           M random terms, M in 1, 2, 3, 4, 5, 7, 8, 16, 33
//            edge<i>        the scalars 0, 1, n - 1, n, n + 1, 2^256 - 1: scalar i in both slots of a
//                           pair and in the lone last term of three
//            zeros          every scalar 0: the identity
//            twice_pair     the same (k, P) in both slots of one pair
//            twice_fold     the same two pairs twice: the partial sums are equal
//            cancel_pair    (k, P) and (k, -P) in one pair, then more terms
//            cancel_fold    two pairs that cancel each other, then more pairs: the identity in the
//                           middle of the fold, which goes on adding
//            total_id       a sum of seven terms that is the identity in total
//            identity_term  (0, 1) as the point of a term, with a random scalar, among others
//            torsion        (ed25519, ed25519_by_hand) terms on the point of order 8 with scalars
//                           = 1 .. 7 mod 8, and on (0, p - 1), among others
//            wide           terms whose coordinates are >= p
//   off      [tag, [[k, point index], ...]]: sums with exactly one term that is not on the curve --
//            first, last, and as the lone last term of an odd m; inputs only, the expected answer is
//            the engine's status 2
// A digest is the first 8 bytes of SHA-256(inf || x || y) of what ellgpu_ed_mul_sum WRITES for the
// sum: x and y of 32 bytes each, (0, 1) at the identity, and inf one byte that is 1 at the identity on
// ed25519 (EdWork::normalize mirrors Point#isInfinity) and 0 everywhere on a user-defined id
// (EdcWork::normalize writes no flag) -- so the identity's digest differs between the preset and the
// other three curves.  The Python-integer model of tests/ed_mul_sum_checks.py is pinned to these
// digests and gives the coordinates themselves.

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
var MS = [1, 2, 3, 4, 5, 7, 8, 16, 33];
var NPTS = 12;          // points from the PRNG; the pool holds each and its negative

function hex(bn) { return bn.toString(16, 2 * B); }

function gen(name, kind, curve, G, n) {
  var rng = new Prng('ellgpu-golden-v1:ed-mul-sum:' + name);
  var p = curve.p, red = curve.red;
  var a = curve.a.fromRed(), d = curve.d.fromRed();
  var euler = function(v) { return v.toRed(red).redPow(p.subn(1).shrn(1)).fromRed().cmpn(1) === 0; };
  if (!euler(a) || euler(d)) throw new Error(name + ': the addition law is not complete');
  if (!G.mul(n).isInfinity()) throw new Error(name + ': n G is not the identity');
  var o = { name: name, kind: kind, B: B, p: hex(p), a: hex(a), d: hex(d), n: hex(n), g: [hex(G.getX()), hex(G.getY())] };
  var TOP = new BN(1).ushln(8 * B);
  // what the call writes: inf = 1 only on the preset, beside (0, 1)
  function digest(P) {
    var buf = Buffer.alloc(1 + 2 * B);
    if (kind === 'preset' && P.isInfinity()) buf[0] = 1;
    Buffer.from(P.getX().toArray('be', B)).copy(buf, 1);
    Buffer.from(P.getY().toArray('be', B)).copy(buf, 1 + B);
    return crypto.createHash('sha256').update(buf).digest('hex').slice(0, 16);
  }
  // the pool: coords[i] = [x, y] as written to the fixture, pts[i] = the reference's point (null off the curve)
  var coords = [], pts = [];
  function take(x, y) {
    var Q = curve.point(x, y);
    if (!curve.validate(Q)) throw new Error(name + ': a pool point is not on the curve');
    coords.push([x, y]);
    pts.push(Q);
    return coords.length - 1;
  }
  for (var i = 0; i < NPTS; i++) {
    var P = G.mul(rng.bits(8 * B - 8).umod(n.subn(2)).addn(2));
    take(P.getX(), P.getY());
    take(P.neg().getX(), P.neg().getY());             // (-x, y)
    if (!pts[2 * i].add(pts[2 * i + 1]).isInfinity()) throw new Error(name + ': P + (-P) is not the identity');
  }
  var ID = take(new BN(0), new BN(1));
  var T2 = take(new BN(0), p.subn(1));
  if (pts[T2].isInfinity() || !pts[T2].dbl().isInfinity()) throw new Error(name + ': (0, -1) is not of order 2');
  var T8 = -1;
  if (p.cmp(P25519) === 0) {
    // a point of order 8: n times a point from the PRNG, until the torsion part has full order
    for (;;) {
      var Q;
      try { Q = curve.pointFromY(rng.bits(254), rng.bytes(1)[0] & 1); } catch (e) { continue; }
      Q = Q.mul(n);
      if (Q.mul(new BN(4)).isInfinity()) continue;
      if (!Q.mul(new BN(8)).isInfinity()) throw new Error(name + ': the cofactor is not 8');
      T8 = take(Q.getX(), Q.getY());
      break;
    }
  }
  var wide = [];
  for (i = 0; i < 4; i++) {
    var x = coords[i][0], y = coords[i][1];
    var c = [i & 1 ? x : x.add(p), i & 2 || i & 1 ? y.add(p) : y];
    if (c[0].cmp(TOP) >= 0 || c[1].cmp(TOP) >= 0) throw new Error(name + ': no room above p');
    var W = curve.point(c[0], c[1]);                 // reduces, as the engine does
    if (!W.eq(pts[i])) throw new Error(name + ': the reference does not reduce a wide coordinate');
    wide.push(coords.length);
    coords.push(c);
    pts.push(W);
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
  // _wnafMulAdd takes precomputed copies of the points: on plain ones its two-point comb calls
  // Point#toJ, which the reference's Edwards points do not have (the same is why
  // tools/gen_golden_fixed_base_ed.js precomputes both operands of mulAdd)
  var pre = {};
  function precomputed(i) {
    if (!pre[i]) {
      pre[i] = curve.point(pts[i].getX(), pts[i].getY());
      pre[i].precompute(8 * B + 1);
    }
    return pre[i];
  }
  function answer(terms) {
    var ps = terms.map(function(t) { return pts[t[1]]; });
    var ks = terms.map(function(t) { return t[0].clone(); });
    var want = ps.map(function(P, j) { return P.mul(ks[j].clone()); }).reduce(function(a, b) { return a.add(b); });
    if (terms.length % 2 === 0) {
      var w = curve._wnafMulAdd(1, terms.map(function(t) { return precomputed(t[1]); }),
        ks.map(function(k) { return k.clone(); }), terms.length);
      if (!w.eq(want)) throw new Error(name + ': _wnafMulAdd differs from the sum of the products');
    }
    return want;
  }
  function row(tag, terms) {
    var want = answer(terms);
    rows.push([tag, terms.map(function(t) { return [hex(t[0]), t[1]]; }), digest(want)]);
    return want;
  }
  function rk() { return rng.bits(8 * B); }
  function rp() { return rng.bytes(1)[0] % (2 * NPTS); }
  function rt() { return [rk(), rp()]; }
  function many(m) { var t = []; for (var j = 0; j < m; j++) t.push(rt()); return t; }
  function isId(tag, P) { if (!P.isInfinity()) throw new Error(name + ': ' + tag + ' is not the identity'); }

  MS.forEach(function(m) { row('m' + m, many(m)); });
  [new BN(0), new BN(1), n.subn(1), n, n.addn(1), TOP.subn(1)].forEach(function(k, j) {
    row('edge' + j, [[k, rp()], [k, rp()], [k, rp()]]);
  });
  isId('zeros', row('zeros', [[new BN(0), 0], [new BN(0), 3], [new BN(0), 5], [new BN(0), 8], [new BN(0), 2]]));
  var t1 = rt(), t2 = rt(), t3 = rt();
  row('twice_pair', [t1, t1, t2]);
  row('twice_fold', [t1, t2, t1, t2]);
  row('twice_fold8', [t1, t2, t3, t3, t1, t2, t3, t3]);
  var neg = function(t) { return [t[0], t[1] ^ 1]; };     // the pool holds P at 2 i and -P at 2 i + 1
  row('cancel_pair', [t1, neg(t1), t2, t3]);
  isId('cancel_pair_alone', row('cancel_pair_alone', [t2, neg(t2)]));
  row('cancel_fold', [t1, t2, neg(t1), neg(t2), t3, rt(), rt()]);
  row('cancel_fold8', [t1, t2, t3, t1, neg(t1), neg(t2), neg(t3), neg(t1), rt()]);
  // the identity in total: six random terms and the negative of their sum as 1 * (-S), S taken into the pool
  var six = many(6);
  var S = answer(six).neg();
  coords.push([S.getX(), S.getY()]);
  pts.push(curve.point(S.getX(), S.getY()));
  o.pts.push([hex(S.getX()), hex(S.getY())]);
  isId('total_id', row('total_id', six.concat([[new BN(1), pts.length - 1]])));
  row('identity_term', [rt(), [rk(), ID], rt()]);
  row('identity_pair', [[rk(), ID], [rk(), ID]]);
  if (T8 >= 0) {
    var tor = [];
    for (i = 1; i <= 7; i++) tor.push([rk().iushrn(3).iushln(3).iaddn(i), T8]);
    tor.push([rk().iushrn(3).iushln(3).iaddn(3), T2], rt(), [rk().iushrn(3).iushln(3).iaddn(6), T2]);
    row('torsion', tor);
    row('torsion_only', [[new BN(5), T8], [new BN(3), T8], [new BN(1), T2]]);
  }
  row('wide', wide.map(function(w) { return [rk(), w]; }).concat([rt()]));
  row('wide_pair', [[rk(), wide[0]], [rk(), wide[wide.length - 1]]]);
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

var out = [gen('ed25519', 'preset', ED, ED.g, ED.n)];
USER.forEach(function(s) {
  var c = new elliptic.curve.edwards({ p: s.p.toString(16), a: s.aconf || s.a.toString(16), c: '1', d: s.d.toString(16),
    n: s.n.toString(16), g: [s.gx.toString(16), s.gy.toString(16)] });
  out.push(gen(s.name, s.kind, c, c.g, c.n));
});

var file = path.join(OUT, 'ed_mul_sum.json');
fs.writeFileSync(file, JSON.stringify(out).replace(/("name"|"pts"|"rows"|"off"):/g, '\n$1:').replace(/\]\],\["/g, ']],\n["') + '\n');
out.forEach(function(c) {
  var terms = c.rows.reduce(function(a, r) { return a + r[1].length; }, 0);
  console.log(c.name + ': ' + c.pts.length + ' points, ' + c.rows.length + ' sums of ' + terms + ' terms, ' + c.off.length + ' off-curve sums');
});
console.log('wrote ' + file + ' (' + fs.statSync(file).size + ' bytes)');
