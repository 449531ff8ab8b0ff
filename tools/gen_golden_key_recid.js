'use strict';
// Golden vectors for EC#getKeyRecoveryParam on the six short presets (ellgpu_ecdsa_recid): every
// recorded answer is the reference's own -- the id it returns, or that it throws.  Runs only where
// the reference is present (see tools/ref_loader.js); all randomness is SHA-256 counter mode over a
// fixed seed, so a rerun reproduces tests/golden/key_recid.json byte for byte.
//
//   node tools/gen_golden_key_recid.js [outdir]
//
// Per curve: name, B (bytes of a coordinate and of a scalar), p, n (hex) and rows
//   [tag, h, r, s, x, y, want]
// h = the digest (hex; e = new BN(h) mod n, not truncated), r, s (2 B hex digits; s may be >= n),
// x, y = the key (2 B hex digits each; a coordinate may be >= p), want =
//   0 .. 3      what getKeyRecoveryParam returns
//   "throws"    it throws ('Unable to find valid recovery factor')
//   "offcurve"  the key is not on the curve: outside the engine's domain (status 2); the reference
//               is not asked
//   "outside"   r = 0, r >= n or s = 0 (mod n): outside the engine's domain (status 3); the
//               reference is not asked
// tag = what the row exercises.

var fs = require('fs');
var path = require('path');
var crypto = require('crypto');
var ref = require('./ref_loader').load();
var elliptic = ref.elliptic;
var BN = ref.BN;

var OUT = process.argv[2] || path.join(__dirname, '..', 'tests', 'golden');
var NAMES = ['secp256k1', 'p192', 'p224', 'p256', 'p384', 'p521'];
var LONG = { secp256k1: 40, p192: 32, p224: 32, p256: 40, p384: 64, p521: 73 };   // a hash longer than n

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

function gen(name) {
  var ec = new elliptic.ec(name);
  var c = ec.curve, n = ec.n, p = c.p, g = ec.g;
  var B = p.byteLength();
  if (n.byteLength() !== B) throw new Error('widths differ');
  var rng = new Prng('ellgpu-golden-key-recid-v1:' + name);
  var TOP = new BN(1).ushln(8 * B);
  var rows = [];
  var hex = function(v) { return v.toString(16, 2 * B); };
  var asked = function(h, r, s, Q) {
    try { return ec.getKeyRecoveryParam(h, { r: r, s: s }, Q); } catch (e) {
      if (!/Unable to find valid recovery factor/.test(e.message)) throw e;
      return 'throws';
    }
  };
  // a row whose answer is the reference's
  var rec = function(tag, h, r, s, Q, expect) {
    var want = asked(h, r, s, Q);
    if (expect !== undefined && String(want) !== String(expect)) throw new Error(name + ' ' + tag + ': ' + want + ', expected ' + expect);
    rows.push([tag, Buffer.from(h).toString('hex'), hex(r), hex(s), hex(Q.getX()), hex(Q.getY()), want]);
    return want;
  };
  var raw = function(tag, h, r, s, x, y, want) {
    rows.push([tag, Buffer.from(h).toString('hex'), hex(r), hex(s), hex(x), hex(y), want]);
  };
  // s = k^-1 (e + r d) with e = new BN(h) mod n, as recoverPubKey reads the hash (EC#sign truncates it)
  var sign = function(h, d, k) {
    for (;;) {
      var r = g.mul(k).getX().umod(n);
      var s = k.invm(n).mul(new BN(h).umod(n).add(r.mul(d))).umod(n);
      if (!r.isZero() && !s.isZero()) return { r: r, s: s };
      k = k.addn(1);
    }
  };
  var keys = [];
  for (var t = 0; t < 3; t++) {
    var d = rng.below(n);
    keys.push({ d: d, Q: g.mul(d) });
  }
  // ordinary signatures of three keys: hashes of 20 bytes, of n's length and longer
  var seen = {};
  keys.forEach(function(key, ki) {
    [20, B, LONG[name]].forEach(function(len) {
      for (var j = 0; j < 2; j++) {
        var h = rng.bytes(len);
        var sg = sign(h, key.d, rng.below(n));
        var id = rec('valid' + len, h, sg.r, sg.s, key.Q);
        seen[id] = true;
        if (j === 0) rec('flipped_s' + len, h, sg.r, n.sub(sg.s), key.Q, id ^ 1);
      }
    });
    // signed by EC#sign over the long hash: it truncates, recoverPubKey does not
    var hl = rng.bytes(LONG[name]);
    var es = ec.sign(hl, ec.keyFromPrivate(key.d), { canonical: ki & 1 });
    rec('ecsign_long', hl, es.r, es.s, key.Q);
    var hn = rng.bytes(B);
    es = ec.sign(hn, ec.keyFromPrivate(key.d));
    rec('ecsign_nlen', hn, es.r, es.s, key.Q);
  });
  while (!(seen[0] && seen[1])) {                 // both parities
    var h0 = rng.bytes(B);
    var s0 = sign(h0, keys[0].d, rng.below(n));
    seen[rec('valid' + B, h0, s0.r, s0.s, keys[0].Q)] = true;
  }
  // an unreduced s: s small, e solved from it (e = s k - r d), then s + n in the same bytes
  for (var u = 0; u < 3; u++) {
    var k = rng.below(n), ss = rng.bits(64).addn(1), key = keys[u];
    var r = g.mul(k).getX().umod(n);
    var e = ss.mul(k).sub(r.mul(key.d)).umod(n);
    var h = e.toArrayLike(Buffer, 'be', B);
    var id = rec('small_s', h, r, ss, key.Q);
    if (ss.add(n).cmp(TOP) >= 0) throw new Error('s + n does not fit');
    rec('s_plus_n', h, r, ss.add(n), key.Q, id);
  }
  // second candidates: x = n + d on the curve, r = d, any s and e, Q as recovered with 2 | parity
  var made = 0;
  for (var dd = 1; made < 6 && dd < 400; dd++) {
    try { c.pointFromX(n.addn(dd), made & 1); } catch (err) { continue; }
    var h2 = rng.bytes([20, B, LONG[name]][made % 3]);
    var r2 = new BN(dd), s2 = rng.below(n);
    var Q2 = ec.recoverPubKey(h2, { r: r2, s: s2 }, 2 + (made & 1));
    rec('second', h2, r2, s2, Q2, 2 + (made & 1));
    made++;
  }
  if (made < 6) throw new Error('no second candidates');
  // ... with r just below p - n, and r = p - n, which has none
  var pmn = p.sub(n);
  for (var j2 = 1; ; j2++) {
    var rj = pmn.subn(j2);
    try { c.pointFromX(rj.add(n), 1); } catch (err2) { continue; }
    var hj = rng.bytes(B), sj = rng.below(n);
    rec('second_top', hj, rj, sj, ec.recoverPubKey(hj, { r: rj, s: sj }, 3), 3);
    break;
  }
  var hp = rng.bytes(B);
  rec('r_is_p_minus_n', hp, pmn, rng.below(n), keys[1].Q, 'throws');
  // the reference throws: a wrong key, r +- 1, s +- 1, e G + r Q = O
  var ht = rng.bytes(B);
  var st = sign(ht, keys[2].d, rng.below(n));
  rec('wrong_key', ht, st.r, st.s, keys[0].Q, 'throws');
  rec('r_plus_1', ht, st.r.addn(1), st.s, keys[2].Q, 'throws');
  rec('r_minus_1', ht, st.r.subn(1), st.s, keys[2].Q, 'throws');
  rec('s_plus_1', ht, st.r, st.s.addn(1), keys[2].Q, 'throws');
  rec('s_minus_1', ht, st.r, st.s.subn(1), keys[2].Q, 'throws');
  var hb = Buffer.from(ht);
  hb[3] ^= 0x10;
  rec('hash_bit', hb, st.r, st.s, keys[2].Q, 'throws');
  var hh = rng.bytes(B);
  var ri = rng.below(n), ei = new BN(hh).umod(n);
  var Qi = g.mul(n.sub(ei.mul(ri.invm(n)).umod(n)));                     // Q = -(e / r) G
  if (!g.mul(ei).add(Qi.mul(ri)).isInfinity()) throw new Error('sum is not O');
  rec('sum_inf', hh, ri, rng.below(n), Qi, 'throws');
  // off the curve: y + 1, and a coordinate >= p that does not reduce to a point
  var Qo = keys[1].Q;
  raw('offcurve_y_plus_1', ht, st.r, st.s, Qo.getX(), Qo.getY().addn(1).umod(p), 'offcurve');
  for (var j3 = 1; ; j3++) {
    var xb = TOP.subn(j3);
    if (xb.cmp(p) < 0) throw new Error('no coordinate >= p fits');
    if (c.validate(c.point(xb, Qo.getY()))) continue;
    raw('offcurve_x_ge_p', ht, st.r, st.s, xb, Qo.getY(), 'offcurve');
    break;
  }
  // a coordinate >= p that does reduce to a point: reduced first, as curve.point() reduces it
  for (var x0 = 1; ; x0++) {
    var P0;
    try { P0 = c.pointFromX(new BN(x0), x0 & 1); } catch (err3) { continue; }
    if (P0.getX().add(p).cmp(TOP) >= 0) throw new Error('x + p does not fit');
    var w = asked(ht, st.r, st.s, c.point(P0.getX().add(p), P0.getY()));
    raw('key_x_plus_p', ht, st.r, st.s, P0.getX().add(p), P0.getY(), w);
    break;
  }
  if (keys[2].Q.getX().add(p).cmp(TOP) < 0 && keys[2].Q.getY().add(p).cmp(TOP) < 0) {
    var id2 = asked(ht, st.r, st.s, c.point(keys[2].Q.getX().add(p), keys[2].Q.getY().add(p)));
    if (id2 === 'throws') throw new Error('reduced key does not recover');
    raw('key_xy_plus_p', ht, st.r, st.s, keys[2].Q.getX().add(p), keys[2].Q.getY().add(p), id2);
  }
  // outside the engine's domain: the reference is not asked
  var Qk = keys[2].Q;
  raw('r_zero', ht, new BN(0), st.s, Qk.getX(), Qk.getY(), 'outside');
  raw('r_n', ht, n, st.s, Qk.getX(), Qk.getY(), 'outside');
  raw('r_n_plus_1', ht, n.addn(1), st.s, Qk.getX(), Qk.getY(), 'outside');
  raw('s_zero', ht, st.r, new BN(0), Qk.getX(), Qk.getY(), 'outside');
  raw('s_n', ht, st.r, n, Qk.getX(), Qk.getY(), 'outside');
  return { name: name, B: B, p: p.toString(16), n: n.toString(16), long: LONG[name], rows: rows };
}

var out = NAMES.map(gen);
var file = path.join(OUT, 'key_recid.json');
fs.writeFileSync(file, JSON.stringify(out, null, 0).replace(/\],\[/g, '],\n[') + '\n');
out.forEach(function(cv) {
  var hist = {};
  cv.rows.forEach(function(r) { hist[r[6]] = (hist[r[6]] || 0) + 1; });
  console.log(cv.name, cv.rows.length, JSON.stringify(hist));
});
console.log(file);
