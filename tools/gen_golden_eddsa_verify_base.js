'use strict';
// Golden vectors for EdDSA verification against a fixed-base table of the signer's key --
// ellgpu_eddsa_verify_base: every verdict is the reference's own `eddsa.verify(msg, sig, point)` with
// the key passed as a Point (eddsa/key.js:17-24).  Runs only where the reference is present (see
// tools/ref_loader.js); all randomness is SHA-256 counter mode over a fixed seed, so a rerun
// reproduces tests/golden/eddsa_verify_base.json byte for byte.
//
//   node tools/gen_golden_eddsa_verify_base.js [outdir]
//
//   keys     eight, each {name, x, y, a}: hex coordinates and, where there is one, the scalar a with
//            A = a G (+ T8 for the last one); null for none
//     G  negG  aG1  aG2 (keyFromSecret of seeded secrets, so that `sign` works)  identity (0, 1)
//     order2 (0, -1)  T8 (a point of order 8)  aG_T8 (a G + T8)
//   cases    per key, rows [tag, msg, sig, verdict]; msg and sig hex, verdict 1 / 0 or "throw: <message>".
//     valid0 valid1 valid47 valid48 valid175 valid176 valid300
//               message lengths on both sides of SHA-512's padding boundaries behind the 64-byte
//               prefix R || A.  aG1 / aG2: `eddsa.sign`.  The other keys: R = r G, S = r + h a with
//               a = 0 on the three torsion-only keys -- "valid" as built; with a torsion component
//               the reference accepts only where h kills it (h mod 8 on T8 and aG_T8, h mod 2 on order2)
//     flip_R flip_S flip_M   one bit of valid48 flipped
//     S_n  S_plus_n (the valid S plus n: false)  S_zero
//     R_undecodable   a y whose x^2 is a non-residue: the reference throws
//     R_x0_odd        y = 1 with the sign bit set: the reference throws
//     R_noncanon      R = the identity encoded as y = p + 1, S = h a with h over those bytes: the
//                     reference reduces y and accepts (asserted on the four keys with a known a)
//     torsion_k       (T8, aG_T8: a component of order 8) further messages, drawn until both verdicts
//                     occur among the built rows (valid* and torsion_*)
// The generator refuses to write a fixture in which a key lacks a tag or does not see both verdicts.

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
Prng.prototype.below = function(n) {
  for (;;) {
    var k = new BN(this.bytes(Math.ceil(n.bitLength() / 8))).maskn(n.bitLength());
    if (!k.isZero() && k.cmp(n) < 0) return k;
  }
};

var eddsa = new elliptic.eddsa('ed25519');
var curve = eddsa.curve;
var N = curve.n, P = curve.p;
var rng = new Prng('eddsa-verify-base');
var TAGS = ['valid0', 'valid1', 'valid47', 'valid48', 'valid175', 'valid176', 'valid300', 'flip_R', 'flip_S', 'flip_M',
  'S_n', 'S_plus_n', 'S_zero', 'R_undecodable', 'R_x0_odd', 'R_noncanon'];

function le32(bn) { return Buffer.from(bn.toArray('le', 32)); }
function arr(buf) { return Array.prototype.slice.call(buf); }
function verdict(msg, sig, A) {
  try { return eddsa.verify(arr(msg), arr(sig), A) ? 1 : 0; } catch (e) { return 'throw: ' + e.message; }
}

// a point of order 8: n * (a random curve point) has its prime-order part killed
function order8() {
  for (;;) {
    var y = new BN(rng.bytes(32)).umod(P), pt;
    try { pt = curve.pointFromY(y, false); } catch (e) { continue; }
    var t = pt.mul(N);
    if (!t.dbl().dbl().isInfinity()) return t;
  }
}
// a y that is no ordinate of the curve
function badY() {
  for (;;) {
    var y = new BN(rng.bytes(32)).maskn(255).umod(P);
    try { curve.pointFromY(y, false); } catch (e) { return y; }
  }
}

var G = curve.g;
var identity = curve.point(new BN(0), new BN(1));
var s1 = eddsa.keyFromSecret(arr(rng.bytes(32))), s2 = eddsa.keyFromSecret(arr(rng.bytes(32)));
var T8 = order8();
var aT = rng.below(N);
var keys = [
  { name: 'G', A: G, a: new BN(1) },
  { name: 'negG', A: G.neg(), a: N.subn(1) },
  { name: 'aG1', A: s1.pub(), a: s1.priv().umod(N), key: s1 },
  { name: 'aG2', A: s2.pub(), a: s2.priv().umod(N), key: s2 },
  { name: 'identity', A: identity, a: new BN(0), torsion: true },
  { name: 'order2', A: curve.point(new BN(0), P.subn(1)), a: new BN(0), torsion: true },
  { name: 'T8', A: T8, a: new BN(0), torsion: true, draw: true },
  { name: 'aG_T8', A: G.mul(aT).add(T8), a: aT, mixed: true, draw: true },
];

// R = r G, S = r + h a: what a signer holding a would produce
function build(k, msg) {
  var r = rng.below(N);
  var Renc = Buffer.from(eddsa.encodePoint(G.mul(r)));
  var h = eddsa.hashInt(arr(Renc), eddsa.encodePoint(k.A), arr(msg));
  return Buffer.concat([Renc, le32(r.add(h.mul(k.a)).umod(N))]);
}
function signed(k, msg) {
  return k.key ? Buffer.from(eddsa.sign(arr(msg), k.key).toBytes()) : build(k, msg);
}

var cases = keys.map(function(k) {
  var rows = [], valid = {};
  function push(tag, msg, sig) { var v = verdict(msg, sig, k.A); rows.push([tag, msg.toString('hex'), sig.toString('hex'), v]); return v; }
  [0, 1, 47, 48, 175, 176, 300].forEach(function(len) {
    var msg = rng.bytes(len), sig = signed(k, msg);
    valid[len] = { msg: msg, sig: sig };
    var v = push('valid' + len, msg, sig);
    if (!k.torsion && !k.mixed && v !== 1) throw new Error(k.name + ': valid' + len + ' is not accepted');
  });
  var m48 = valid[48].msg, g48 = valid[48].sig, t;
  t = Buffer.from(g48); t[rng.bytes(1)[0] % 32] ^= 1 << (rng.bytes(1)[0] % 7); push('flip_R', m48, t);
  t = Buffer.from(g48); t[32 + rng.bytes(1)[0] % 31] ^= 1 << (rng.bytes(1)[0] % 8); push('flip_S', m48, t);
  t = Buffer.from(m48); t[rng.bytes(1)[0] % 48] ^= 1 << (rng.bytes(1)[0] % 8); push('flip_M', t, g48);
  push('S_n', m48, Buffer.concat([g48.slice(0, 32), le32(N)]));
  push('S_plus_n', m48, Buffer.concat([g48.slice(0, 32), le32(new BN(arr(g48.slice(32)), 'le').add(N))]));
  push('S_zero', m48, Buffer.concat([g48.slice(0, 32), le32(new BN(0))]));
  var v = push('R_undecodable', m48, Buffer.concat([le32(badY()), g48.slice(32)]));
  if (typeof v !== 'string') throw new Error('R_undecodable did not throw');
  var x0 = Buffer.alloc(32); x0[0] = 1; x0[31] = 0x80;
  v = push('R_x0_odd', m48, Buffer.concat([x0, g48.slice(32)]));
  if (typeof v !== 'string') throw new Error('R_x0_odd did not throw');
  var nc = le32(P.addn(1));
  var h = eddsa.hashInt(arr(nc), eddsa.encodePoint(k.A), arr(m48));
  v = push('R_noncanon', m48, Buffer.concat([nc, le32(h.mul(k.a).umod(N))]));
  if (!k.torsion && !k.mixed && v !== 1) throw new Error(k.name + ': R_noncanon is not accepted');
  if (k.draw) {
    var seen = function(want) { return rows.some(function(r) { return /^(valid|torsion_)/.test(r[0]) && r[3] === want; }); };
    for (var j = 0; !(seen(0) && seen(1)); j++) {
      if (j > 200) throw new Error(k.name + ': no message with both verdicts');
      var msg = rng.bytes(32);
      push('torsion_' + j, msg, build(k, msg));
    }
  }
  var tags = {}, verdicts = {};
  rows.forEach(function(r) { tags[r[0]] = 1; verdicts[r[3]] = 1; });
  TAGS.forEach(function(tg) { if (!tags[tg]) throw new Error(k.name + ': no case ' + tg); });
  if (!verdicts[0] || !verdicts[1]) throw new Error(k.name + ': does not see both verdicts');
  return rows;
});

var lines = ['{', '"curve": "ed25519",', '"n": "' + N.toString(16) + '",', '"p": "' + P.toString(16) + '",',
  '"tags": ' + JSON.stringify(TAGS) + ',', '"keys": ['];
keys.forEach(function(k, i) {
  lines.push(JSON.stringify({ name: k.name, x: k.A.getX().toString(16), y: k.A.getY().toString(16),
    a: k.torsion ? null : k.a.toString(16) }) + (i + 1 < keys.length ? ',' : ''));
});
lines.push('],', '"cases": [');
cases.forEach(function(rows, i) {
  lines.push('[');
  rows.forEach(function(r, j) { lines.push(JSON.stringify(r) + (j + 1 < rows.length ? ',' : '')); });
  lines.push(i + 1 < cases.length ? '],' : ']');
});
lines.push(']', '}');
var file = path.join(OUT, 'eddsa_verify_base.json');
fs.writeFileSync(file, lines.join('\n') + '\n');
console.log('wrote ' + file + ': ' + keys.length + ' keys, ' + cases.reduce(function(s, r) { return s + r.length; }, 0) + ' cases');
