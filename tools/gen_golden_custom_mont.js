'use strict';
// Golden vectors for user-defined Montgomery curves -- ellgpu_custom_mont_ladder, _validate,
// _derive: every abscissa, Z == 0 flag, validate answer and derive answer (or the message
// thrown) from the reference itself.  Runs only where the reference is present (see
// tools/ref_loader.js); all randomness is SHA-256 counter mode over a fixed seed, so a rerun
// reproduces tests/golden/custom_mont.json byte for byte.
//
//   node tools/gen_golden_custom_mont.js [outdir]
//
// Curves (b = 1 throughout: no formula of mont.js reads b):
//   c25519_user  2^255 - 19, a = 486662      p = 1 mod 4; curve25519 written out by hand
//   m221         2^221 - 3,  a = 117050      p.byteLength() = 28, p = 1 mod 4
//   bp256_mont   brainpoolP256r1's p, a 256-bit a from the PRNG   p = 3 mod 4, full-width a24
//   top256_mont  2^256 - 189, a from the PRNG                     p = 3 mod 4, top of the range
//   toy_p23      23, a = 5                   every x in 0..22 with every k in 0..30
//
// One case = (k, x), the point being curve.point(x, 1) as decodePoint builds it:
//   k, x     64 hex digits; x may be >= p (toRed reduces it)
//   z0       1 where Point#mul(k) has z == 0 (read BEFORE getX, which normalizes in place)
//   getx     Point#mul(k).getX(): 0 where z0 (redInvm of 0 is 0 on a curve without a prime name)
//   valid    MontCurve#validate: 1 true, 0 false; absent where it throws -- then vmsg
//   derive   KeyPair#derive(pub) of a key pair whose priv is k (n = 2^256, so _importPrivate leaves
//            k as it stands): 64 hex digits; absent where it throws -- then dmsg
//   tag      what the case exercises
// The toy curve's 713 cases are written one row per x instead (`rows`): x, valid / vmsg and dmsg as
// above (they depend on x alone), and z0, getx, derive as lists over k = 0..30 of plain numbers.

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

function hex32(bn) { return bn.toString(16, 64); }

var TOP = new BN(1).ushln(256);
var P25519 = new BN(1).ushln(255).subn(19);
var BP256 = new BN('a9fb57dba1eea9bc3e660a909d838d726e3bf623d52620282013481d1f6e5377', 16);
var arng = new Prng('ellgpu-golden-v1:custom-mont:coefficients');
var SPECS = [
  { name: 'c25519_user', p: P25519, a: new BN(486662) },
  { name: 'm221', p: new BN(1).ushln(221).subn(3), a: new BN(117050) },
  { name: 'bp256_mont', p: BP256, a: arng.bits(256).umod(BP256) },
  { name: 'top256_mont', p: TOP.subn(189), a: arng.bits(256).umod(TOP.subn(189)) },
  { name: 'toy_p23', p: new BN(23), a: new BN(5), toy: true },
];

function gen(spec) {
  var rng = new Prng('ellgpu-golden-v1:custom-mont:' + spec.name);
  var p = spec.p;
  // a curve without a `prime` name: bn.js's generic Mont reduction context
  // (not through PresetCurve, which insists on G * n = O: the key pairs below need an n only so that
  // _importPrivate's umod(n) leaves every 256-bit priv as it stands, and G is never used)
  var curve = new elliptic.curve.mont({ p: p.toString(16), a: spec.a.toString(16), b: '1', n: TOP.toString(16), g: ['9'] });
  var ec = new elliptic.ec({ curve: { curve: curve, n: curve.n, g: curve.g }, hash: hash.sha256 });
  if (curve.red.prime) throw new Error('expected the generic reduction context');
  var o = { name: spec.name, p: hex32(p), a: hex32(curve.a.fromRed()), a24: hex32(curve.a24.fromRed()), pl: p.byteLength(),
    pmod4: p.modn(4), cases: [] };

  function validity(x) {
    try { return curve.point(x.clone(), 1).validate() ? 1 : 0; } catch (e) { return String(e.message); }
  }
  function add(tag, k, x) {
    var c = { tag: tag, k: hex32(k), x: hex32(x) };
    var R = curve.point(x.clone(), 1).mul(k.clone());
    c.z0 = R.z.cmpn(0) === 0 ? 1 : 0;
    c.getx = hex32(R.getX());
    var v = validity(x);
    if (typeof v === 'number') c.valid = v; else c.vmsg = v.slice(0, 60);
    try {
      c.derive = hex32(ec.keyFromPrivate(k.clone()).derive(curve.point(x.clone(), 1)));
    } catch (e) {
      c.dmsg = String(e.message).slice(0, 60);
    }
    o.cases.push(c);
    return c;
  }

  if (spec.toy) {
    o.rows = [];
    for (var x = 0; x < 23; x++) {
      for (var k = 0; k <= 30; k++) add('exhaustive', new BN(k), new BN(x));
      var cs = o.cases.splice(0), r = { x: x, z0: [], getx: [] };
      ['valid', 'vmsg', 'dmsg'].forEach(function(f) {
        if (cs.some(function(c) { return c[f] !== cs[0][f]; })) throw new Error(f + ' depends on k');
        if (cs[0][f] !== undefined) r[f] = cs[0][f];
      });
      if (cs[0].derive !== undefined) r.derive = [];
      cs.forEach(function(c) {
        r.z0.push(c.z0);
        r.getx.push(parseInt(c.getx, 16));
        if (r.derive) r.derive.push(parseInt(c.derive, 16));
      });
      o.rows.push(r);
    }
    delete o.cases;
    return o;
  }

  // abscissae found by search: valid ones and non-residues
  var good = [], bad = [];
  while (good.length < 8 || bad.length < 4) {
    var cand = rng.bits(256).umod(p);
    var v = validity(cand);
    if (v === 1) { if (good.length < 8) good.push(cand); } else if (bad.length < 4) bad.push(cand);
  }
  var scalars = [
    ['k_0', new BN(0)], ['k_1', new BN(1)], ['k_2', new BN(2)], ['k_3', new BN(3)],
    ['k_2^255', new BN(1).ushln(255)], ['k_2^256-1', TOP.subn(1)],
  ];
  [8, 31, 32, 33, 64, 128, 191, 224].forEach(function(b) {      // long runs of leading zero bytes
    scalars.push(['k_' + b + '_bits', rng.bits(b).setn(b - 1, 1)]);
  });
  for (var i = 0; i < 40; i++) scalars.push(['k_random', rng.bits(256)]);

  scalars.forEach(function(s, j) { add(s[0], s[1], good[j % good.length]); });
  var special = [['x_0', new BN(0)], ['x_1', new BN(1)], ['x_p-1', p.subn(1)], ['x_p', p], ['x_p+1', p.addn(1)],
    ['x_2^256-1', TOP.subn(1)]];
  special.forEach(function(sx) {
    if (sx[1].cmp(TOP) >= 0) return;
    [0, 1, 5, 14].forEach(function(j) { add(sx[0] + ':' + scalars[j][0], scalars[j][1], sx[1]); });
  });
  if (spec.name === 'c25519_user') add('low_order_x_1_k_4', new BN(4), new BN(1));
  good.slice(0, 2).forEach(function(gx, j) {
    if (gx.add(p).cmp(TOP) < 0) add('valid_x_plus_p', scalars[16 + j][1], gx.add(p));
  });
  bad.forEach(function(bx, j) {
    add('non_residue:k_random', scalars[20 + j][1], bx);
    add('non_residue:' + scalars[j][0], scalars[j][1], bx);
    if (j < 2 && bx.add(p).cmp(TOP) < 0) add('non_residue_x_plus_p', scalars[30 + j][1], bx.add(p));
  });
  return o;
}

var out = SPECS.map(gen);
var file = path.join(OUT, 'custom_mont.json');
fs.writeFileSync(file, JSON.stringify(out).replace(/\{"(tag|x)"/g, '\n{"$1"') + '\n');
out.forEach(function(c) {
  var h = { z0: 0, valid: 0, invalid: 0, vthrow: 0, derive: 0, dthrow: {} };
  if (c.rows) return console.log(c.name + ': ' + c.rows.length + ' rows of ' + c.rows[0].z0.length);
  c.cases.forEach(function(r) {
    h.z0 += r.z0;
    if (r.valid === 1) h.valid++; else if (r.valid === 0) h.invalid++; else h.vthrow++;
    if (r.derive) h.derive++; else h.dthrow[r.dmsg] = (h.dthrow[r.dmsg] || 0) + 1;
  });
  console.log(c.name + ': ' + c.cases.length + ' cases ' + JSON.stringify(h));
});
console.log('wrote ' + file + ' (' + fs.statSync(file).size + ' bytes)');
