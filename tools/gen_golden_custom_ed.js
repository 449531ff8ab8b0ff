'use strict';
// Golden vectors for the key side of user-defined Edwards curves -- ellgpu_custom_ed_decompress,
// _decode_points, _validate, _derive, _derive_wire, _encode_points: every point, status and message
// from the reference itself.  Runs only where the reference is present (see tools/ref_loader.js);
// all randomness is SHA-256 counter mode over a fixed seed, so a rerun reproduces
// tests/golden/custom_ed.json byte for byte.
//
//   node tools/gen_golden_custom_ed.js [outdir]
//
// Large curves: the four of custom_edwards.json (Curve1174, E-222, two twisted curves over
// 2^255 - 19) and p224_d11: a = 1, d = 11 over the P-224 prime 2^224 - 2^96 + 1, whose p - 1 has
// 2-adicity 96 (the longest Tonelli-Shanks schedule) and whose least non-residue is 11.  d is a
// non-square and a a square on all five (checked below): the addition laws are complete.
// `n` is what KeyPair#validate multiplies by.  Curve1174 and E-222 have their published prime subgroup
// orders, with a generator of that order (checked below: n * G = O); the other curves' group orders
// are not known here, so their n is 4 and
// their "subgroup points" are the points of order 1, 2 and 4 -- the reference's pub.mul(n) decides
// either way, and the engine takes the scalar as it stands.
// Cases, by `op` (coordinates and scalars 64 hex digits, `msg` the message thrown):
//   fromx / fromy  v, odd -> xy | msg                      pointFromX / pointFromY (odd passed as a boolean:
//                                                          pointFromY compares it with !==)
//   decode         enc -> xy | msg                         decodePoint
//   validate       xy -> result, reason                    KeyPair#validate (with n)
//   derive         priv, xy [, enc] -> x | msg [, z0]        KeyPair#derive; with enc the peer key also
//                                                          goes through decodePoint (dmsg if that throws)
//   encode         xy -> compact, full                     Point#encode
// priv is set on the key pair AFTER _importPrivate (which would reduce it mod n): derive reads
// this.priv alone, and the engine uses priv as it stands.
// Toy curves (p13_d4, p13_d2, p17_d3, p19_d4; a = 1), exhaustive, one row per value v = 0 .. p - 1:
//   fx: [even, odd] results of pointFromX(v, odd), fy the same for pointFromY -- a result is [x, y]
//   or the message.

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
function legendre(x, p) {
  var r = x.toRed(BN.red(p)).redPow(p.subn(1).ushrn(1)).fromRed();
  return r.cmpn(1) === 0 ? 1 : r.isZero() ? 0 : -1;
}

var TOP = new BN(1).ushln(256);
var P25519 = new BN(1).ushln(255).subn(19);
var P1174 = new BN(1).ushln(251).subn(9);
var P224 = new BN(1).ushln(224).sub(new BN(1).ushln(96)).addn(1);
var golden = JSON.parse(fs.readFileSync(path.join(OUT, 'custom_edwards.json'), 'utf8'));
function dOf(name) { return new BN(golden.filter(function(c) { return c.name === name; })[0].d, 16); }
var BIG = [
  { name: 'curve1174', p: P1174, a: new BN(1), d: P1174.subn(1174),
    n: new BN(1).ushln(249).sub(new BN('11332719920821432534773113288178349711', 10)), cof: 4 },
  { name: 'e222', p: new BN(1).ushln(222).subn(117), a: new BN(1), d: new BN(160102),
    n: new BN('1684996666696914987166688442938726735569737456760058294185521417407', 10), cof: 4 },
  { name: 'twisted_a4', p: P25519, a: new BN(4), d: dOf('twisted_a4') },
  { name: 'twisted_am1', p: P25519, a: P25519.subn(1), d: dOf('twisted_am1'), aconf: '-1' },
  { name: 'p224_d11', p: P224, a: new BN(1), d: new BN(11) },
];
var TOY = [
  { name: 'p13_d4', p: 13, d: 4 }, { name: 'p13_d2', p: 13, d: 2 }, { name: 'p17_d3', p: 17, d: 3 },
  { name: 'p19_d4', p: 19, d: 4 },
];

function outcome(f, conv) {
  try { return { v: conv(f()) }; } catch (e) { return { msg: String(e.message).slice(0, 60) }; }
}

function genBig(spec) {
  var rng = new Prng('ellgpu-golden-v1:custom-ed:' + spec.name);
  var p = spec.p;
  if (legendre(spec.a, p) !== 1 || legendre(spec.d, p) !== -1) throw new Error(spec.name + ': addition law not complete');
  var conf = { p: p.toString(16), a: spec.aconf || spec.a.toString(16), c: '1', d: spec.d.toString(16) };
  var bare = new elliptic.curve.edwards(conf);
  if (bare.red.prime) throw new Error('expected the generic reduction context');
  // a base point: the least y >= 2 on the curve, cleared of the cofactor where the order is known
  var G = null;
  for (var y = 2; !G; y++) {
    try { G = bare.pointFromY(new BN(y), false); } catch (e) { G = null; }
    if (G && G.getX().isZero()) G = null;
  }
  var n = spec.n || new BN(4);
  if (spec.n) {
    G = G.mul(new BN(spec.cof));
    if (G.isInfinity() || !G.mul(n).isInfinity()) throw new Error(spec.name + ': n is not the order of G');
  }
  conf.n = n.toString(16);
  conf.g = [G.getX().toString(16), G.getY().toString(16)];
  var curve = new elliptic.curve.edwards(conf);
  var ec = new elliptic.ec({ curve: { curve: curve, n: curve.n, g: curve.g }, hash: hash.sha256 });
  var PL = p.byteLength();
  var o = { name: spec.name, p: hex32(p), a: hex32(curve.a.fromRed()), d: hex32(curve.d.fromRed()), n: hex32(n),
    pl: PL, pmod4: p.modn(4), cases: [] };
  function xyOf(P) { var q = curve.point(P.x, P.y, P.z, P.t); return hex32(q.getX()) + hex32(q.getY()); }
  function put(c, r, f) { if (r.msg !== undefined) c[f ? f + 'msg' : 'msg'] = r.msg; else c[f || 'xy'] = r.v; }
  function coord(op, tag, v, odd) {
    var c = { op: op, tag: tag, v: hex32(v), odd: odd ? 1 : 0 };
    put(c, outcome(function() { return op === 'fromx' ? curve.pointFromX(v.clone(), !!odd) : curve.pointFromY(v.clone(), !!odd); }, xyOf));
    o.cases.push(c);
    return c;
  }
  function decode(tag, bytes) {
    var c = { op: 'decode', tag: tag, enc: Buffer.from(bytes).toString('hex') };
    put(c, outcome(function() { return curve.decodePoint(bytes); }, xyOf));
    o.cases.push(c);
  }
  function validate(tag, x, y) {
    var r = ec.keyFromPublic({ x: x.toString(16), y: y.toString(16) }).validate();
    o.cases.push({ op: 'validate', tag: tag, xy: hex32(x) + hex32(y), result: r.result ? 1 : 0, reason: r.reason });
  }
  function derive(tag, k, x, y, enc) {
    var key = ec.keyFromPrivate(new BN(1));
    key.priv = k.clone();
    var c = { op: 'derive', tag: tag, priv: hex32(k) };
    var pub;
    if (enc) {
      c.enc = Buffer.from(enc).toString('hex');
      var d = outcome(function() { return curve.decodePoint(enc); }, function(P) { return P; });
      if (d.msg !== undefined) { c.dmsg = d.msg; o.cases.push(c); return; }
      pub = d.v;
    } else {
      c.xy = hex32(x) + hex32(y);
      pub = curve.point(x.toString(16), y.toString(16));
    }
    var R = outcome(function() { return pub.validate() ? pub.mul(k.clone()) : null; }, function(P) { return P; });
    if (R.v && R.v.z.cmpn(0) === 0) c.z0 = 1;
    put(c, outcome(function() { return key.derive(pub); }, hex32), 'x');
    o.cases.push(c);
  }
  function encode(tag, x, y) {
    var P = curve.point(x.toString(16), y.toString(16));
    o.cases.push({ op: 'encode', tag: tag, xy: hex32(x) + hex32(y), compact: P.encode('hex', true), full: P.encode('hex', false) });
  }
  function coords(P) { var q = curve.point(P.x, P.y, P.z, P.t); return [q.getX(), q.getY()]; }

  // ---- pointFromX / pointFromY
  var i, v;
  var seen = { fromx: {}, fromy: {} };
  ['fromx', 'fromy'].forEach(function(op) {
    [new BN(0), new BN(1), p.subn(1), p, p.addn(1), TOP.subn(1)].forEach(function(sv, j) {
      if (sv.cmp(TOP) < 0) [0, 1].forEach(function(odd) { coord(op, 'special_' + j, sv, odd); });
    });
    var good = 0, bad = 0;
    while (good < 3 || bad < 2) {
      v = rng.bits(256).umod(p);
      var c0 = coord(op, 'random', v, 0);
      var isGood = c0.xy !== undefined;
      if ((isGood && good >= 3) || (!isGood && bad >= 2)) { o.cases.pop(); continue; }
      coord(op, 'random', v, 1);
      if (isGood) good++; else bad++;
      if (isGood && good <= 1 && v.add(p).cmp(TOP) < 0) { coord(op, 'plus_p', v.add(p), 0); coord(op, 'plus_p', v.add(p), 1); }
    }
    seen[op] = o.cases.filter(function(c) { return c.op === op && c.tag === 'random'; });
  });
  // ---- the points the other calls work on
  var Q = [];                                                       // subgroup points (multiples of G)
  for (i = 0; i < 6; i++) Q.push(coords(G.mul(rng.bits(p.bitLength() + 8))));
  var ID = [new BN(0), new BN(1)], M1 = [new BN(0), p.subn(1)];       // (0, 1), (0, -1): orders 1 and 2
  var ainv = curve.a.redInvm().redSqrt();                             // (a^-1/2, 0): order 4
  var O4 = [ainv.fromRed(), new BN(0)];
  var shifted = coords(curve.point(Q[0][0].toString(16), Q[0][1].toString(16)).add(curve.point('0', p.subn(1).toString(16))));
  var off = [Q[1][0], Q[1][1].addn(1).umod(p)];
  // ---- decodePoint: every prefix, a hybrid parity mismatch, a wrong length
  function be(x) { return x.toArray('be', PL); }
  var bad02 = seen.fromx.filter(function(c) { return c.msg !== undefined; })[0];
  Q.slice(0, 2).forEach(function(q, j) {
    var par = q[1].isOdd() ? 1 : 0;
    decode('04', [4].concat(be(q[0]), be(q[1])));
    decode('hybrid_ok', [6 + par].concat(be(q[0]), be(q[1])));
    decode('hybrid_mismatch', [7 - par].concat(be(q[0]), be(q[1])));
    decode('02', [2].concat(be(q[0])));
    decode('03', [3].concat(be(q[0])));
    if (j === 0) {
      [0, 5, 255].forEach(function(t) { decode('prefix_' + t, [t].concat(be(q[0]), be(q[1]))); decode('prefix_' + t, [t].concat(be(q[0]))); });
      decode('04_short', [4].concat(be(q[0]), be(q[1])).slice(0, 2 * PL));
      decode('04_long', [4].concat(be(q[0]), be(q[1]), [0]));
      decode('02_short', [2].concat(be(q[0])).slice(0, PL));
      decode('02_long', [2].concat(be(q[0]), [1]));
      decode('04_as_02_length', [4].concat(be(q[0])));
      decode('02_as_04_length', [2].concat(be(q[0]), be(q[1])));
    }
  });
  decode('04_off_curve', [4].concat(be(off[0]), be(off[1])));
  [2, 3].forEach(function(t) { decode('no_root', [t].concat(be(new BN(bad02.v, 16)))); });
  var top = new BN(1).ushln(8 * PL).subn(1);                          // coordinates >= p
  decode('04_all_ones', [4].concat(be(top), be(top)));
  decode('02_all_ones', [2].concat(be(top)));
  decode('03_all_ones', [3].concat(be(top)));
  decode('04_p_and_p+1', [4].concat(be(p), be(p.addn(1))));
  // ---- KeyPair#validate
  Q.slice(0, 3).forEach(function(q) { validate('subgroup', q[0], q[1]); });
  validate('identity', ID[0], ID[1]);
  validate('identity_plus_p', p, p.addn(1));
  validate('minus_one', M1[0], M1[1]);
  validate('order_4', O4[0], O4[1]);
  validate('order_4_neg', p.sub(O4[0]), O4[1]);
  validate('shifted_by_(0,-1)', shifted[0], shifted[1]);
  validate('off_curve', off[0], off[1]);
  validate('off_curve_zero', new BN(0), new BN(0));
  if (Q[2][0].add(p).cmp(TOP) < 0) validate('subgroup_plus_p', Q[2][0].add(p), Q[2][1].add(p));
  // ---- KeyPair#derive, raw and over the wire
  var privs = [['0', new BN(0)], ['1', new BN(1)], ['n', n], ['2^256-1', TOP.subn(1)]];
  for (i = 0; i < 3; i++) privs.push(['random', rng.bits(256)]);
  privs.forEach(function(pv, j) {
    var q = Q[j % Q.length];
    derive('priv_' + pv[0], pv[1], q[0], q[1]);
    derive('priv_' + pv[0] + ':04', pv[1], null, null, [4].concat(be(q[0]), be(q[1])));
    derive('priv_' + pv[0] + ':compressed', pv[1], null, null, [q[1].isOdd() ? 3 : 2].concat(be(q[0])));
  });
  [['identity', ID], ['minus_one', M1], ['order_4', O4], ['shifted', shifted], ['off_curve', off]].forEach(function(pr, j) {
    (j ? [privs[4 + j % 3]] : [privs[1], privs[4]]).concat(j === 4 ? [privs[0]] : []).forEach(function(pv) {
      derive(pr[0] + ':priv_' + pv[0], pv[1], pr[1][0], pr[1][1]);
      derive(pr[0] + ':priv_' + pv[0] + ':04', pv[1], null, null, [4].concat(be(pr[1][0]), be(pr[1][1])));
    });
  });
  if (Q[3][0].add(p).cmp(TOP) < 0) derive('peer_plus_p', privs[4][1], Q[3][0].add(p), Q[3][1].add(p));
  var par0 = Q[0][1].isOdd() ? 1 : 0;
  derive('wire:hybrid_ok', privs[5][1], null, null, [6 + par0].concat(be(Q[0][0]), be(Q[0][1])));
  derive('wire:hybrid_mismatch', privs[5][1], null, null, [7 - par0].concat(be(Q[0][0]), be(Q[0][1])));
  derive('wire:prefix_5', privs[5][1], null, null, [5].concat(be(Q[0][0]), be(Q[0][1])));
  derive('wire:02_as_04_length', privs[5][1], null, null, [2].concat(be(Q[0][0]), be(Q[0][1])));
  derive('wire:no_root', privs[6][1], null, null, [2].concat(be(new BN(bad02.v, 16)), be(new BN(0))).slice(0, 1 + PL));
  derive('wire:no_root_04_length', privs[6][1], null, null, [3].concat(be(new BN(bad02.v, 16)), be(new BN(0))));
  // ---- Point#encode
  Q.slice(0, 4).forEach(function(q) { encode('subgroup', q[0], q[1]); });
  encode('identity', ID[0], ID[1]);
  encode('minus_one', M1[0], M1[1]);
  encode('off_curve', off[0], off[1]);
  if (Q[4][0].add(p).cmp(TOP) < 0) encode('plus_p', Q[4][0].add(p), Q[4][1].add(p));
  return o;
}

function genToy(spec) {
  var p = new BN(spec.p);
  var curve = new elliptic.curve.edwards({ p: p.toString(16), a: '1', c: '1', d: new BN(spec.d).toString(16) });
  var o = { name: spec.name, p: hex32(p), a: hex32(new BN(1)), d: hex32(new BN(spec.d)), pl: 1, pmod4: spec.p % 4, rows: [] };
  function res(f) {
    try { var P = f(); return [P.getX().toNumber(), P.getY().toNumber()]; } catch (e) { return String(e.message).slice(0, 60); }
  }
  for (var v = 0; v < spec.p; v++) {
    o.rows.push({ v: v,
      fx: [false, true].map(function(odd) { return res(function() { return curve.pointFromX(new BN(v), odd); }); }),
      fy: [false, true].map(function(odd) { return res(function() { return curve.pointFromY(new BN(v), odd); }); }) });
  }
  return o;
}

var out = BIG.map(genBig).concat(TOY.map(genToy));
var file = path.join(OUT, 'custom_ed.json');
fs.writeFileSync(file, JSON.stringify(out).replace(/\{"(op|v)"/g, '\n{"$1"') + '\n');
out.forEach(function(c) {
  if (c.rows) return console.log(c.name + ': ' + c.rows.length + ' rows');
  var h = {};
  c.cases.forEach(function(r) {
    var k = r.op + ':' + (r.msg || r.dmsg || r.xmsg || r.reason || 'ok');
    h[k] = (h[k] || 0) + 1;
  });
  console.log(c.name + ': ' + c.cases.length + ' cases ' + JSON.stringify(h));
});
console.log('wrote ' + file + ' (' + fs.statSync(file).size + ' bytes)');
