'use strict';
// install() on ECDSA over USER-DEFINED short curves (tests/golden/custom_ecdsa.json's domains): the
// patched library's EC#verify, eng.verifyMany, eng.verifyManyAsync and eng.verifyAsync must answer
// what an unpatched copy of the reference answers -- verdicts and thrown errors -- on every fixture
// case and on random draws; a 1 000-item verifyMany must be ONE engine call; edits of ec.n, curve.n,
// curve.g or a G table entry after first use must give the reference's answer; with
// options.customCurves === false (ELLGPU_CUSTOM=0) no verify may reach the engine.  Prints one JSON line.
//   ELLGPU_LIB=<hostsim or real library> [ELLGPU_CUSTOM=0] node tools/check_custom_ecdsa.js
var path = require('path');
var crypto = require('crypto');
var loader = require('./ref_loader');
var plain = loader.load();
var patchedRef = loader.load();
var CUSTOM = process.env.ELLGPU_CUSTOM !== '0';
var eng = require('../elliptic_amd/js').install(patchedRef.elliptic, { libPath: process.env.ELLGPU_LIB,
  customCurves: CUSTOM });
var golden = require(path.join(__dirname, '..', 'tests', 'golden', 'custom_ecdsa.json'));
var checked = 0;

function fail(m) { console.log(JSON.stringify({ ok: false, error: m })); process.exit(1); }
function build(lib, c) {
  var pc = new lib.elliptic.curves.PresetCurve({ type: 'short', prime: null, p: c.p, a: c.a, b: c.b, n: c.n,
    hash: lib.breq(19).sha256, gRed: false, g: [c.g.x, c.g.y] });
  return new lib.elliptic.ec(pc);
}
function outcome(f) {
  try { return 'v:' + !!f(); } catch (e) { return 'e:' + e.message; }
}
function item(c) {
  var o = { msg: Buffer.from(c.h, 'hex'), signature: { r: c.r, s: c.s }, key: { x: c.q.x, y: c.q.y } };
  if (c.bits) o.options = { msgBitLength: c.bits };
  return o;
}
function ver(ec, it) { return ec.verify(it.msg, it.signature, ec.keyFromPublic(it.key, 'hex'), undefined, it.options); }
function cmpOne(ecp, ecq, it, what) {
  var a = outcome(function() { return ver(ecp, it); }), b = outcome(function() { return ver(ecq, it); });
  if (a !== b) fail(what + ': reference ' + a + ', patched ' + b);
  checked++;
  return a;
}
function rnd(n) { return crypto.randomBytes(n); }
function draws(ecp, count, hl) {
  var out = [];
  for (var i = 0; i < count; i++) {
    var kp = ecp.keyFromPrivate(rnd(40));
    if (kp.getPrivate().isZero()) continue;
    var h = rnd(hl), sig;
    try { sig = kp.sign(h); } catch (e) {          // secp112r1: HmacDRBG wants 192 bits of key
      var k = ecp.keyFromPrivate(rnd(40)).getPrivate(), n = ecp.n;
      var r = ecp.g.mul(k).getX().umod(n), m = ecp._truncateToN(h);
      sig = { r: r, s: k.invm(n).mul(m.add(kp.getPrivate().mul(r))).umod(n) };
    }
    var r = sig.r.toString(16), s = sig.s.toString(16);
    var kind = i % 4;
    if (kind === 1) h[0] ^= 1;
    if (kind === 2) s = sig.s.addn(1).toString(16);
    var pub = kp.getPublic();
    out.push({ msg: h, signature: { r: r, s: s }, key: { x: pub.getX().toString(16), y: pub.getY().toString(16) } });
  }
  return out;
}
function groupsOf(items) {
  var g = {};
  items.forEach(function(it) {
    var k = it.msg.length + ':' + (it.options ? it.options.msgBitLength : 0);
    (g[k] = g[k] || []).push(it);
  });
  return Object.keys(g).map(function(k) { return g[k]; });
}
function manyItems(ecq, its) {
  return its.map(function(it) { return { msg: it.msg, signature: it.signature, key: ecq.keyFromPublic(it.key, 'hex'), options: it.options }; });
}

var jobs = [];
var calls0 = eng.stats.gpuCalls;
golden.forEach(function(c) {
  var ecp = build(plain, c), ecq = build(patchedRef, c);
  var its = c.verify.map(item).concat(draws(ecp, 24, 32));
  var want = its.map(function(it, i) { return cmpOne(ecp, ecq, it, c.name + ' verify #' + i); });
  groupsOf(its).forEach(function(g) {
    var ref = g.map(function(it) { return outcome(function() { return ver(ecp, it); }); });
    var got;
    try { got = eng.verifyMany(ecq, manyItems(ecq, g)); } catch (e) { got = null; }
    if (got && ref.every(function(r) { return r[0] === 'v'; }))
      got.forEach(function(v, i) { if ('v:' + v !== ref[i]) fail(c.name + ' verifyMany #' + i); checked++; });
    jobs.push(eng.verifyManyAsync(ecq, manyItems(ecq, g)).then(function(v) {
      v.forEach(function(x, i) { if ('v:' + x !== ref[i]) fail(c.name + ' verifyManyAsync #' + i); checked++; });
    }, function(e) { if (ref.every(function(r) { return r[0] === 'v'; })) fail(c.name + ' verifyManyAsync threw ' + e.message); }));
    g.forEach(function(it, i) {
      jobs.push(eng.verifyAsync(ecq, it.msg, it.signature, ecq.keyFromPublic(it.key, 'hex'), it.options).then(function(v) {
        if ('v:' + v !== ref[i]) fail(c.name + ' verifyAsync #' + i + ': ' + v + ' vs ' + ref[i]);
        checked++;
      }, function(e) { if ('e:' + e.message !== ref[i]) fail(c.name + ' verifyAsync threw ' + e.message); checked++; }));
    });
  });
  if (!want.some(function(w) { return w === 'v:true'; })) fail(c.name + ': no accepted signature');
});

Promise.all(jobs).then(function() {
  if (!CUSTOM) {
    if (eng.stats.gpuCalls !== calls0) fail('customCurves: false, yet ' + (eng.stats.gpuCalls - calls0) + ' engine calls');
    console.log(JSON.stringify({ ok: true, checked: checked, custom: false, gpuCalls: 0 }));
    process.exit(0);
  }
  if (eng.stats.gpuCalls === calls0) fail('no verify reached the engine');
  // 1 000 brainpoolP256r1 signatures: one engine call
  var c = golden[0];
  var ecp = build(plain, c), ecq = build(patchedRef, c);
  var its = draws(ecp, 1000, 32);
  var want = its.map(function(it) { return ver(ecp, it); });
  var before = eng.stats.gpuCalls;
  var t0 = process.hrtime();
  var got = eng.verifyMany(ecq, manyItems(ecq, its));
  var dt = process.hrtime(t0);
  if (eng.stats.gpuCalls - before !== 1) fail('1 000-item verifyMany cost ' + (eng.stats.gpuCalls - before) + ' engine calls');
  got.forEach(function(v, i) { if (v !== want[i]) fail('1 000-item verifyMany #' + i); checked++; });
  // edits after first use (both libraries get the same edit)
  var it0 = its[0];
  function both(edit, what) {
    edit(ecp); edit(ecq);
    cmpOne(ecp, ecq, it0, what);
    var a = its.slice(0, 8).map(function(it) { return ver(ecp, it); });
    var b = eng.verifyMany(ecq, manyItems(ecq, its.slice(0, 8)));
    a.forEach(function(v, i) { if (v !== b[i]) fail(what + ': verifyMany #' + i); checked++; });
  }
  var e1 = build(plain, c), e2 = build(patchedRef, c);
  ecp = e1; ecq = e2;
  cmpOne(ecp, ecq, it0, 'fresh');
  both(function(ec) { ec.g.precompute(); }, 'G precomputed');
  both(function(ec) { var d = ec.g.precomputed.doubles.points; d[3] = d[3].add(ec.g); }, 'G table entry edited');
  ecp = build(plain, c); ecq = build(patchedRef, c);
  cmpOne(ecp, ecq, it0, 'fresh 2');
  both(function(ec) { ec.n = ec.n.subn(2); }, 'ec.n replaced');
  ecp = build(plain, c); ecq = build(patchedRef, c);
  cmpOne(ecp, ecq, it0, 'fresh 3');
  both(function(ec) { ec.curve.n.isubn(2); }, 'curve.n edited in place');
  ecp = build(plain, c); ecq = build(patchedRef, c);
  cmpOne(ecp, ecq, it0, 'fresh 4');
  both(function(ec) { ec.curve.g = ec.curve.g.dbl(); ec.g = ec.curve.g; }, 'curve.g replaced');
  console.log(JSON.stringify({ ok: true, checked: checked, custom: true, verifyMany1000_ms: dt[0] * 1e3 + dt[1] / 1e6,
    offCurve: eng.stats.offCurve, passthrough: eng.stats.passthrough }));
  process.exit(0);
}, function(e) { fail(String(e && e.stack || e)); });
