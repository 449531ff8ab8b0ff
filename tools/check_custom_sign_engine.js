'use strict';
// EC#sign on user-defined domains through the N-API addon: on every domain of
// tests/golden/custom_sign.json, Engine#customSignBatch / customSignDetBatch and their Async forms
// equal the reference's recorded answers -- r, s, the recovery parameter and the acceptance; r, s
// and recid are zeroed where the reference went on to another nonce.  A record of a thrown
// 'Not enough entropy' expects customSignDetBatch to throw.  One engine call per batch (a batch =
// the cases of one digest length, msgBitLength, canonical value and hash).  A plain curve id is
// refused.  The library is ELLGPU_LIB's (the CPU unit-test build) or the device's.  Prints one JSON
// line.
//
//   [ELLGPU_LIB=...] node tools/check_custom_sign_engine.js

var path = require('path');
var Engine = require('../elliptic_amd/js/index.js').Engine;
var golden = require(path.join(__dirname, '..', 'tests', 'golden', 'custom_sign.json'));

function hex(h) { return Buffer.from(h, 'hex'); }
function b32(h) { var b = Buffer.alloc(32); var v = hex(h.length % 2 ? '0' + h : h); v.copy(b, 32 - v.length); return b; }
function fail(msg) { console.log(JSON.stringify({ ok: false, error: msg })); process.exit(1); }
function groupBy(items, keyOf) {
  var g = {};
  items.forEach(function(v) { var k = keyOf(v); (g[k] = g[k] || []).push(v); });
  return Object.keys(g).sort().map(function(k) { return g[k]; });
}

var eng = new Engine();
var checked = 0;
var pending = [];
var ZERO = Buffer.alloc(32).toString('hex');

function check(c, vs, res, what) {
  vs.forEach(function(v, i) {
    var ok = v.r !== undefined ? 1 : 0;
    var want = ok ? [v.r, v.s, v.j, 1] : [ZERO, ZERO, 0, 0];
    var got = [res.r.slice(32 * i, 32 * i + 32).toString('hex'), res.s.slice(32 * i, 32 * i + 32).toString('hex'),
      res.recid[i], res.ok[i]];
    if (JSON.stringify(got) !== JSON.stringify(want))
      fail(c.name + ' ' + what + ' ' + v.tag + ': ' + JSON.stringify(got) + ', want ' + JSON.stringify(want));
    checked++;
  });
}
function keyOf(v) { return [v.h.length / 2 + 1000, v.bits + 1000, v.c, v.hash || '', v.msg ? 1 : 0].join(':'); }

golden.forEach(function(c) {
  var id = eng.defineShortDomain(b32(c.p), b32(c.a), b32(c.b), b32(c.n), b32(c.g.x), b32(c.g.y));
  groupBy(c.det, keyOf).forEach(function(vs) {
    var v0 = vs[0], hl = v0.h.length / 2;
    var h = Buffer.concat(vs.map(function(v) { return hex(v.h); }));
    var d = Buffer.concat(vs.map(function(v) { return b32(v.d); }));
    if (v0.msg) {
      try {
        eng.customSignDetBatch(id, h, hl, v0.bits, d, v0.hash, v0.c);
      } catch (e) {
        if (!/Not enough entropy/.test(e.message) || !/Not enough entropy/.test(v0.msg)) fail(c.name + ': ' + e.message);
        checked += vs.length;
        pending.push(eng.customSignDetBatchAsync(id, h, hl, v0.bits, d, v0.hash, v0.c).then(function() {
          fail(c.name + ': customSignDetBatchAsync did not reject');
        }, function() { checked += vs.length; }));
        return;
      }
      fail(c.name + ': customSignDetBatch did not throw');
    }
    var calls = eng.stats.gpuCalls;
    check(c, vs, eng.customSignDetBatch(id, h, hl, v0.bits, d, v0.hash, v0.c), 'signDet');
    if (eng.stats.gpuCalls !== calls + 1) fail('not one engine call per batch');
    pending.push(eng.customSignDetBatchAsync(id, h, hl, v0.bits, d, v0.hash, v0.c).then(function(res) {
      check(c, vs, res, 'signDetAsync');
    }));
  });
  groupBy(c.sup, keyOf).forEach(function(vs) {
    var v0 = vs[0], hl = v0.h.length / 2;
    var h = Buffer.concat(vs.map(function(v) { return hex(v.h); }));
    var d = Buffer.concat(vs.map(function(v) { return b32(v.d); }));
    var k = Buffer.concat(vs.map(function(v) { return b32(v.k); }));
    var calls = eng.stats.gpuCalls;
    check(c, vs, eng.customSignBatch(id, h, hl, v0.bits, d, k, v0.c), 'sign');
    if (eng.stats.gpuCalls !== calls + 1) fail('not one engine call per batch');
    pending.push(eng.customSignBatchAsync(id, h, hl, v0.bits, d, k, v0.c).then(function(res) { check(c, vs, res, 'signAsync'); }));
  });
  // the plain curve under the domain has no order: refused
  var plain = eng.defineShort(b32(c.p), b32(c.a), b32(c.b));
  try {
    eng.customSignBatch(plain, Buffer.alloc(32), 32, 0, Buffer.alloc(32, 1), Buffer.alloc(32, 1), false);
  } catch (e) { checked++; return; }
  fail(c.name + ': customSignBatch accepted a plain curve id');
});
Promise.all(pending).then(function() {
  eng.close();
  console.log(JSON.stringify({ ok: true, checked: checked, curves: golden.length }));
  process.exit(0);
}, function(e) { fail('async: ' + e.message); });
