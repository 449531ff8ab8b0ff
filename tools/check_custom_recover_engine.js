'use strict';
// EC#recoverPubKey on user-defined domains through the N-API addon: on every domain of
// tests/golden/custom_recover.json, Engine#customRecoverBatch and its Async form equal the
// reference's recorded answers -- status 0 with the point, 1 for infinity, 2 for every thrown
// message, 3 for r = 0 or r >= n; the point is zeroed unless the status is 0.  One engine call per
// batch (a batch = the cases of one digest length).  A plain curve id is refused.  The library is
// ELLGPU_LIB's (the CPU unit-test build) or the device's.  Prints one JSON line.
//
//   [ELLGPU_LIB=...] node tools/check_custom_recover_engine.js

var path = require('path');
var Engine = require('../elliptic_amd/js/index.js').Engine;
var golden = require(path.join(__dirname, '..', 'tests', 'golden', 'custom_recover.json'));

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
var ZERO = Buffer.alloc(64).toString('hex');

function check(c, vs, res, what) {
  vs.forEach(function(v, i) {
    if ((v.st === 2) !== (v.msg !== undefined)) fail(c.name + ': a fixture row with status ' + v.st + ' and msg ' + v.msg);
    var want = v.st === 0 ? v.x + v.y : ZERO;
    if (res.status[i] !== v.st || res.xy.slice(64 * i, 64 * i + 64).toString('hex') !== want)
      fail(c.name + ' ' + what + ' ' + v.tag + ' j=' + v.j + ' r=' + v.r + ': status ' + res.status[i] + ', want ' + v.st);
    checked++;
  });
}

golden.forEach(function(c) {
  var id = eng.defineShortDomain(b32(c.p), b32(c.a), b32(c.b), b32(c.n), b32(c.g.x), b32(c.g.y));
  groupBy(c.recover, function(v) { return String(v.h.length / 2 + 1000); }).forEach(function(vs) {
    var hl = vs[0].h.length / 2;
    var h = Buffer.concat(vs.map(function(v) { return hex(v.h); }));
    var r = Buffer.concat(vs.map(function(v) { return b32(v.r); }));
    var s = Buffer.concat(vs.map(function(v) { return b32(v.s); }));
    var j = Buffer.from(vs.map(function(v) { return v.j; }));
    var calls = eng.stats.gpuCalls;
    check(c, vs, eng.customRecoverBatch(id, h, hl, r, s, j), 'recover');
    if (eng.stats.gpuCalls !== calls + 1) fail('not one engine call per batch');
    pending.push(eng.customRecoverBatchAsync(id, h, hl, r, s, j).then(function(res) { check(c, vs, res, 'recoverAsync'); }));
  });
  // the plain curve under the domain has no order: refused
  var plain = eng.defineShort(b32(c.p), b32(c.a), b32(c.b));
  try {
    eng.customRecoverBatch(plain, Buffer.alloc(32), 32, Buffer.alloc(32, 1), Buffer.alloc(32, 1), Buffer.alloc(1));
  } catch (e) { checked++; return; }
  fail(c.name + ': customRecoverBatch accepted a plain curve id');
});
Promise.all(pending).then(function() {
  eng.close();
  console.log(JSON.stringify({ ok: true, checked: checked, curves: golden.length }));
  process.exit(0);
}, function(e) { fail('async: ' + e.message); });
