'use strict';
// The key side on user-defined domains through the N-API addon: on every domain of
// tests/golden/custom_ecdh.json, Engine#customDeriveBatch, customDeriveWireBatch,
// customValidateBatch and customEncodePointBatch and their Async forms equal the reference's recorded
// answers -- the shared secret (zeroed unless the status is 0), every status and decoder status,
// KeyPair#validate's reasons with and without the order test, both encodings.  One engine call
// per batch (a batch of derive_wire = the cases of one encoding length).  The order test on a plain
// curve id is refused.  The library is ELLGPU_LIB's (the CPU unit-test build) or the device's.
// Prints one JSON line.
//
//   [ELLGPU_LIB=...] node tools/check_custom_ecdh_engine.js

var path = require('path');
var Engine = require('../elliptic_amd/js/index.js').Engine;
var golden = require(path.join(__dirname, '..', 'tests', 'golden', 'custom_ecdh.json'));

function hex(h) { return Buffer.from(h, 'hex'); }
function b32(h) { var b = Buffer.alloc(32); var v = hex(h.length % 2 ? '0' + h : h); v.copy(b, 32 - v.length); return b; }
function fail(msg) { console.log(JSON.stringify({ ok: false, error: msg })); process.exit(1); }
function groupBy(items, keyOf) {
  var g = {};
  items.forEach(function(v) { var k = keyOf(v); (g[k] = g[k] || []).push(v); });
  return Object.keys(g).sort().map(function(k) { return g[k]; });
}
function cat(vs, f) { return Buffer.concat(vs.map(f)); }
function xy(v) { return Buffer.concat([b32(v.x), b32(v.y)]); }

var eng = new Engine();
var checked = 0;
var pending = [];
var ZERO = Buffer.alloc(32).toString('hex');

function checkDerive(c, vs, res, what, wire) {
  vs.forEach(function(v, i) {
    var want = v.st === 0 ? v.out : ZERO;
    if (res.status[i] !== v.st || res.x.slice(32 * i, 32 * i + 32).toString('hex') !== want ||
        (wire && res.err[i] !== v.err))
      fail(c.name + ' ' + what + ' ' + v.tag + ': status ' + res.status[i] + (wire ? ' err ' + res.err[i] : '') +
        ', want ' + v.st + (wire ? ' err ' + v.err : ''));
    checked++;
  });
}
function checkValidate(c, vs, res, key, what) {
  vs.forEach(function(v, i) {
    if (res.status[i] !== v[key]) fail(c.name + ' ' + what + ' ' + v.tag + ': status ' + res.status[i] + ', want ' + v[key]);
    checked++;
  });
}
function checkEncode(c, vs, res, key, what) {
  var w = res.enc.length / vs.length;
  vs.forEach(function(v, i) {
    if (res.enc.slice(w * i, w * i + w).toString('hex') !== v[key]) fail(c.name + ' ' + what + ' ' + v.tag);
    checked++;
  });
}
function once(f) {
  var calls = eng.stats.gpuCalls;
  var r = f();
  if (eng.stats.gpuCalls !== calls + 1) fail('not one engine call per batch');
  return r;
}

golden.forEach(function(c) {
  var id = eng.defineShortDomain(b32(c.p), b32(c.a), b32(c.b), b32(c.n), b32(c.g.x), b32(c.g.y));
  var vs = c.derive;
  var priv = cat(vs, function(v) { return b32(v.priv); }), pub = cat(vs, xy);
  checkDerive(c, vs, once(function() { return eng.customDeriveBatch(id, priv, pub); }), 'derive', false);
  (function(vs) {
    pending.push(eng.customDeriveBatchAsync(id, priv, pub).then(function(res) { checkDerive(c, vs, res, 'deriveAsync', false); }));
  })(vs);
  groupBy(c.derive_wire, function(v) { return String(v.enc.length / 2 + 1000); }).forEach(function(vs) {
    var len = vs[0].enc.length / 2;
    var priv = cat(vs, function(v) { return b32(v.priv); }), enc = cat(vs, function(v) { return hex(v.enc); });
    checkDerive(c, vs, once(function() { return eng.customDeriveWireBatch(id, priv, enc, len); }), 'deriveWire', true);
    pending.push(eng.customDeriveWireBatchAsync(id, priv, enc, len).then(function(res) { checkDerive(c, vs, res, 'deriveWireAsync', true); }));
  });
  var vv = c.validate;
  var pts = cat(vv, xy), inf = Buffer.from(vv.map(function(v) { return v.inf; }));
  checkValidate(c, vv, once(function() { return eng.customValidateBatch(id, pts, inf, true); }), 'st', 'validate');
  checkValidate(c, vv, once(function() { return eng.customValidateBatch(id, pts, inf, false); }), 'st0', 'validate0');
  pending.push(eng.customValidateBatchAsync(id, pts, inf, true).then(function(res) { checkValidate(c, vv, res, 'st', 'validateAsync'); }));
  pending.push(eng.customValidateBatchAsync(id, pts, inf, false).then(function(res) { checkValidate(c, vv, res, 'st0', 'validate0Async'); }));
  var ve = c.encode, epts = cat(ve, xy);
  // the row width is the engine's own record of p.byteLength(): given or not, the rows are c.pl wide
  [[false, 'full'], [true, 'compact']].forEach(function(m) {
    var res = once(function() { return eng.customEncodePointBatch(id, epts, m[0]); });
    if (res.enc.length !== ve.length * (1 + (m[0] ? 1 : 2) * c.pl)) fail(c.name + ': encode rows are not p.byteLength() wide');
    checkEncode(c, ve, res, m[1], 'encode');
    pending.push(eng.customEncodePointBatchAsync(id, epts, m[0], c.pl).then(function(res) { checkEncode(c, ve, res, m[1], 'encodeAsync'); }));
  });
  // a coordBytes that is not the curve's is refused before anything runs, in both forms: the
  // library would write rows of its own width into a result sized by the caller's
  [c.pl - 4, c.pl + 1].forEach(function(w) {
    var calls = eng.stats.gpuCalls;
    try {
      eng.customEncodePointBatch(id, epts, false, w);
    } catch (e) {
      if (!/coordBytes/.test(e.message) || eng.stats.gpuCalls !== calls) fail(c.name + ': wrong coordBytes: ' + e.message);
      checked++;
      return;
    }
    fail(c.name + ': customEncodePointBatch accepted coordBytes ' + w + ' on a curve of ' + c.pl);
  });
  pending.push(eng.customEncodePointBatchAsync(id, epts, true, c.pl - 1).then(function() {
    fail(c.name + ': customEncodePointBatchAsync accepted a wrong coordBytes');
  }, function(e) {
    if (!/coordBytes/.test(e.message)) throw e;
    checked++;
  }));
  // the plain curve under the domain has no order: the order test is refused, the rest is served
  var plain = eng.defineShort(b32(c.p), b32(c.a), b32(c.b));
  checkValidate(c, vv, eng.customValidateBatch(plain, pts, inf, false), 'st0', 'validate0 on the plain id');
  try {
    eng.customValidateBatch(plain, pts, inf, true);
  } catch (e) { checked++; return; }
  fail(c.name + ': customValidateBatch ran the order test on a plain curve id');
});
Promise.all(pending).then(function() {
  eng.close();
  console.log(JSON.stringify({ ok: true, checked: checked, curves: golden.length }));
  process.exit(0);
}, function(e) { fail('async: ' + e.message); });
