'use strict';
// ECDSA on user-defined Edwards domains through the N-API addon: on every domain of
// tests/golden/custom_ed_ecdsa.json, Engine#customEdVerifyBatch, customEdSignBatch and
// customEdSignDetBatch and their Async forms equal the reference's recorded answers -- EC#verify's
// verdict (status 2 for the keys recorded off the curve), EC#sign's r, s and recovery parameter,
// the acceptance of a supplied nonce, the refusal where EC#sign throws.  One engine call per batch
// (cases are grouped by digest length, msgBitLength, canonical and hash).  A plain Edwards id, a
// short id and a preset id are refused by these calls, and the domain id by the short-domain calls.
// The library is ELLGPU_LIB's (the CPU unit-test build) or the device's.  Prints one JSON line.
//
//   [ELLGPU_LIB=...] node tools/check_custom_ed_ecdsa_engine.js

var path = require('path');
var Engine = require('../elliptic_amd/js/index.js').Engine;
var golden = require(path.join(__dirname, '..', 'tests', 'golden', 'custom_ed_ecdsa.json'));

function b32(h) { var b = Buffer.alloc(32); var v = Buffer.from(h.length % 2 ? '0' + h : h, 'hex'); v.copy(b, 32 - v.length); return b; }
function fail(msg) { console.log(JSON.stringify({ ok: false, error: msg })); process.exit(1); }
function cat(vs, f) { return Buffer.concat(vs.map(f)); }
function hexRow(buf, i, w) { return buf.slice(w * i, w * i + w).toString('hex'); }

var eng = new Engine();
var checked = 0;
var pending = [];
var ZERO = '0'.repeat(64);

function once(f) {
  var calls = eng.stats.gpuCalls;
  var r = f();
  if (eng.stats.gpuCalls !== calls + 1) fail('not one engine call per batch');
  return r;
}
function refused(what, f) {
  try { f(); } catch (e) { checked++; return; }
  fail(what + ' was not refused');
}
function groups(cs, keyOf) {
  var g = {}, order = [];
  cs.forEach(function(c) { var k = keyOf(c); if (!g[k]) { g[k] = []; order.push(k); } g[k].push(c); });
  return order.map(function(k) { return g[k]; });
}
function checkVerify(d, cs, res, what) {
  cs.forEach(function(c, i) {
    var off = c.ok === undefined;
    var want = off ? [0, c.tag === 'off_curve_r_0' ? 0 : 2] : [c.ok, 0];
    if (res.ok[i] !== want[0] || res.status[i] !== want[1])
      fail(d.name + ' ' + what + ' ' + c.tag + ': ' + res.ok[i] + ' / ' + res.status[i] + ', want ' + want);
    checked++;
  });
}
function checkSign(d, cs, res, what) {
  cs.forEach(function(c, i) {
    var ok = c.r !== undefined && c.ok !== 0;
    var want = ok ? [c.r, c.s, c.j, 1] : [ZERO, ZERO, 0, 0];
    if (hexRow(res.r, i, 32) !== want[0] || hexRow(res.s, i, 32) !== want[1] || res.recid[i] !== want[2] || res.ok[i] !== want[3])
      fail(d.name + ' ' + what + ' ' + c.tag + ': ok ' + res.ok[i] + ', want ' + want[3]);
    checked++;
  });
}
function hashes(cs) { return cat(cs, function(c) { return Buffer.from(c.h, 'hex'); }); }

// a short curve and a plain Edwards curve for the refusals
var short = eng.defineShort(b32(golden[0].p), b32('01'), b32('07'));
golden.forEach(function(d) {
  var args = [d.p, d.a, d.d, d.n, d.gx, d.gy].map(b32);
  var id = eng.defineEdwardsDomain.apply(eng, args);
  if (eng.defineEdwardsDomain.apply(eng, args) !== id) fail(d.name + ': the same parameters gave another id');
  var plain = eng.defineEdwards(args[0], args[1], args[2]);
  if (plain === id || short === id) fail(d.name + ': the domain shares an id');
  groups(d.verify, function(c) { return c.h.length + ':' + c.bits; }).forEach(function(cs) {
    var hl = cs[0].h.length / 2, bits = cs[0].bits;
    var h = hashes(cs), r = cat(cs, function(c) { return b32(c.r); }), s = cat(cs, function(c) { return b32(c.s); });
    var q = cat(cs, function(c) { return Buffer.from(c.q, 'hex'); });
    checkVerify(d, cs, once(function() { return eng.customEdVerifyBatch(id, h, hl, bits, r, s, q); }), 'verify');
    pending.push(eng.customEdVerifyBatchAsync(id, h, hl, bits, r, s, q).then(function(res) { checkVerify(d, cs, res, 'verifyAsync'); }));
  });
  groups(d.det, function(c) { return [c.h.length, c.bits, c.c, c.hash, c.msg !== undefined].join(':'); }).forEach(function(cs) {
    var hl = cs[0].h.length / 2, bits = cs[0].bits, can = cs[0].c, hn = cs[0].hash;
    var h = hashes(cs), priv = cat(cs, function(c) { return b32(c.d); });
    if (cs[0].msg !== undefined) {                         // EC#sign throws: 'Not enough entropy'
      refused(d.name + ': customEdSignDetBatch where EC#sign throws', function() { eng.customEdSignDetBatch(id, h, hl, bits, priv, hn, can); });
      checked += cs.length - 1;
      pending.push(eng.customEdSignDetBatchAsync(id, h, hl, bits, priv, hn, can).then(
        function() { fail(d.name + ': customEdSignDetBatchAsync was not refused'); }, function() { checked += cs.length; }));
      return;
    }
    checkSign(d, cs, once(function() { return eng.customEdSignDetBatch(id, h, hl, bits, priv, hn, can); }), 'signDet');
    pending.push(eng.customEdSignDetBatchAsync(id, h, hl, bits, priv, hn, can).then(function(res) { checkSign(d, cs, res, 'signDetAsync'); }));
  });
  groups(d.sup, function(c) { return [c.h.length, c.bits, c.c].join(':'); }).forEach(function(cs) {
    var hl = cs[0].h.length / 2, bits = cs[0].bits, can = cs[0].c;
    var h = hashes(cs), priv = cat(cs, function(c) { return b32(c.d); }), ks = cat(cs, function(c) { return b32(c.k); });
    checkSign(d, cs, once(function() { return eng.customEdSignBatch(id, h, hl, bits, priv, ks, can); }), 'sign');
    pending.push(eng.customEdSignBatchAsync(id, h, hl, bits, priv, ks, can).then(function(res) { checkSign(d, cs, res, 'signAsync'); }));
  });
  // refusals: the new calls on a plain Edwards, a short and a preset id; the short-domain calls on the domain id
  var h1 = Buffer.alloc(32, 7), one = b32('09'), pt = Buffer.concat([b32(d.gx), b32(d.gy)]);
  [plain, short, 'ed25519', 'secp256k1'].forEach(function(bad) {
    refused(d.name + ': customEdVerifyBatch on ' + bad, function() { eng.customEdVerifyBatch(bad, h1, 32, 0, one, one, pt); });
    refused(d.name + ': customEdSignBatch on ' + bad, function() { eng.customEdSignBatch(bad, h1, 32, 0, one, one, false); });
    refused(d.name + ': customEdSignDetBatch on ' + bad, function() { eng.customEdSignDetBatch(bad, h1, 32, 0, one, 'sha256', false); });
  });
  refused(d.name + ': customSignBatch on the Edwards domain', function() { eng.customSignBatch(id, h1, 32, 0, one, one, false); });
  refused(d.name + ': customRecoverBatch on the Edwards domain', function() { eng.customRecoverBatch(id, h1, 32, one, one, Buffer.from([0])); });
  // the domain id is a plain Edwards id too
  var a = eng.mulBatch(id, one, pt), b = eng.mulBatch(plain, one, pt);
  if (!a.xy.equals(b.xy)) fail(d.name + ': mulBatch differs between the domain and the plain id');
  checked++;
});
Promise.all(pending).then(function() {
  eng.close();
  console.log(JSON.stringify({ ok: true, checked: checked, domains: golden.length }));
  process.exit(0);
}, function(e) { fail('async: ' + e.message); });
