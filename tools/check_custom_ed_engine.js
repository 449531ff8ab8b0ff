'use strict';
// The key side of user-defined Edwards curves through the N-API addon: on every curve of
// tests/golden/custom_ed.json, Engine#customEdDecompressBatch, customEdDecodePointBatch,
// customEdValidateBatch (with the recorded n and without an order), customEdDeriveBatch,
// customEdDeriveWireBatch and customEdEncodePointBatch and their Async forms equal the reference's
// recorded answers -- the point or the message thrown, KeyPair#validate's reason, derive's secret.
// One engine call per batch (encodings are grouped by their length).  An Edwards id is refused by
// the short-curve and Montgomery calls, and a short id by these.  The library is ELLGPU_LIB's (the
// CPU unit-test build) or the device's.  Prints one JSON line.
//
//   [ELLGPU_LIB=...] node tools/check_custom_ed_engine.js

var path = require('path');
var Engine = require('../elliptic_amd/js/index.js').Engine;
var golden = require(path.join(__dirname, '..', 'tests', 'golden', 'custom_ed.json'));

function b32(h) { var b = Buffer.alloc(32); var v = Buffer.from(h.length % 2 ? '0' + h : h, 'hex'); v.copy(b, 32 - v.length); return b; }
function fail(msg) { console.log(JSON.stringify({ ok: false, error: msg })); process.exit(1); }
function cat(vs, f) { return Buffer.concat(vs.map(f)); }
function hexRow(buf, i, w) { return buf.slice(w * i, w * i + w).toString('hex'); }
function pad(v) { return ('0'.repeat(64) + v.toString(16)).slice(-64); }

var eng = new Engine();
var checked = 0;
var pending = [];
var ZERO = '0'.repeat(64);
var MSG = { 'Unknown point format': 1, 'invalid point': 2, 'Assertion failed': 3 };
var REASON = { 'Invalid public key': 1, 'Public key is not a point': 2, 'Public key * N != O': 3 };

function status(msg) {
  if (MSG[msg] === undefined) fail('unexpected message ' + msg);
  return MSG[msg];
}
// a point-valued case: xy or msg
function checkPoints(c, vs, res, what) {
  vs.forEach(function(v, i) {
    var st = v.xy === undefined ? status(v.msg) : 0;
    var want = st === 0 ? v.xy : ZERO + ZERO;
    if (res.status[i] !== st || hexRow(res.xy, i, 64) !== want)
      fail(c.name + ' ' + what + ' ' + v.tag + ' ' + (v.v || v.enc) + ': status ' + res.status[i] + ', want ' + st);
    checked++;
  });
}
function checkValidate(c, vs, res, what, noOrder) {
  vs.forEach(function(v, i) {
    var st = v.reason === null ? 0 : REASON[v.reason];
    if (st === undefined) fail('unexpected reason ' + v.reason);
    if ((st === 0) !== (v.result === 1)) fail('reason and result disagree');
    if (noOrder && st === 3) st = 0;
    if (res.status[i] !== st) fail(c.name + ' ' + what + ' ' + v.tag + ': status ' + res.status[i] + ', want ' + st);
    checked++;
  });
}
function checkDerive(c, vs, res, what) {
  vs.forEach(function(v, i) {
    var st, err = 0;
    if (v.dmsg !== undefined) { st = 3; err = status(v.dmsg); }
    else if (v.x !== undefined) st = v.z0 ? 2 : 0;
    else if (v.xmsg === 'public point not validated') st = 1;
    else fail('unexpected derive message ' + v.xmsg);
    var want = st === 0 ? v.x : ZERO;
    if (res.status[i] !== st || hexRow(res.x, i, 32) !== want || (res.err && res.err[i] !== err))
      fail(c.name + ' ' + what + ' ' + v.tag + ': status ' + res.status[i] + ', want ' + st);
    checked++;
  });
}
function checkEncode(c, vs, res, what, field, w) {
  vs.forEach(function(v, i) {
    if (hexRow(res.enc, i, w) !== v[field]) fail(c.name + ' ' + what + ' ' + v.tag + ': ' + hexRow(res.enc, i, w));
    checked++;
  });
  if (res.enc.length !== vs.length * w) fail(c.name + ' ' + what + ': result length');
}
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
function byLength(vs) {
  var g = {};
  vs.forEach(function(v) { (g[v.enc.length / 2] = g[v.enc.length / 2] || []).push(v); });
  return Object.keys(g).map(Number).sort(function(a, b) { return a - b; }).map(function(l) { return [l, g[l]]; });
}
// a row of a toy curve (one value, both parities, both coordinates) -> cases of the common shape
function toyCases(r) {
  var out = [];
  [['fromx', r.fx], ['fromy', r.fy]].forEach(function(f) {
    f[1].forEach(function(res, odd) {
      var c = { op: f[0], tag: 'exhaustive', v: pad(r.v), odd: odd };
      if (typeof res === 'string') c.msg = res; else c.xy = pad(res[0]) + pad(res[1]);
      out.push(c);
    });
  });
  return out;
}

// one short curve for the refusals (a context holds sixteen user-defined curves; the fixture has nine)
var short = eng.defineShort(b32(golden[0].p), b32('01'), b32('07'));
golden.forEach(function(c) {
  if (c.rows) c.cases = [].concat.apply([], c.rows.map(toyCases));
  var id = eng.defineEdwards(b32(c.p), b32(c.a), b32(c.d));
  if (eng.defineEdwards(b32(c.p), b32(c.a), b32(c.d)) !== id) fail(c.name + ': the same parameters gave another id');
  function of(op) { return c.cases.filter(function(v) { return v.op === op; }); }
  [['fromx', 0], ['fromy', 1]].forEach(function(f) {
    var vs = of(f[0]);
    var xs = cat(vs, function(v) { return b32(v.v); }), odds = Buffer.from(vs.map(function(v) { return v.odd ? 255 : 0; }));
    checkPoints(c, vs, once(function() { return eng.customEdDecompressBatch(id, xs, odds, f[1]); }), f[0]);
    pending.push(eng.customEdDecompressBatchAsync(id, xs, odds, f[1]).then(function(res) { checkPoints(c, vs, res, f[0] + 'Async'); }));
  });
  byLength(of('decode')).forEach(function(g) {
    var enc = cat(g[1], function(v) { return Buffer.from(v.enc, 'hex'); });
    checkPoints(c, g[1], once(function() { return eng.customEdDecodePointBatch(id, enc, g[0]); }), 'decode');
    pending.push(eng.customEdDecodePointBatchAsync(id, enc, g[0]).then(function(res) { checkPoints(c, g[1], res, 'decodeAsync'); }));
  });
  var vs = of('validate');
  if (vs.length) {
    var xy = cat(vs, function(v) { return Buffer.from(v.xy, 'hex'); }), n = b32(c.n);
    checkValidate(c, vs, once(function() { return eng.customEdValidateBatch(id, xy, n); }), 'validate', false);
    checkValidate(c, vs, once(function() { return eng.customEdValidateBatch(id, xy, null); }), 'validate without order', true);
    pending.push(eng.customEdValidateBatchAsync(id, xy, n).then(function(res) { checkValidate(c, vs, res, 'validateAsync', false); }));
    pending.push(eng.customEdValidateBatchAsync(id, xy).then(function(res) { checkValidate(c, vs, res, 'validateAsync without order', true); }));
  }
  var raw = of('derive').filter(function(v) { return v.xy !== undefined; });
  if (raw.length) {
    var ks = cat(raw, function(v) { return b32(v.priv); }), pub = cat(raw, function(v) { return Buffer.from(v.xy, 'hex'); });
    checkDerive(c, raw, once(function() { return eng.customEdDeriveBatch(id, ks, pub); }), 'derive');
    pending.push(eng.customEdDeriveBatchAsync(id, ks, pub).then(function(res) { checkDerive(c, raw, res, 'deriveAsync'); }));
  }
  byLength(of('derive').filter(function(v) { return v.enc !== undefined; })).forEach(function(g) {
    var ks = cat(g[1], function(v) { return b32(v.priv); }), enc = cat(g[1], function(v) { return Buffer.from(v.enc, 'hex'); });
    checkDerive(c, g[1], once(function() { return eng.customEdDeriveWireBatch(id, ks, enc, g[0]); }), 'deriveWire');
    pending.push(eng.customEdDeriveWireBatchAsync(id, ks, enc, g[0]).then(function(res) { checkDerive(c, g[1], res, 'deriveWireAsync'); }));
  });
  var es = of('encode');
  if (es.length) {
    var pts = cat(es, function(v) { return Buffer.from(v.xy, 'hex'); });
    [[true, 'compact', 1 + c.pl], [false, 'full', 1 + 2 * c.pl]].forEach(function(f) {
      checkEncode(c, es, once(function() { return eng.customEdEncodePointBatch(id, pts, f[0]); }), 'encode', f[1], f[2]);
      pending.push(eng.customEdEncodePointBatchAsync(id, pts, f[0], c.pl).then(function(res) { checkEncode(c, es, res, 'encodeAsync', f[1], f[2]); }));
    });
    refused(c.name + ': a coordBytes that is not PL', function() { eng.customEdEncodePointBatch(id, pts, true, c.pl === 32 ? 31 : c.pl + 1); });
  }
  // refusals: the short-curve and Montgomery calls on the Edwards id, these on a short and a preset id
  var one = b32('01'), x = b32('05'), pt = Buffer.concat([x, x]);
  refused(c.name + ': customDecompressBatch on an Edwards id', function() { eng.customDecompressBatch(id, x, Buffer.from([0])); });
  refused(c.name + ': customDeriveBatch on an Edwards id', function() { eng.customDeriveBatch(id, one, pt); });
  refused(c.name + ': customMontLadderBatch on an Edwards id', function() { eng.customMontLadderBatch(id, one, x); });
  refused(c.name + ': customEncodePointBatch on an Edwards id', function() { eng.customEncodePointBatch(id, pt, true); });
  if (short === id) fail(c.name + ': a short curve shares the Edwards id');
  refused(c.name + ': customEdDeriveBatch on a short id', function() { eng.customEdDeriveBatch(short, one, pt); });
  refused(c.name + ': customEdEncodePointBatch on a short id', function() { eng.customEdEncodePointBatch(short, pt, true); });
  refused(c.name + ': customEdDecompressBatch on the preset id', function() { eng.customEdDecompressBatch('ed25519', x, Buffer.from([0]), 1); });
});
Promise.all(pending).then(function() {
  eng.close();
  console.log(JSON.stringify({ ok: true, checked: checked, curves: golden.length }));
  process.exit(0);
}, function(e) { fail('async: ' + e.message); });
