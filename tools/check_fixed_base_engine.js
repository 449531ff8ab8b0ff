'use strict';
// Fixed-base tables of caller-chosen points through the N-API addon: on every curve of
// tests/golden/fixed_base.json, Engine#defineBase, baseInfo, mulBaseBatch, mulBase2Batch, their
// Async forms and releaseBase give the reference's recorded answers (a digest per answer: the
// first 8 bytes of SHA-256(inf || x || y)).  The result's size follows the curve's width.  One
// engine call per batch.  The library is ELLGPU_LIB's (the CPU unit-test build) or the device's.
// Prints one JSON line.
//
//   [ELLGPU_LIB=...] node tools/check_fixed_base_engine.js

var path = require('path');
var crypto = require('crypto');
var Engine = require('../elliptic_amd/js/index.js').Engine;
var golden = require(path.join(__dirname, '..', 'tests', 'golden', 'fixed_base.json'));

function fail(msg) { console.log(JSON.stringify({ ok: false, error: msg })); process.exit(1); }
function wide(h, B) { var b = Buffer.alloc(B); var v = Buffer.from(h.length % 2 ? '0' + h : h, 'hex'); v.copy(b, B - v.length); return b; }
function digest(res, i, B) {
  var buf = Buffer.concat([Buffer.from([res.inf[i]]), res.xy.slice(2 * B * i, 2 * B * (i + 1))]);
  return crypto.createHash('sha256').update(buf).digest('hex').slice(0, 16);
}

var eng = new Engine();
var checked = 0, refused = 0;

function once(f) {
  var calls = eng.stats.gpuCalls;
  var r = f();
  if (eng.stats.gpuCalls !== calls + 1) fail('not one engine call per batch');
  return r;
}
function check(c, res, want, n, what) {
  if (res.xy.length !== n * 2 * c.B || res.inf.length !== n) fail(c.name + ' ' + what + ': result of ' + res.xy.length + ' bytes for ' + n + ' items of width ' + c.B);
  for (var i = 0; i < n; i++) {
    if (digest(res, i, c.B) !== want[i]) fail(c.name + ' ' + what + ' item ' + i + ': inf ' + res.inf[i] + ' xy ' + res.xy.slice(2 * c.B * i, 2 * c.B * (i + 1)).toString('hex'));
    checked++;
  }
}
function throws(f, needle) {
  try { f(); } catch (e) { if (String(e.message).indexOf(needle) < 0) fail('unexpected message: ' + e.message); refused++; return; }
  fail('no refusal where "' + needle + '" was expected');
}

// one curve at a time: at most 16 bases are live
function runCurve(c) {
  var pending = [];
  var B = c.B;
  var curve = c.name;
  if (c.p !== undefined) {
    curve = c.domain ? eng.defineShortDomain(wide(c.p, 32), wide(c.a, 32), wide(c.b, 32), wide(c.n, 32), wide(c.g[0], 32), wide(c.g[1], 32))
                     : eng.defineShort(wide(c.p, 32), wide(c.a, 32), wide(c.b, 32));
  }
  var width = (c.name === 'secp256k1' || c.name === 'p256') ? 8 : 0;
  var hs = c.bases.map(function(xy) { return eng.defineBase(curve, Buffer.concat([wide(xy[0], B), wide(xy[1], B)]), width); });
  if (eng.defineBase(curve, Buffer.concat([wide(c.bases[0][0], B), wide(c.bases[0][1], B)]), width) !== hs[0]) fail(c.name + ': the same base twice gave two handles');
  var info = eng.baseInfo(hs[3]);
  if (info.windowBits !== 8 || !(info.tableBytes > 0) || eng.addon.fieldBytes(info.curve) !== B) fail(c.name + ': baseInfo ' + JSON.stringify(info));
  var ks = Buffer.concat(c.k.map(function(k) { return wide(k, B); }));
  hs.forEach(function(h, bi) {
    check(c, once(function() { return eng.mulBaseBatch(h, ks); }), c.mul[bi], c.k.length, 'mulBaseBatch base ' + bi);
    pending.push(eng.mulBaseBatchAsync(h, ks).then(function(res) { check(c, res, c.mul[bi], c.k.length, 'mulBaseBatchAsync base ' + bi); }));
  });
  var groups = {};
  c.pairs.forEach(function(p) { var key = p[0] + ':' + p[1]; (groups[key] = groups[key] || []).push(p); });
  Object.keys(groups).forEach(function(key) {
    var ps = groups[key], b1 = hs[ps[0][0]], b2 = hs[ps[0][1]];
    var k1 = Buffer.concat(ps.map(function(p) { return wide(p[2], B); }));
    var k2 = Buffer.concat(ps.map(function(p) { return wide(p[3], B); }));
    var want = ps.map(function(p) { return p[4]; });
    check(c, once(function() { return eng.mulBase2Batch(b1, b2, k1, k2); }), want, ps.length, 'mulBase2Batch ' + key);
    pending.push(eng.mulBase2BatchAsync(b1, b2, k1, k2).then(function(res) { check(c, res, want, ps.length, 'mulBase2BatchAsync ' + key); }));
  });
  throws(function() { eng.defineBase(curve, Buffer.alloc(2 * B), 0); }, 'not a point of the curve');
  throws(function() { eng.defineBase(curve, Buffer.concat([wide(c.bases[0][0], B), wide(c.bases[0][1], B)]), 5); }, 'window_bits');
  throws(function() { eng.mulBaseBatch(hs[0], Buffer.alloc(B + 1)); }, 'buffer length mismatch');
  (c.refused || []).forEach(function(xy) {
    throws(function() { eng.defineBase(curve, Buffer.concat([wide(xy[0], 32), wide(xy[1], 32)]), 0); }, 'point at infinity');
  });
  // the handles are released once the Promise forms have run
  return Promise.all(pending).then(function() {
    hs.forEach(function(h) { eng.releaseBase(h); });
    throws(function() { eng.baseInfo(hs[0]); }, 'unknown base handle');
  });
}

golden.reduce(function(p, c) { return p.then(function() { return runCurve(c); }); }, Promise.resolve()).then(function() {
  eng.close();
  console.log(JSON.stringify({ ok: true, checked: checked, refused: refused, curves: golden.length }));
}).catch(function(e) { fail(String(e && e.stack || e)); });
