'use strict';
// Fixed-base tables of caller-chosen points on Edwards curves through the N-API addon: on every curve
// of tests/golden/fixed_base_ed.json, Engine#defineEdBase, baseInfo, mulBaseBatch, mulBase2Batch,
// their Async forms and releaseBase give the reference's recorded answers (a digest per answer: the
// first 8 bytes of SHA-256(inf || x || y), the identity as inf = 1 beside (0, 1) -- a user-defined id
// writes inf = 0 there, so the byte is taken from the coordinates).  Bases 0, 2, 3 and 5 of each
// curve (G, -G, the PRNG point, the point of order 2) and the recorded pairs among them: a table
// costs the CPU unit-test build seconds.  One engine call per batch.  The library is ELLGPU_LIB's (the
// CPU unit-test build) or the device's.  Prints one JSON line.
//
//   [ELLGPU_LIB=...] node tools/check_fixed_base_ed_engine.js

var path = require('path');
var crypto = require('crypto');
var Engine = require('../elliptic_amd/js/index.js').Engine;
var golden = require(path.join(__dirname, '..', 'tests', 'golden', 'fixed_base_ed.json'));
var B = 32;
var BASES = [0, 2, 3, 5];

function fail(msg) { console.log(JSON.stringify({ ok: false, error: msg })); process.exit(1); }
function wide(h) { var b = Buffer.alloc(B); var v = Buffer.from(h.length % 2 ? '0' + h : h, 'hex'); v.copy(b, B - v.length); return b; }
function point(xy) { return Buffer.concat([wide(xy[0]), wide(xy[1])]); }
var ID = point(['0', '1']);
function digest(res, i) {
  var xy = res.xy.slice(2 * B * i, 2 * B * (i + 1));
  var buf = Buffer.concat([Buffer.from([xy.equals(ID) ? 1 : 0]), xy]);
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
  if (res.xy.length !== n * 2 * B || res.inf.length !== n) fail(c.name + ' ' + what + ': result of ' + res.xy.length + ' bytes for ' + n + ' items');
  for (var i = 0; i < n; i++) {
    var id = res.xy.slice(2 * B * i, 2 * B * (i + 1)).equals(ID);
    if (res.inf[i] !== (c.kind === 'preset' && id ? 1 : 0)) fail(c.name + ' ' + what + ' item ' + i + ': inf ' + res.inf[i]);
    if (digest(res, i) !== want[i]) fail(c.name + ' ' + what + ' item ' + i + ': xy ' + res.xy.slice(2 * B * i, 2 * B * (i + 1)).toString('hex'));
    checked++;
  }
}
function throws(f, needle) {
  try { f(); } catch (e) { if (String(e.message).indexOf(needle) < 0) fail('unexpected message: ' + e.message); refused++; return; }
  fail('no refusal where "' + needle + '" was expected');
}

function runCurve(c) {
  var pending = [];
  var curve = c.name;
  if (c.kind === 'domain') curve = eng.defineEdwardsDomain(wide(c.p), wide(c.a), wide(c.d), wide(c.n), wide(c.g[0]), wide(c.g[1]));
  else if (c.kind === 'plain') curve = eng.defineEdwards(wide(c.p), wide(c.a), wide(c.d));
  var hs = {};
  BASES.forEach(function(bi) { hs[bi] = eng.defineEdBase(curve, point(c.bases[bi]), 0); });
  if (eng.defineEdBase(curve, point(c.bases[0]), 0) !== hs[0]) fail(c.name + ': the same base twice gave two handles');
  if (c.kind !== 'plain' && c.kind !== 'preset' && eng.defineEdBase(curve, null, 0) !== hs[0]) fail(c.name + ': the domain\'s generator is another handle');
  var info = eng.baseInfo(hs[3]);
  if (!(info.windowBits === 8 || info.windowBits === 16) || !(info.tableBytes > 0) || eng.addon.fieldBytes(info.curve) !== B) fail(c.name + ': baseInfo ' + JSON.stringify(info));
  var ks = Buffer.concat(c.k.map(wide));
  BASES.forEach(function(bi) {
    var h = hs[bi];
    check(c, once(function() { return eng.mulBaseBatch(h, ks); }), c.mul[bi], c.k.length, 'mulBaseBatch base ' + bi);
    pending.push(eng.mulBaseBatchAsync(h, ks).then(function(res) { check(c, res, c.mul[bi], c.k.length, 'mulBaseBatchAsync base ' + bi); }));
  });
  var groups = {};
  c.pairs.forEach(function(p) {
    if (BASES.indexOf(p[0]) < 0 || BASES.indexOf(p[1]) < 0) return;
    var key = p[0] + ':' + p[1]; (groups[key] = groups[key] || []).push(p);
  });
  Object.keys(groups).forEach(function(key) {
    var ps = groups[key], b1 = hs[ps[0][0]], b2 = hs[ps[0][1]];
    var k1 = Buffer.concat(ps.map(function(p) { return wide(p[2]); }));
    var k2 = Buffer.concat(ps.map(function(p) { return wide(p[3]); }));
    var want = ps.map(function(p) { return p[4]; });
    check(c, once(function() { return eng.mulBase2Batch(b1, b2, k1, k2); }), want, ps.length, 'mulBase2Batch ' + key);
    pending.push(eng.mulBase2BatchAsync(b1, b2, k1, k2).then(function(res) { check(c, res, want, ps.length, 'mulBase2BatchAsync ' + key); }));
  });
  throws(function() { eng.defineEdBase(curve, Buffer.alloc(2 * B), 0); }, 'not a point of the curve');
  throws(function() { eng.defineEdBase(curve, point(c.bases[0]), 5); }, 'window_bits');
  throws(function() { eng.defineBase(curve, point(c.bases[0]), 0); }, 'short Weierstrass');
  throws(function() { eng.mulBaseBatch(hs[0], Buffer.alloc(B + 1)); }, 'buffer length mismatch');
  return Promise.all(pending).then(function() {
    BASES.forEach(function(bi) { eng.releaseBase(hs[bi]); });
    throws(function() { eng.baseInfo(hs[0]); }, 'unknown base handle');
  });
}

golden.reduce(function(p, c) { return p.then(function() { return runCurve(c); }); }, Promise.resolve()).then(function() {
  throws(function() { eng.defineEdBase('secp256k1', Buffer.alloc(2 * B), 0); }, 'ellgpu_base_define');
  eng.close();
  console.log(JSON.stringify({ ok: true, checked: checked, refused: refused, curves: golden.length }));
}).catch(function(e) { fail(String(e && e.stack || e)); });
