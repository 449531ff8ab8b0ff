'use strict';
// ECDSA verification against a fixed-base table of the signer's key through the N-API addon: on
// every curve of tests/golden/verify_base.json, Engine#ecdsaVerifyBaseBatch and its Async form give
// the reference's recorded verdicts for every key (a handle of Engine#defineBase; the key d = 1 also
// as the generator alias), strictly 0 / 1, one engine call per batch.  The library is ELLGPU_LIB's
// (the CPU unit-test build) or the device's.  Prints one JSON line.
//
//   [ELLGPU_LIB=...] node tools/check_verify_base_engine.js

var path = require('path');
var Engine = require('../elliptic_amd/js/index.js').Engine;
var golden = require(path.join(__dirname, '..', 'tests', 'golden', 'verify_base.json'));

function fail(msg) { console.log(JSON.stringify({ ok: false, error: msg })); process.exit(1); }
function wide(h, B) { var b = Buffer.alloc(B); var v = Buffer.from(h.length % 2 ? '0' + h : h, 'hex'); v.copy(b, B - v.length); return b; }

var eng = new Engine();
var checked = 0, refused = 0;

function once(f) {
  var calls = eng.stats.gpuCalls;
  var r = f();
  if (eng.stats.gpuCalls !== calls + 1) fail('not one engine call per batch');
  return r;
}
function check(c, res, want, what) {
  if (Object.keys(res).join() !== 'ok' || res.ok.length !== want.length) fail(c.name + ' ' + what + ': result ' + Object.keys(res).join() + ' of ' + res.ok.length + ' bytes for ' + want.length + ' items');
  for (var i = 0; i < want.length; i++) {
    if (res.ok[i] !== want[i]) fail(c.name + ' ' + what + ' item ' + i + ': verdict ' + res.ok[i] + ', the reference says ' + want[i]);
    checked++;
  }
}
function throws(f, needle) {
  try { f(); } catch (e) { if (String(e.message).indexOf(needle) < 0) fail('unexpected message: ' + e.message); refused++; return; }
  fail('no refusal where "' + needle + '" was expected');
}

function runCurve(c) {
  var pending = [];
  var B = c.B;
  var curve = c.name;
  if (c.p !== undefined) curve = eng.defineShortDomain(wide(c.p, 32), wide(c.a, 32), wide(c.b, 32), wide(c.n, 32), wide(c.g[0], 32), wide(c.g[1], 32));
  var hs = c.keys.map(function(k) { return eng.defineBase(curve, Buffer.concat([wide(k[1], B), wide(k[2], B)]), 0); });
  var alias = eng.defineBase(curve, null, 0);
  function runKey(h, cases, what) {
    var groups = {};
    cases.forEach(function(cs) { var key = cs[1].length / 2 + ':' + cs[2]; (groups[key] = groups[key] || []).push(cs); });
    Object.keys(groups).forEach(function(key) {
      var g = groups[key];
      var b = { hashes: Buffer.concat(g.map(function(cs) { return Buffer.from(cs[1], 'hex'); })), hashLen: g[0][1].length / 2,
        msgBits: g[0][2], r: Buffer.concat(g.map(function(cs) { return wide(cs[3], B); })),
        s: Buffer.concat(g.map(function(cs) { return wide(cs[4], B); })) };
      var want = g.map(function(cs) { return cs[5]; });
      check(c, once(function() { return eng.ecdsaVerifyBaseBatch(h, b); }), want, 'ecdsaVerifyBaseBatch ' + what + ' ' + key);
      pending.push(eng.ecdsaVerifyBaseBatchAsync(h, b).then(function(res) { check(c, res, want, 'ecdsaVerifyBaseBatchAsync ' + what + ' ' + key); }));
    });
  }
  hs.forEach(function(h, ki) { runKey(h, c.cases[ki], 'key ' + ki); });
  runKey(alias, c.cases[0], 'alias');
  var one = { hashes: Buffer.alloc(32), hashLen: 32, msgBits: 0, r: wide('1', B), s: wide('1', B) };
  throws(function() { eng.ecdsaVerifyBaseBatch(hs[0], { hashes: one.hashes, hashLen: 32, msgBits: 0, r: Buffer.alloc(B + 1), s: one.s }); }, 'buffer length mismatch');
  throws(function() { eng.ecdsaVerifyBaseBatch(hs[0], { hashes: Buffer.alloc(72), hashLen: 72, msgBits: 1, r: one.r, s: one.s }); }, 'more bits than the order width');
  throws(function() { eng.ecdsaVerifyBaseBatch(12345, one); }, 'unknown base handle');
  // the handles are released once the Promise forms have run
  return Promise.all(pending).then(function() {
    hs.concat([alias]).forEach(function(h) { eng.releaseBase(h); });
    throws(function() { eng.ecdsaVerifyBaseBatch(hs[0], one); }, 'unknown base handle');
    return eng.ecdsaVerifyBaseBatchAsync(hs[0], one).then(function() { fail('a released handle was accepted'); },
      function(e) { if (String(e.message).indexOf('unknown base handle') < 0) fail('unexpected message: ' + e.message); refused++; });
  });
}

golden.reduce(function(p, c) { return p.then(function() { return runCurve(c); }); }, Promise.resolve()).then(function() {
  // an Edwards handle is refused
  var ed = eng.defineEdBase('ed25519', null, 0);
  throws(function() { eng.ecdsaVerifyBaseBatch(ed, { hashes: Buffer.alloc(32), hashLen: 32, msgBits: 0, r: wide('1', 32), s: wide('1', 32) }); }, 'short Weierstrass');
  eng.releaseBase(ed);
  eng.close();
  console.log(JSON.stringify({ ok: true, checked: checked, refused: refused, curves: golden.length }));
}).catch(function(e) { fail(String(e && e.stack || e)); });
