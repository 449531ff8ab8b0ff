'use strict';
// EdDSA verification against a fixed-base table of the signer's key through the N-API addon: for
// every key of tests/golden/eddsa_verify_base.json (a handle of Engine#defineEdBase on ed25519; the
// key G also as the generator alias) Engine#eddsaVerifyBaseBatch and its Async form give the
// reference's recorded verdicts -- ok strictly 0 / 1, err = 1 where the reference throws -- one engine
// call per batch, the mixed message lengths of a key in one call.  The library is ELLGPU_LIB's (the
// CPU unit-test build) or the device's.  Prints one JSON line.
//
//   [ELLGPU_LIB=...] node tools/check_eddsa_verify_base_engine.js

var path = require('path');
var Engine = require('../elliptic_amd/js/index.js').Engine;
var golden = require(path.join(__dirname, '..', 'tests', 'golden', 'eddsa_verify_base.json'));

function fail(msg) { console.log(JSON.stringify({ ok: false, error: msg })); process.exit(1); }
function wide(h) { var b = Buffer.alloc(32); var v = Buffer.from(h.length % 2 ? '0' + h : h, 'hex'); v.copy(b, 32 - v.length); return b; }

var eng = new Engine();
var checked = 0, refused = 0;

function once(f) {
  var calls = eng.stats.gpuCalls;
  var r = f();
  if (eng.stats.gpuCalls !== calls + 1) fail('not one engine call per batch');
  return r;
}
function check(res, cases, what) {
  if (Object.keys(res).join() !== 'ok,err' || res.ok.length !== cases.length || res.err.length !== cases.length)
    fail(what + ': result ' + Object.keys(res).join() + ' of ' + res.ok.length + ' bytes for ' + cases.length + ' items');
  cases.forEach(function(cs, i) {
    var thrown = typeof cs[3] === 'string';
    var ok = thrown ? 0 : cs[3], err = thrown ? 1 : 0;
    if (res.ok[i] !== ok || res.err[i] !== err)
      fail(what + ' ' + cs[0] + ': (ok, err) = (' + res.ok[i] + ', ' + res.err[i] + '), the reference says ' + cs[3]);
    checked++;
  });
}
function throws(f, needle) {
  try { f(); } catch (e) { if (String(e.message).indexOf(needle) < 0) fail('unexpected message: ' + e.message); refused++; return; }
  fail('no refusal where "' + needle + '" was expected');
}

var pending = [];
var hs = golden.keys.map(function(k) { return eng.defineEdBase('ed25519', Buffer.concat([wide(k.x), wide(k.y)]), 0); });
var alias = eng.defineEdBase('ed25519', null, 0);
function runKey(h, cases, what) {
  var msgs = cases.map(function(cs) { return Buffer.from(cs[1], 'hex'); });
  var sigs = Buffer.concat(cases.map(function(cs) { return Buffer.from(cs[2], 'hex'); }));
  check(once(function() { return eng.eddsaVerifyBaseBatch(h, msgs, sigs); }), cases, 'eddsaVerifyBaseBatch ' + what);
  pending.push(eng.eddsaVerifyBaseBatchAsync(h, msgs, sigs).then(function(res) { check(res, cases, 'eddsaVerifyBaseBatchAsync ' + what); }));
}
hs.forEach(function(h, ki) { runKey(h, golden.cases[ki], golden.keys[ki].name); });
runKey(alias, golden.cases[0], 'alias');

var oneMsg = [Buffer.from('abc')], oneSig = Buffer.alloc(64);
throws(function() { eng.eddsaVerifyBaseBatch(hs[0], oneMsg, Buffer.alloc(63)); }, 'buffer length mismatch');
throws(function() { eng.eddsaVerifyBaseBatch(12345, oneMsg, oneSig); }, 'unknown base handle');
var sh = eng.defineBase('p256', null, 0);
throws(function() { eng.eddsaVerifyBaseBatch(sh, oneMsg, oneSig); }, 'ellgpu_ed_base_define');
eng.releaseBase(sh);

Promise.all(pending).then(function() {
  hs.concat([alias]).forEach(function(h) { eng.releaseBase(h); });
  throws(function() { eng.eddsaVerifyBaseBatch(hs[0], oneMsg, oneSig); }, 'unknown base handle');
  return eng.eddsaVerifyBaseBatchAsync(hs[0], oneMsg, oneSig).then(function() { fail('a released handle was accepted'); },
    function(e) { if (String(e.message).indexOf('unknown base handle') < 0) fail('unexpected message: ' + e.message); refused++; });
}).then(function() {
  eng.close();
  console.log(JSON.stringify({ ok: true, checked: checked, refused: refused, keys: golden.keys.length }));
}).catch(function(e) { fail(String(e && e.stack || e)); });
