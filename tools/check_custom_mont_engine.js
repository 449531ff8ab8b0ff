'use strict';
// User-defined Montgomery curves through the N-API addon: on every curve of
// tests/golden/custom_mont.json, Engine#customMontLadderBatch, customMontValidateBatch and
// customMontDeriveBatch and their Async forms equal the reference's recorded answers -- getX() and
// the Z == 0 flag, validate's answer or 'Assertion failed', derive's secret or the message it
// throws (where Z == 0 the reference returns 0 and the engine flags the item: inf 1 / status 2).
// One engine call per batch.  A Montgomery id is refused by the short-curve calls, and a short id
// by these.  The library is ELLGPU_LIB's (the CPU unit-test build) or the device's.  Prints one
// JSON line.
//
//   [ELLGPU_LIB=...] node tools/check_custom_mont_engine.js

var path = require('path');
var Engine = require('../elliptic_amd/js/index.js').Engine;
var golden = require(path.join(__dirname, '..', 'tests', 'golden', 'custom_mont.json'));

function b32(h) { var b = Buffer.alloc(32); var v = Buffer.from(h.length % 2 ? '0' + h : h, 'hex'); v.copy(b, 32 - v.length); return b; }
function fail(msg) { console.log(JSON.stringify({ ok: false, error: msg })); process.exit(1); }
function cat(vs, f) { return Buffer.concat(vs.map(f)); }
function row(buf, i) { return buf.slice(32 * i, 32 * i + 32).toString('hex'); }

var eng = new Engine();
var checked = 0;
var pending = [];
var ZERO = Buffer.alloc(32).toString('hex');
var DMSG = { 'public point not validated': 1, 'Assertion failed': 3 };

function vstatus(v) {
  if (v.valid !== undefined) return 1 - v.valid;
  if (v.vmsg !== 'Assertion failed') fail('unexpected validate message ' + v.vmsg);
  return 3;
}
function checkLadder(c, vs, res, what) {
  vs.forEach(function(v, i) {
    if (res.inf[i] !== v.z0 || row(res.x, i) !== v.getx)
      fail(c.name + ' ' + what + ' ' + v.tag + ' k ' + v.k + ' x ' + v.x + ': inf ' + res.inf[i] + ' x ' + row(res.x, i));
    checked++;
  });
}
function checkValidate(c, vs, res, what) {
  vs.forEach(function(v, i) {
    if (res.status[i] !== vstatus(v)) fail(c.name + ' ' + what + ' ' + v.tag + ' x ' + v.x + ': status ' + res.status[i]);
    checked++;
  });
}
function checkDerive(c, vs, res, what) {
  vs.forEach(function(v, i) {
    var st = v.derive === undefined ? DMSG[v.dmsg] : (v.z0 ? 2 : 0);
    if (st === undefined) fail('unexpected derive message ' + v.dmsg);
    var want = st === 0 ? v.derive : ZERO;
    if (res.status[i] !== st || row(res.x, i) !== want)
      fail(c.name + ' ' + what + ' ' + v.tag + ' k ' + v.k + ' x ' + v.x + ': status ' + res.status[i] + ', want ' + st);
    checked++;
  });
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

function pad(v) { return ('0'.repeat(64) + v.toString(16)).slice(-64); }
// a row of the toy curve (one x, lists over k = 0, 1, ...) -> cases of the common shape
function rowCases(r) {
  return r.z0.map(function(z0, k) {
    return { tag: 'exhaustive', k: pad(k), x: pad(r.x), z0: z0, getx: pad(r.getx[k]), valid: r.valid, vmsg: r.vmsg,
      dmsg: r.dmsg, derive: r.derive && pad(r.derive[k]) };
  });
}

golden.forEach(function(c) {
  if (c.rows) c.cases = [].concat.apply([], c.rows.map(rowCases));
  var id = eng.defineMont(b32(c.p), b32(c.a));
  if (eng.defineMont(b32(c.p), b32(c.a)) !== id) fail(c.name + ': the same parameters gave another id');
  var vs = c.cases;
  var ks = cat(vs, function(v) { return b32(v.k); }), xs = cat(vs, function(v) { return b32(v.x); });
  checkLadder(c, vs, once(function() { return eng.customMontLadderBatch(id, ks, xs); }), 'ladder');
  checkValidate(c, vs, once(function() { return eng.customMontValidateBatch(id, xs); }), 'validate');
  checkDerive(c, vs, once(function() { return eng.customMontDeriveBatch(id, ks, xs); }), 'derive');
  pending.push(eng.customMontLadderBatchAsync(id, ks, xs).then(function(res) { checkLadder(c, vs, res, 'ladderAsync'); }));
  pending.push(eng.customMontValidateBatchAsync(id, xs).then(function(res) { checkValidate(c, vs, res, 'validateAsync'); }));
  pending.push(eng.customMontDeriveBatchAsync(id, ks, xs).then(function(res) { checkDerive(c, vs, res, 'deriveAsync'); }));
  // four refusals per curve: the short-curve calls on the Montgomery id, these on a short id
  var one = ks.slice(0, 32), pt = Buffer.concat([xs.slice(0, 32), xs.slice(0, 32)]);
  refused(c.name + ': mulBatch on a Montgomery id', function() { eng.mulBatch(id, one, pt); });
  refused(c.name + ': customDeriveBatch on a Montgomery id', function() { eng.customDeriveBatch(id, one, pt); });
  var short = eng.defineShort(b32(c.p), b32(c.a), b32('07'));
  if (short === id) fail(c.name + ': a short curve shares the Montgomery id');
  refused(c.name + ': customMontLadderBatch on a short id', function() { eng.customMontLadderBatch(short, one, xs.slice(0, 32)); });
  refused(c.name + ': customMontDeriveBatch on the preset id', function() { eng.customMontDeriveBatch('curve25519', one, xs.slice(0, 32)); });
});
Promise.all(pending).then(function() {
  eng.close();
  console.log(JSON.stringify({ ok: true, checked: checked, curves: golden.length }));
  process.exit(0);
}, function(e) { fail('async: ' + e.message); });
