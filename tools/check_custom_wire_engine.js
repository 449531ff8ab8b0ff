'use strict';
// The wire formats on user-defined short curves through the N-API addon: on every curve of
// tests/golden/custom_wire.json, Engine#customDecodePointBatch and #customDecompressBatch equal the
// reference's recorded decodePoint / pointFromX answers (status and coordinates), and on every
// domain Engine#customVerifyWireBatch and its Async form equal the recorded EC#verify(msg, der, key)
// verdicts -- a thrown message is its err code with verdict 0, an off-curve uncompressed key is
// verdict 0 / err 5.  One engine call per batch.  The library is ELLGPU_LIB's (the CPU unit-test
// build) or the device's.  Prints one JSON line.
//
//   [ELLGPU_LIB=...] node tools/check_custom_wire_engine.js

var path = require('path');
var Engine = require('../elliptic_amd/js/index.js').Engine;
var golden = require(path.join(__dirname, '..', 'tests', 'golden', 'custom_wire.json'));

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

function checkPoint(c, d, xy, st, i, what) {
  var want = d.st === 0 ? d.x + d.y : Buffer.alloc(64).toString('hex');
  if (st[i] !== d.st || xy.slice(64 * i, 64 * i + 64).toString('hex') !== want)
    fail(c.name + ' ' + what + ' ' + d.tag + ' ' + d.enc + ': status ' + st[i] + ', want ' + d.st);
  checked++;
}
function checkWire(c, vs, res, what) {
  vs.forEach(function(v, i) {
    var want = v.msg ? [0, Engine.WIRE_ERROR.indexOf(v.msg)] : v.tag === 'key_off_curve' ? [0, 5] : [v.ok, 0];
    if (want[1] < 0) fail(c.name + ': unknown message ' + v.msg);
    if (res.ok[i] !== want[0] || res.err[i] !== want[1])
      fail(c.name + ' ' + what + ' ' + v.tag + ': got ' + res.ok[i] + '/' + res.err[i] + ', want ' + want.join('/'));
    checked++;
  });
}

golden.forEach(function(c) {
  var id = c.n ? eng.defineShortDomain(b32(c.p), b32(c.a), b32(c.b), b32(c.n), b32(c.g.x), b32(c.g.y))
    : eng.defineShort(b32(c.p), b32(c.a), b32(c.b));
  var again = c.n ? eng.defineShortDomain(b32(c.p), b32(c.a), b32(c.b), b32(c.n), b32(c.g.x), b32(c.g.y))
    : eng.defineShort(b32(c.p), b32(c.a), b32(c.b));
  if (again !== id) fail(c.name + ': a second definition gave another id');
  groupBy(c.decode, function(d) { return String(d.enc.length / 2 + 1000); }).forEach(function(ds) {
    var encLen = ds[0].enc.length / 2;
    var calls = eng.stats.gpuCalls;
    var r = eng.customDecodePointBatch(id, Buffer.concat(ds.map(function(d) { return hex(d.enc); })), encLen);
    if (eng.stats.gpuCalls !== calls + 1) fail('not one engine call per batch');
    ds.forEach(function(d, i) { checkPoint(c, d, r.xy, r.status, i, 'decodePoint'); });
  });
  var comp = c.decode.filter(function(d) {
    return d.enc.length / 2 === 1 + c.pl && (d.enc.slice(0, 2) === '02' || d.enc.slice(0, 2) === '03');
  });
  var r = eng.customDecompressBatch(id, Buffer.concat(comp.map(function(d) { return b32(d.enc.slice(2)); })),
    Buffer.from(comp.map(function(d) { return d.enc.slice(0, 2) === '03' ? 1 : 0; })));
  comp.forEach(function(d, i) { checkPoint(c, d, r.xy, r.status, i, 'pointFromX'); });
  if (!c.wire) {
    // a plain curve has no ECDSA domain: the verify is refused
    try {
      eng.customVerifyWireBatch(id, { hashes: Buffer.alloc(32), hashLen: 32, sigs: [hex('3006020101020101')],
        keys: Buffer.alloc(1 + c.pl), keyLen: 1 + c.pl });
    } catch (e) { checked++; return; }
    fail(c.name + ': customVerifyWireBatch accepted a plain curve id');
  }
  groupBy(c.wire, function(v) { return [v.h.length / 2, v.bits, v.key.length / 2].join(':'); }).forEach(function(vs) {
    var o = { hashes: Buffer.concat(vs.map(function(v) { return hex(v.h); })), hashLen: vs[0].h.length / 2,
      msgBits: vs[0].bits, sigs: vs.map(function(v) { return hex(v.der); }),
      keys: Buffer.concat(vs.map(function(v) { return hex(v.key); })), keyLen: vs[0].key.length / 2 };
    var calls = eng.stats.gpuCalls;
    checkWire(c, vs, eng.customVerifyWireBatch(id, o), 'verify');
    if (eng.stats.gpuCalls !== calls + 1) fail('not one engine call per batch');
    pending.push(eng.customVerifyWireBatchAsync(id, o).then(function(res) { checkWire(c, vs, res, 'verifyAsync'); }));
  });
});
Promise.all(pending).then(function() {
  eng.close();
  console.log(JSON.stringify({ ok: true, checked: checked, curves: golden.length }));
  process.exit(0);
}, function(e) { fail('async: ' + e.message); });
