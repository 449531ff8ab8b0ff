'use strict';
// Engine#defineShortDomain through the N-API addon: on every domain of
// tests/golden/custom_ecdsa.json, ecdsaVerifyBatch equals the reference's recorded EC#verify
// verdicts (off-curve keys: verdict 0 with status 2; digests that leave more than 256 bits after
// truncation: refused, as on the presets), mulBatch(id, k, null) equals k*G and
// mulAddBatch(id, k1, null, k2, Q) equals k1*G + k2*Q -- one engine call per batch.  The library is
// ELLGPU_LIB's (the CPU unit-test build) or the device's.  Prints one JSON line.
//
//   [ELLGPU_LIB=...] node tools/check_custom_domain_engine.js

var path = require('path');
var Engine = require('../elliptic_amd/js/index.js').Engine;
var golden = require(path.join(__dirname, '..', 'tests', 'golden', 'custom_ecdsa.json'));

function hex(h) { return Buffer.from(h, 'hex'); }
function b32(h) { var b = Buffer.alloc(32); var v = hex(h.length % 2 ? '0' + h : h); v.copy(b, 32 - v.length); return b; }
function fail(msg) { console.log(JSON.stringify({ ok: false, error: msg })); process.exit(1); }

var eng = new Engine();
var checked = 0, refused = 0;
golden.forEach(function(c) {
  var id = eng.defineShortDomain(b32(c.p), b32(c.a), b32(c.b), b32(c.n), b32(c.g.x), b32(c.g.y));
  if (eng.defineShortDomain(b32(c.p), b32(c.a), b32(c.b), b32(c.n), b32(c.g.x), b32(c.g.y)) !== id)
    fail(c.name + ': a second definition gave another id');
  var nbits = BigInt('0x' + c.n).toString(2).length;
  var groups = {};
  c.verify.forEach(function(v) {
    var key = (v.h.length / 2) + ':' + v.bits;
    (groups[key] = groups[key] || []).push(v);
  });
  Object.keys(groups).forEach(function(key) {
    var vs = groups[key];
    var hl = vs[0].h.length / 2, bits = vs[0].bits;
    var o = { hashes: Buffer.concat(vs.map(function(v) { return hex(v.h); })), hashLen: hl, msgBits: bits,
      r: Buffer.concat(vs.map(function(v) { return b32(v.r); })),
      s: Buffer.concat(vs.map(function(v) { return b32(v.s); })),
      pub: Buffer.concat(vs.map(function(v) { return Buffer.concat([b32(v.q.x), b32(v.q.y)]); })),
      status: Buffer.alloc(vs.length) };
    var calls = eng.stats.gpuCalls;
    var wide = 8 * hl - Math.max(0, (bits || 8 * hl) - nbits) > 256;
    var ok;
    try {
      ok = eng.ecdsaVerifyBatch(id, o);
    } catch (e) {
      if (!wide) fail(c.name + ': ' + e.message);
      refused += vs.length;
      return;
    }
    if (wide) fail(c.name + ': a digest wider than 256 bits after truncation was accepted');
    if (eng.stats.gpuCalls !== calls + 1) fail('not one engine call per batch');
    vs.forEach(function(v, i) {
      var want = v.tag === 'off_curve' ? [0, 2] : [v.ok, 0];
      if (ok[i] !== want[0] || o.status[i] !== want[1])
        fail(c.name + ' ' + v.tag + ': got ' + ok[i] + '/' + o.status[i] + ', want ' + want.join('/'));
      checked++;
    });
  });
  function same(xy, inf, i, want, what) {
    if (want.inf) { if (inf[i] !== 1) fail(c.name + ' ' + what + ': want infinity'); return; }
    if (inf[i] !== 0 || xy.slice(64 * i, 64 * i + 32).toString('hex') !== want.x ||
        xy.slice(64 * i + 32, 64 * i + 64).toString('hex') !== want.y) fail(c.name + ' ' + what + ' differs');
    checked++;
  }
  var r = eng.mulBatch(id, Buffer.concat(c.mulg.map(function(m) { return b32(m.k); })), null);
  c.mulg.forEach(function(m, i) { same(r.xy, r.inf, i, m.r, 'k*G'); });
  r = eng.mulAddBatch(id, Buffer.concat(c.muladd.map(function(m) { return b32(m.k1); })), null,
    Buffer.concat(c.muladd.map(function(m) { return b32(m.k2); })),
    Buffer.concat(c.muladd.map(function(m) { return Buffer.concat([b32(m.q.x), b32(m.q.y)]); })));
  c.muladd.forEach(function(m, i) { same(r.xy, r.inf, i, m.r, 'mulAdd(G)'); });
});
eng.close();
console.log(JSON.stringify({ ok: true, checked: checked, refused: refused, curves: golden.length }));
process.exit(0);
