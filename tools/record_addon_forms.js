'use strict';
// Records tests/golden/addon_forms.json: what the N-API addon (elliptic_amd/js/ellgpu_napi.c) answers,
// form by form, for every export that takes operand Buffers -- talking to the addon directly
// (require of ellgpu.node, open(path)), not through Engine:
//   - one valid call of two items (where an operand may be null, or a flag picks another row kind, one
//     call of each kind): the result's property names in order, each result Buffer's length and hex;
//   - the same call through callAsync where the operation has an id: the Promise's value, pinned the
//     same way (tests/test_addon_forms.py asserts that it equals the synchronous one);
//   - mulFixed / mulVar / mulAdd2 once more with caller-supplied trailing (xy, inf) result Buffers;
//   - the refusals, with the exact message thrown: every operand Buffer one byte too long, every
//     operand Buffer passed as null, too few arguments, the non-positive hashLen / encLen / stride /
//     keyLen / coordBytes that have a check, an op out of range for callAsync -- in both forms.  A
//     changed call that is NOT refused (a null operand that is optional, a longer message buffer) is
//     pinned by its names, lengths and a SHA-256 of its bytes.
// Operands come from the goldens this repository has (tests/golden/captured_*.json, custom_*.json,
// fixed_base.json, eddsa_verify_base.json): preset secp256k1, ed25519, curve25519; one user-defined
// short domain, one Edwards domain, one Montgomery curve.  Every operation is deterministic in them.
//
// The fixture pins the addon as it stood when every operation was written out by hand in up to five
// places; tests/test_addon_forms.py compares the addon under test (one descriptor per operation)
// with it.  So run this in a checkout of the commit whose addon is to be kept, against the CPU
// unit-test build of the library (tests/hostsim/build.py) -- never to make a failing test pass.
//
//   ELLGPU_LIB=tests/hostsim/_build/libellgpu_hostsim.so node tools/record_addon_forms.js            (records)
//   [ELLGPU_LIB=...] node tools/record_addon_forms.js --compare     (prints one JSON line; exit 1 on a difference)

var crypto = require('crypto');
var fs = require('fs');
var path = require('path');

var ROOT = path.join(__dirname, '..');
var FIXTURE = path.join(ROOT, 'tests', 'golden', 'addon_forms.json');
function golden(name) { return require(path.join(ROOT, 'tests', 'golden', name + '.json')); }

var addon = require(path.join(ROOT, 'elliptic_amd', 'js', 'ellgpu.node'));
addon.open(process.env.ELLGPU_LIB || path.join(ROOT, 'elliptic_amd', 'lib', 'libellgpu.so'));
var ctx = addon.createContext(0);

function wide(h, B) { var b = Buffer.alloc(B); var v = Buffer.from(h.length % 2 ? '0' + h : h, 'hex'); v.copy(b, B - v.length); return b; }
function b32(h) { return wide(h, 32); }
function cat() { return Buffer.concat(Array.prototype.slice.call(arguments)); }
function hex(h) { return Buffer.from(h, 'hex'); }
function aligned(b) { var a = Buffer.alloc(b.length); b.copy(a); return a; }     // Buffer.alloc: never out of the pool
function u32(vs) { var b = Buffer.alloc(4 * vs.length); vs.forEach(function(v, i) { b.writeUInt32LE(v, 4 * i); }); return b; }
function offsets(msgs) {
  var b = Buffer.alloc(8 * (msgs.length + 1)), pos = 0;
  msgs.forEach(function(m, i) { pos += m.length; b.writeUInt32LE(pos, 8 * (i + 1)); });
  return b;
}

// ---- what a call answered ------------------------------------------------------------------
function pinValue(v, digest) {
  function one(b) {
    if (!Buffer.isBuffer(b)) return { value: b === undefined ? null : b };
    return digest ? { length: b.length, sha256: crypto.createHash('sha256').update(b).digest('hex') } :
      { length: b.length, hex: b.toString('hex') };
  }
  if (Buffer.isBuffer(v)) return { bare: one(v) };
  if (v === null || typeof v !== 'object') return { value: v === undefined ? null : v };
  var names = Object.keys(v);
  return { names: names, buffers: names.map(function(k) { return one(v[k]); }) };
}
function syncOutcome(f, digest) {
  try { return pinValue(f(), digest); } catch (e) { return { throws: String(e.message) }; }
}
function asyncOutcome(args, digest) {
  var p;
  try { p = addon.callAsync.apply(addon, args); } catch (e) { return Promise.resolve({ throws: String(e.message) }); }
  return p.then(function(v) { return pinValue(v, digest); }, function(e) { return { rejects: String(e.message) }; });
}

// ---- the calls -------------------------------------------------------------------------------
// { name: the export, tag, args: the arguments after ctx, ints: {label: index in args} of the lengths
//   that must be positive, id + aargs: callAsync's (curve, hashLen, msgBits, b0, b1, b2, b3, i0, i1),
//   aints: the same lengths by index in aargs, own: index of the first trailing result Buffer }
var calls = [];
function add(name, tag, args, o) {
  o = o || {};
  calls.push({ name: name, tag: tag, args: args, ints: o.ints || {}, id: o.id, aargs: o.aargs, aints: o.aints || {}, op: o.op });
}

var K = addon.curveId('secp256k1');
var cap = golden('captured_secp256k1');
var fb = golden('fixed_base')[0];
var k2 = cat(b32(cap.mul[0].k), b32(cap.mul[1].k));
var P2 = cat(b32(cap.mul[0].px), b32(cap.mul[0].py), b32(cap.mul[1].px), b32(cap.mul[1].py));
var ma = cap.muladd;
var ka = cat(b32(ma[0].k1), b32(ma[1].k1)), kb = cat(b32(ma[0].k2), b32(ma[1].k2));
var Pa = cat(b32(ma[0].p1x), b32(ma[0].p1y), b32(ma[1].p1x), b32(ma[1].p1y));
var Pb = cat(b32(ma[0].p2x), b32(ma[0].p2y), b32(ma[1].p2x), b32(ma[1].p2y));
var vf = cap.verify;
var H2 = cat(hex(vf[0].z), hex(vf[1].z)), HL = vf[0].z.length / 2;
var R2 = cat(b32(vf[0].r), b32(vf[1].r)), S2 = cat(b32(vf[0].s), b32(vf[1].s));
var Q2 = cat(b32(vf[0].qx), b32(vf[0].qy), b32(vf[1].qx), b32(vf[1].qy));
var d2 = cat(b32(fb.k[3]), b32(fb.k[4])), nonce2 = cat(b32(fb.k[5]), b32(fb.k[6]));
var recid = Buffer.from([0, 1]), zeros2 = Buffer.from([0, 0]), inf01 = Buffer.from([0, 1]);
var enc65 = cat(Buffer.from([4]), Q2.slice(0, 64), Buffer.from([4]), Q2.slice(64));
var X2 = cat(Q2.slice(0, 32), Q2.slice(64, 96));

add('mulFixed', '', [K, k2], { id: 0, aargs: [K, 0, 0, k2, null, null, null, 0, 0] });
add('mulVar', '', [K, k2, P2], { id: 1, aargs: [K, 0, 0, k2, P2, null, null, 0, 0] });
add('mulAdd2', 'p1', [K, ka, Pa, kb, Pb], { id: 2, aargs: [K, 0, 0, ka, Pa, kb, Pb, 0, 0] });
add('mulAdd2', 'generator', [K, ka, null, kb, Pb], { id: 2, aargs: [K, 0, 0, ka, null, kb, Pb, 0, 0] });
add('ecdsaVerify', '', [K, H2, HL, 0, R2, S2, Q2], { ints: { hashLen: 2 }, id: 3, aargs: [K, HL, 0, H2, R2, S2, Q2, 0, 0], aints: { hashLen: 1 } });
add('ecdsaSign', '', [K, H2, HL, 0, d2, nonce2, true], { ints: { hashLen: 2 } });
add('ecdsaSignDet', '', [K, H2, HL, 0, d2, true], { ints: { hashLen: 2 }, id: 5, aargs: [K, HL, 0, H2, d2, null, null, 1, 0], aints: { hashLen: 1 } });
add('ecdsaRecover', '', [K, H2, HL, R2, S2, recid], { ints: { hashLen: 2 }, id: 6, aargs: [K, HL, 0, H2, R2, S2, recid, 0, 0], aints: { hashLen: 1 } });
add('decodePoints', '', [K, enc65, 65], { ints: { encLen: 2 }, id: 8, aargs: [K, 0, 0, enc65, null, null, null, 65, 0], aints: { encLen: 7 } });
add('encodePoints', 'full', [K, Q2, false]);
add('encodePoints', 'compact', [K, Q2, true]);
add('validate', 'inf', [K, Q2, inf01, true]);
add('validate', 'noinf', [K, Q2, null, false]);
add('pointAdd', '', [K, Q2, zeros2, P2, null]);
add('decompress', '', [K, X2, inf01]);
var der = addon.sigToDer(ctx, K, R2, S2);
var STRIDE = der.der.length / 2, lens = aligned(der.lens);
add('sigToDer', '', [K, R2, S2]);
add('sigFromDer', '', [K, der.der, STRIDE, lens], { ints: { stride: 2 } });
add('ecdsaVerifyWire', '', [K, H2, HL, 0, der.der, STRIDE, lens, enc65, 65], { ints: { hashLen: 2, stride: 5, keyLen: 8 }, id: 7,
  aargs: [K, HL, 0, H2, der.der, lens, enc65, STRIDE, 65], aints: { hashLen: 1, stride: 7, keyLen: 8 } });

var c25 = golden('captured_curve25519').mul;
var xk = cat(b32(c25[0].k), b32(c25[1].k)), xx = cat(b32(c25[0].px), b32(c25[1].px));
add('x25519', '', [xk, xx], { id: 4, aargs: [7, 0, 0, xk, xx, null, null, 0, 0] });
add('x25519Derive', '', [xk, xx]);

var ev = golden('eddsa_verify_base');
var ED = addon.curveId('ed25519');
function edEncode(k) { var e = Buffer.from(b32(k.y)).reverse(); if (b32(k.x)[31] & 1) e[31] |= 0x80; return e; }
var ecs = [ev.cases[1][1], ev.cases[1][2]];                    // two messages of different lengths under one key
var emsgs = ecs.map(function(c) { return hex(c[1]); });
var emsg = Buffer.concat(emsgs), eoff = offsets(emsgs), esig = cat(hex(ecs[0][2]), hex(ecs[1][2]));
var epub = cat(edEncode(ev.keys[1]), edEncode(ev.keys[1]));
var fixedMsg = Buffer.from('abcdef');
add('eddsaVerify', 'offsets', [emsg, eoff, 0, esig, epub]);
add('eddsaVerify', 'msgLen', [fixedMsg, null, 3, esig, epub]);
add('eddsaSign', 'offsets', [emsg, eoff, 0, d2]);
add('eddsaSign', 'msgLen', [fixedMsg, null, 3, d2]);

// fixed-base tables of caller-chosen points: the narrowest comb the call accepts
function basePoint(b) { return cat(b32(b[0]), b32(b[1])); }
var h1 = addon.defineBase(ctx, K, basePoint(fb.bases[1]), 4), h2 = addon.defineBase(ctx, K, basePoint(fb.bases[2]), 4);
var he = addon.defineEdBase(ctx, ED, cat(b32(ev.keys[1].x), b32(ev.keys[1].y)), 0);
add('mulBase', '', [h1, k2], { id: 29, aargs: [K, 0, 0, k2, null, null, null, h1, 0] });
add('mulBase2', '', [h1, h2, ka, kb], { id: 30, aargs: [K, 0, 0, ka, kb, null, null, h1, h2] });
add('ecdsaVerifyBase', '', [h1, H2, HL, 0, R2, S2], { ints: { hashLen: 2 }, id: 31, aargs: [K, HL, 0, H2, R2, S2, null, h1, 0], aints: { hashLen: 1 } });
add('eddsaVerifyBase', 'offsets', [he, emsg, eoff, 0, esig], { id: 32, aargs: [ED, 0, 0, emsg, eoff, esig, null, he, 0] });
add('eddsaVerifyBase', 'msgLen', [he, fixedMsg, null, 3, esig]);

// one user-defined short domain (as tools/check_custom_wire_engine.js defines it)
var sw = golden('custom_wire')[0];
var SD = addon.defineShortDomain(ctx, b32(sw.p), b32(sw.a), b32(sw.b), b32(sw.n), b32(sw.g.x), b32(sw.g.y));
var sdec = sw.decode.filter(function(c) { return c.enc.length === sw.decode[0].enc.length; }).slice(0, 2);
var senc = cat(hex(sdec[0].enc), hex(sdec[1].enc)), SEL = sdec[0].enc.length / 2;
var sxy = cat(b32(sdec[0].x), b32(sdec[0].y), b32(sw.g.x), b32(sw.g.y));
var swr = sw.wire.filter(function(c) { return c.h.length === sw.wire[0].h.length && c.key.length === sw.wire[0].key.length && c.bits === sw.wire[0].bits; }).slice(0, 2);
var sH = cat(hex(swr[0].h), hex(swr[1].h)), SHL = swr[0].h.length / 2, SKL = swr[0].key.length / 2;
var SST = Math.max(swr[0].der.length, swr[1].der.length) / 2;
var sder = cat(wide('', SST), wide('', SST)); hex(swr[0].der).copy(sder, 0); hex(swr[1].der).copy(sder, SST);
var slens = u32([swr[0].der.length / 2, swr[1].der.length / 2]);
var skeys = cat(hex(swr[0].key), hex(swr[1].key));
var sr = cat(b32(sw.g.x), b32(sdec[0].x)), ss = cat(b32('1234567'), b32('89abcdef'));
var sd = cat(b32('07'), b32('0b')), sk = cat(b32('0d'), b32('11'));
add('customDecompress', '', [SD, cat(b32(sdec[0].x), b32(sw.g.x)), inf01]);
add('customDecodePoints', '', [SD, senc, SEL], { ints: { encLen: 2 } });
add('customVerifyWire', '', [SD, sH, SHL, 0, sder, SST, slens, skeys, SKL], { ints: { hashLen: 2, stride: 5, keyLen: 8 }, id: 9,
  aargs: [SD, SHL, 0, sH, sder, slens, skeys, SST, SKL], aints: { hashLen: 1, stride: 7, keyLen: 8 } });
add('customRecover', '', [SD, sH, SHL, sr, ss, recid], { ints: { hashLen: 2 }, id: 10, aargs: [SD, SHL, 0, sH, sr, ss, recid, 0, 0], aints: { hashLen: 1 } });
add('customSign', '', [SD, sH, SHL, 0, sd, sk, true], { ints: { hashLen: 2 }, id: 11, aargs: [SD, SHL, 0, sH, sd, sk, null, 1, 0], aints: { hashLen: 1 } });
add('customSignDet', '', [SD, sH, SHL, 0, sd, 0, true], { ints: { hashLen: 2 }, id: 12, aargs: [SD, SHL, 0, sH, sd, null, null, 1, 0], aints: { hashLen: 1 } });
// customEcdh(ctx, op, curve, b0, b1, i0, i1): the ops 13..25
function ecdh(op, tag, curve, b0, b1, i0, i1, o) {
  o = o || {};
  add('customEcdh', op + (tag ? '/' + tag : ''), [op, curve, b0, b1, i0, i1], { ints: o.ints, id: op, aargs: [curve, 0, 0, b0, b1, null, null, i0, i1], aints: o.aints, op: op });
}
ecdh(13, '', SD, sd, sxy, 0, 0);
ecdh(14, '', SD, sd, senc, SEL, 0, { ints: { keyLen: 4 }, aints: { keyLen: 7 } });
ecdh(15, 'inf', SD, sxy, inf01, 1, 0);
ecdh(15, 'noinf', SD, sxy, null, 0, 0);
ecdh(16, 'full', SD, sxy, null, 0, sw.pl, { ints: { coordBytes: 5 }, aints: { coordBytes: 8 } });
ecdh(16, 'compact', SD, sxy, null, 1, sw.pl, { ints: { coordBytes: 5 }, aints: { coordBytes: 8 } });

// one Montgomery curve (as tools/check_custom_mont_engine.js defines it)
var mc = golden('custom_mont')[0];
var MC = addon.defineMont(ctx, b32(mc.p), b32(mc.a));
var mk = cat(b32(mc.cases[3].k), b32(mc.cases[4].k)), mx = cat(b32(mc.cases[3].x), b32(mc.cases[4].x));
ecdh(17, '', MC, mk, mx, 0, 0);
ecdh(18, '', MC, mx, null, 0, 0);
ecdh(19, '', MC, mk, mx, 0, 0);

// one Edwards domain (as tools/check_custom_ed_ecdsa_engine.js defines it)
var ec = golden('custom_ed_ecdsa')[0];
var EDD = addon.defineEdwardsDomain(ctx, b32(ec.p), b32(ec.a), b32(ec.d), b32(ec.n), b32(ec.gx), b32(ec.gy));
var evf = ec.verify.filter(function(c) { return c.h.length === ec.verify[0].h.length && c.bits === ec.verify[0].bits; }).slice(0, 2);
var eH = cat(hex(evf[0].h), hex(evf[1].h)), EHL = evf[0].h.length / 2;
var eR = cat(b32(evf[0].r), b32(evf[1].r)), eS = cat(b32(evf[0].s), b32(evf[1].s)), eQ = cat(hex(evf[0].q), hex(evf[1].q));
var exy = cat(b32(ec.gx), b32(ec.gy), hex(evf[0].q));
var EPL = 32; while (EPL > 1 && b32(ec.p)[32 - EPL] === 0) EPL--;
var eenc = cat(Buffer.from([4]), wide(ec.gx, EPL), wide(ec.gy, EPL), Buffer.from([4]), hex(evf[0].q).slice(32 - EPL, 32), hex(evf[0].q).slice(64 - EPL, 64));
var EEL = 1 + 2 * EPL;
ecdh(20, 'fromX', EDD, cat(b32(ec.gx), hex(evf[0].q).slice(0, 32)), inf01, 0, 0);
ecdh(20, 'fromY', EDD, cat(b32(ec.gy), hex(evf[0].q).slice(32)), inf01, 1, 0);
ecdh(21, '', EDD, eenc, null, EEL, 0, { ints: { encLen: 4 }, aints: { encLen: 7 } });
ecdh(22, 'order', EDD, exy, b32(ec.n), 0, 0);
ecdh(22, 'noorder', EDD, exy, null, 0, 0);
ecdh(23, '', EDD, sd, exy, 0, 0);
ecdh(24, '', EDD, sd, eenc, EEL, 0, { ints: { keyLen: 4 }, aints: { keyLen: 7 } });
ecdh(25, 'full', EDD, exy, null, 0, EPL, { ints: { coordBytes: 5 }, aints: { coordBytes: 8 } });
ecdh(25, 'compact', EDD, exy, null, 1, EPL, { ints: { coordBytes: 5 }, aints: { coordBytes: 8 } });
add('customEdVerify', '', [EDD, eH, EHL, 0, eR, eS, eQ], { ints: { hashLen: 2 }, id: 26, aargs: [EDD, EHL, 0, eH, eR, eS, eQ, 0, 0], aints: { hashLen: 1 } });
add('customEdSign', '', [EDD, eH, EHL, 0, sd, sk, true], { ints: { hashLen: 2 }, id: 27, aargs: [EDD, EHL, 0, eH, sd, sk, null, 1, 0], aints: { hashLen: 1 } });
add('customEdSignDet', '', [EDD, eH, EHL, 0, sd, 0, true], { ints: { hashLen: 2 }, id: 28, aargs: [EDD, EHL, 0, eH, sd, null, null, 1, 0], aints: { hashLen: 1 } });

// ---- running them ----------------------------------------------------------------------------
function longer(b) { return Buffer.concat([b, Buffer.alloc(1)]); }
function withArg(args, i, v) { var a = args.slice(); a[i] = v; return a; }
function syncCall(c, args, digest) {
  return syncOutcome(function() { return addon[c.name].apply(addon, [ctx].concat(args)); }, digest);
}
function asyncCall(c, aargs, digest, id) {
  return asyncOutcome([id === undefined ? c.id : id, ctx].concat(aargs), digest);
}

function runCall(c) {
  var e = { sync: syncCall(c, c.args, false), refusals: {} };
  var r = e.refusals;
  c.args.forEach(function(a, i) {
    if (!Buffer.isBuffer(a)) return;
    r['arg' + i + ' one byte longer'] = syncCall(c, withArg(c.args, i, longer(a)), true);
    r['arg' + i + ' null'] = syncCall(c, withArg(c.args, i, null), true);
  });
  r['last argument missing'] = syncCall(c, c.args.slice(0, -1), true);
  r['ctx only'] = syncCall(c, [], true);
  Object.keys(c.ints).forEach(function(k) {
    r[k + ' 0'] = syncCall(c, withArg(c.args, c.ints[k], 0), true);
    r[k + ' -1'] = syncCall(c, withArg(c.args, c.ints[k], -1), true);
    if (k === 'coordBytes') r[k + ' 33'] = syncCall(c, withArg(c.args, c.ints[k], 33), true);
  });
  if (c.name === 'customEcdh') {
    r['op 12'] = syncCall(c, withArg(c.args, 0, 12), true);
    r['op 26'] = syncCall(c, withArg(c.args, 0, 26), true);
  }
  if (c.name === 'mulFixed' || c.name === 'mulVar' || c.name === 'mulAdd2') {
    // the synchronous-only form: trailing (xy, inf) result Buffers of the caller's
    var xy = Buffer.alloc(128, 0xee), inf = Buffer.alloc(2, 0xee);
    var res = addon[c.name].apply(addon, [ctx].concat(c.args, [xy, inf]));
    e.own = pinValue(res, false);
    e.own.same = res.xy === xy && res.inf === inf;
    r['own xy one byte longer'] = syncCall(c, c.args.concat([longer(xy), inf]), true);
    r['own inf one byte longer'] = syncCall(c, c.args.concat([xy, longer(inf)]), true);
    r['own inf not a Buffer'] = syncCall(c, c.args.concat([xy, 7]), true);
  }
  if (c.id === undefined) return Promise.resolve(e);
  var steps = [];
  function step(label, aargs, id) {
    steps.push(function() {
      return asyncCall(c, aargs, label !== null, id).then(function(o) { if (label === null) e.async = o; else e.asyncRefusals[label] = o; });
    });
  }
  e.asyncRefusals = {};
  step(null, c.aargs);
  c.aargs.forEach(function(a, i) {
    if (i < 3 || i > 6) return;
    if (Buffer.isBuffer(a)) step('b' + (i - 3) + ' one byte longer', withArg(c.aargs, i, longer(a)));
    if (Buffer.isBuffer(a)) step('b' + (i - 3) + ' null', withArg(c.aargs, i, null));
  });
  step('too few arguments', c.aargs.slice(0, 6));
  Object.keys(c.aints).forEach(function(k) {
    step(k + ' 0', withArg(c.aargs, c.aints[k], 0));
    step(k + ' -1', withArg(c.aargs, c.aints[k], -1));
    if (k === 'coordBytes') step(k + ' 33', withArg(c.aargs, c.aints[k], 33));
  });
  step('op -1', c.aargs, -1);
  step('op 33', c.aargs, 33);
  step('curve -1', withArg(c.aargs, 0, -1));
  return steps.reduce(function(p, s) { return p.then(s); }, Promise.resolve()).then(function() { return e; });
}

function record() {
  var out = { ops: addon.ops === undefined ? null : addon.ops, calls: {} };
  return calls.reduce(function(p, c) {
    return p.then(function() { return runCall(c); }).then(function(e) { out.calls[c.name + (c.tag ? ':' + c.tag : '')] = e; });
  }, Promise.resolve()).then(function() {
    [h1, h2, he].forEach(function(h) { addon.releaseBase(ctx, h); });
    addon.destroyContext(ctx);
    return out;
  });
}

function differences(want, got, where, out) {
  if (out.length > 20) return;
  if (want === null || got === null || typeof want !== 'object' || typeof got !== 'object') {
    if (want !== got) out.push(where + ': ' + JSON.stringify(got) + ', recorded ' + JSON.stringify(want));
    return;
  }
  Object.keys(want).concat(Object.keys(got).filter(function(k) { return !(k in want); })).forEach(function(k) {
    if (!(k in want) || !(k in got)) out.push(where + '.' + k + ': ' + (k in got ? 'not recorded' : 'missing'));
    else differences(want[k], got[k], where + '.' + k, out);
  });
}

var compare = process.argv.indexOf('--compare') >= 0;
record().then(function(got) {
  var nref = 0, nasync = 0;
  Object.keys(got.calls).forEach(function(k) {
    var e = got.calls[k];
    nref += Object.keys(e.refusals).length + Object.keys(e.asyncRefusals || {}).length;
    if (e.async) nasync++;
  });
  if (!compare) {
    delete got.ops;                                  // (the id table is compared with index.js's use of it by the test)
    fs.writeFileSync(FIXTURE, JSON.stringify(got, null, 0).replace(/\},"/g, '},\n"') + '\n');
    console.log(FIXTURE + ': ' + Object.keys(got.calls).length + ' calls, ' + nasync + ' Promise forms, ' + nref + ' changed calls');
    return;
  }
  var want = JSON.parse(fs.readFileSync(FIXTURE, 'utf8'));
  var diffs = [], forms = [];
  differences(want.calls, got.calls, 'calls', diffs);
  Object.keys(got.calls).forEach(function(k) {      // the Promise resolves to what the synchronous form returns
    if (got.calls[k].async) differences(got.calls[k].sync, got.calls[k].async, k + ': Promise form', forms);
  });
  console.log(JSON.stringify({ ok: diffs.length + forms.length === 0, calls: Object.keys(got.calls).length, promiseForms: nasync,
    changedCalls: nref, ops: got.ops, differences: diffs.concat(forms) }));
  process.exit(diffs.length + forms.length ? 1 : 0);
}).catch(function(e) { console.log(JSON.stringify({ ok: false, error: String(e && e.stack || e) })); process.exit(1); });
