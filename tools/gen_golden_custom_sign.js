'use strict';
// Golden vectors for EC#sign on user-defined ECDSA domains (ellgpu_custom_sign, _custom_sign_det):
// every r, s, recovery parameter and acceptance from the reference's own EC#sign.  Runs only where
// the reference is present (see tools/ref_loader.js); all randomness is SHA-256 counter mode over a
// fixed seed, so a rerun reproduces tests/golden/custom_sign.json byte for byte.
//
//   node tools/gen_golden_custom_sign.js [outdir]
//
// Domains: the six of custom_recover.json (tools/gen_golden_custom_recover.js).
//
// `det`: EC#sign(h, d, {canonical: c, msgBitLength: bits || undefined}) on an EC whose hash is
//   `hash` (sha256 / sha384 / sha512) -> r, s (64 hex digits), j = recoveryParam; or `msg`, what the
//   reference throws (secp112r1: HmacDRBG refuses 14 bytes of entropy).
// `sup`: the same call with options.k = a function that hands out the BN `k` on the first pass and
//   stops the loop on the second -> ok = 1 with r, s, j where the reference accepted the nonce on
//   that pass, ok = 0 where it went on to ask for another.  On secp112r1, where EC#sign throws before
//   its loop, the pass is restated below (onePass) from the reference's own _truncateToN, BN and
//   curve objects; on the other domains onePass is checked against EC#sign here and not recorded.
// h = the digest (hex), d = the private key as given (64 hex digits, possibly >= n), tag = what the
// case exercises.

var fs = require('fs');
var path = require('path');
var crypto = require('crypto');
var ref = require('./ref_loader').load();
var elliptic = ref.elliptic;
var BN = ref.BN;
var hash = ref.breq(19);

var OUT = process.argv[2] || path.join(__dirname, '..', 'tests', 'golden');
var GOLDEN_RECOVER = path.join(__dirname, '..', 'tests', 'golden', 'custom_recover.json');

function Prng(seed) { this.seed = seed; this.ctr = 0; }
Prng.prototype.bytes = function(n) {
  var out = [];
  while (out.length < n) {
    var h = crypto.createHash('sha256').update(this.seed + ':' + (this.ctr++)).digest();
    for (var i = 0; i < h.length && out.length < n; i++) out.push(h[i]);
  }
  return Buffer.from(out);
};
Prng.prototype.below = function(n) {            // uniform-ish in [1, n)
  for (;;) {
    var k = new BN(this.bytes(Math.ceil(n.bitLength() / 8))).maskn(n.bitLength()).umod(n);
    if (!k.isZero()) return k;
  }
};

function hex32(bn) { return bn.toString(16, 64); }

var HASHES = ['sha256', 'sha384', 'sha512'];

// the domains' parameters are the committed ones of custom_recover.json (made from the reference)
function build(spec, hname) {
  var pc = new elliptic.curves.PresetCurve({ type: 'short', prime: null, p: spec.p, a: spec.a, b: spec.b,
    n: spec.n, hash: hash[hname], gRed: false, g: [spec.g.x, spec.g.y] });
  return new elliptic.ec(pc);
}

var STOP = { stop: true };

// one pass of EC#sign's loop (ec/index.js:126, 157-184) with the reference's own objects
function onePass(ec, h, bits, d, k, canonical) {
  var n = ec.n;
  var msg = ec._truncateToN(h, false, bits || undefined);
  var priv = ec.keyFromPrivate(d.clone()).getPrivate();
  k = ec._truncateToN(k.clone(), true);
  if (k.cmpn(1) <= 0 || k.cmp(n.sub(new BN(1))) >= 0) return null;
  var kp = ec.g.mul(k);
  if (kp.isInfinity()) return null;
  var kpX = kp.getX();
  var r = kpX.umod(n);
  if (r.cmpn(0) === 0) return null;
  var s = k.invm(n).mul(r.mul(priv).iadd(msg)).umod(n);
  if (s.cmpn(0) === 0) return null;
  var j = (kp.getY().isOdd() ? 1 : 0) | (kpX.cmp(r) !== 0 ? 2 : 0);
  if (canonical && s.cmp(ec.nh) > 0) { s = n.sub(s); j ^= 1; }
  return { r: r, s: s, j: j };
}

function gen(spec) {
  var rng = new Prng('ellgpu-golden-v1:custom-sign:' + spec.name);
  var ecs = {};
  HASHES.forEach(function(hn) { ecs[hn] = build(spec, hn); });
  var ec0 = ecs.sha256, n = ec0.n, nb = n.byteLength(), nbits = n.bitLength();
  var small = nb < 24;
  var top = new BN(1).ushln(256);
  var det = [], sup = [];

  function recDet(tag, hn, h, bits, d, c) {
    var o = { tag: tag, hash: hn, h: Buffer.from(h).toString('hex'), bits: bits, d: hex32(d), c: c };
    try {
      var sg = ecs[hn].sign(Buffer.from(h), d.clone(), { canonical: !!c, msgBitLength: bits || undefined });
      o.r = hex32(sg.r); o.s = hex32(sg.s); o.j = sg.recoveryParam;
      if (small) throw new Error('EC#sign was expected to throw on ' + spec.name);
    } catch (e) {
      if (!small || !/Not enough entropy/.test(e.message)) throw e;
      o.msg = e.message;
    }
    det.push(o);
  }
  function recSup(tag, h, bits, d, k, c) {
    var o = { tag: tag, h: Buffer.from(h).toString('hex'), bits: bits, d: hex32(d), k: hex32(k), c: c };
    var mine = onePass(ec0, Buffer.from(h), bits, d, k, c);
    var got;
    if (small) {
      got = mine;
    } else {
      try {
        var sg = ec0.sign(Buffer.from(h), d.clone(), { canonical: !!c, msgBitLength: bits || undefined,
          k: function(iter) { if (iter > 0) throw STOP; return k.clone(); } });
        got = { r: sg.r, s: sg.s, j: sg.recoveryParam };
      } catch (e) {
        if (e !== STOP) throw e;
        got = null;
      }
      if ((got === null) !== (mine === null) ||
          (got && (got.r.cmp(mine.r) || got.s.cmp(mine.s) || got.j !== mine.j)))
        throw new Error('the restated pass differs from EC#sign: ' + spec.name + ' ' + tag);
    }
    o.ok = got ? 1 : 0;
    if (got) { o.r = hex32(got.r); o.s = hex32(got.s); o.j = got.j; }
    sup.push(o);
  }

  // digests shorter than, as long as and longer than n, an explicit msgBitLength (a shift of its
  // own: 8 nb + 4 - nbits bits), and a digest whose truncation is >= n
  var ones = Buffer.alloc(nb, 0xff);
  var kinds = [
    function() { return ['short_digest', rng.bytes(20), 0]; },
    function() { return ['digest_as_n', rng.bytes(nb), 0]; },
    function() { return ['digest_64', rng.bytes(64), 0]; },
    function() { return ['msg_bits', rng.bytes(nb), 8 * nb + 4]; },
    function() { return ['truncation_ge_n', ones, 0]; },
  ];
  if (small) {
    HASHES.forEach(function(hn) { recDet('throws', hn, rng.bytes(nb), 0, rng.below(n), 0); });
  } else {
    var cnt = 0;
    HASHES.forEach(function(hn) {
      kinds.forEach(function(kf) {
        var kd = kf();
        recDet(kd[0], hn, kd[1], kd[2], rng.below(n), (cnt++) & 1);
      });
    });
    // private keys 1, n - 1, >= n and a full 32-byte value: both canonical values, the hashes in turn
    var privs = [['priv_one', new BN(1)], ['priv_n_minus_1', n.subn(1)],
      ['priv_ge_n', n.addn(5).cmp(top) < 0 ? n.addn(5) : n.clone()], ['priv_32_bytes', top.subn(3)]];
    privs.forEach(function(pv, i) {
      var h = rng.bytes(nb);
      recDet(pv[0], HASHES[i % 3], h, 0, pv[1], 0);
      recDet(pv[0], HASHES[(i + 1) % 3], h, 0, pv[1], 1);
    });
  }
  // supplied nonces
  var zt = new BN(rng.bytes(nb - 1));
  var full = rng.bytes(nb); full[0] |= 0x80;
  var ks = [['k_0', new BN(0)], ['k_1', new BN(1)], ['k_2', new BN(2)], ['k_n_minus_2', n.subn(2)],
    ['k_n_minus_1', n.subn(1)], ['k_n', n.clone()], ['k_zero_top_byte', zt], ['k_full_width', new BN(full)],
    ['k_ordinary', rng.below(n)]];
  if (nb < 32) {
    var wide = rng.bytes(32); wide[0] |= 0x80;
    ks.push(['k_wider_than_n', new BN(wide)]);
    ks.push(['k_one_byte_wider', new BN(rng.bytes(nb + 1))]);
  }
  ks.forEach(function(kv, i) {
    var kd = kinds[i % kinds.length]();
    recSup(kv[0], kd[1], kd[2], i === 3 ? top.subn(7) : rng.below(n), kv[1], i & 1);
  });
  // the ordinary nonce again under the other canonical value, and a few more of them
  for (var i = 0; i < 4; i++) {
    var h = rng.bytes(nb), d = rng.below(n), k = rng.below(n);
    recSup('k_ordinary', h, 0, d, k, 0);
    recSup('k_ordinary', h, 0, d, k, 1);
  }
  return { name: spec.name, p: spec.p, a: spec.a, b: spec.b, n: spec.n, g: spec.g, nbits: nbits, nbytes: nb,
    det: det, sup: sup };
}

var specs = JSON.parse(fs.readFileSync(GOLDEN_RECOVER, 'utf8'));
var out = specs.map(gen);
var file = path.join(OUT, 'custom_sign.json');
fs.writeFileSync(file, JSON.stringify(out).replace(/\{"tag"/g, '\n{"tag"') + '\n');
out.forEach(function(c) {
  var acc = c.sup.filter(function(d) { return d.ok; }).length;
  console.log(c.name + ': ' + c.det.length + ' EC#sign cases (' + c.det.filter(function(d) { return d.msg; }).length +
    ' thrown), ' + c.sup.length + ' supplied nonces (' + acc + ' accepted)');
});
console.log('wrote ' + file);
