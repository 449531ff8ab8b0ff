'use strict';
// Golden vectors for ECDSA on user-defined Edwards domains (ellgpu_curve_define_edwards_domain,
// ellgpu_custom_ed_verify, _custom_ed_sign, _custom_ed_sign_det): every verdict, r, s, recovery
// parameter and acceptance from the reference's own EC#verify and EC#sign over
//   new elliptic.ec(new elliptic.curves.PresetCurve({type: 'edwards', prime: null, p, a, c: '1', d,
//                                                    n, hash, gRed: false, g: [gx, gy]}))
// Runs only where the reference is present (see tools/ref_loader.js); all randomness is SHA-256
// counter mode over a fixed seed, so a rerun reproduces tests/golden/custom_ed_ecdsa.json byte for byte.
//
//   node tools/gen_golden_custom_ed_ecdsa.js [outdir]
//
// Domains (a a square and d a non-square on all four: the addition law is complete; asserted):
//   curve1174        a = 1, d = -1174 over 2^251 - 9, the published generator and prime subgroup
//                    order, floor(p / n) = 4
//   e222             a = 1, d = 160102 over 2^222 - 117, published n and G; p has 28 bytes, so the
//                    usual digests are longer than n
//   ed25519_by_hand  a = -1, d = -121665/121666 over 2^255 - 19 with the preset's n and G, passed as
//                    a = '-1': the reference runs its EXTENDED formulas here; cofactor 8, floor(p / n) = 7
//                    (n lies just above 2^252)
//   toy_p65521       the one domain without _maxwellTrick (floor(p / n) > 100), which is the only way
//                    to reach EC#verify's getX().umod(n) branch.  Found by counting: p = 65521 (the
//                    largest 16-bit prime), a = 1, and the least non-residue d whose curve order
//                    #E = sum over x of (1 + legendre((1 - x^2) / (1 - d x^2))) has an odd prime factor
//                    q with 257 <= q < p / 100; G = (#E / q) * (the first point from pointFromY, y = 2,
//                    3, ...) that is not the identity.  toyDomain() below redoes the search.
// Per domain:
//   verify  {tag, h, bits, r, s, q, ok}: EC#verify(h, {r, s}, {x, y}, undefined, {msgBitLength: bits ||
//           undefined}); q = x || y (128 hex digits).  Off-curve keys (tag off_curve*) carry no ok: the
//           engine's answer there is status 2.
//   det     EC#sign on an EC whose hash is `hash`, as tools/gen_golden_custom_sign.js records it; or
//           msg, what the reference throws (the toy domain: 'Not enough entropy')
//   sup     one pass of the loop for a supplied nonce (the options.k / stop trick of
//           gen_golden_custom_sign.js); on the toy domain, where EC#sign throws before its loop, the
//           pass restated from the reference's own objects (onePass), which is checked against
//           EC#sign on the other domains

var fs = require('fs');
var path = require('path');
var crypto = require('crypto');
var ref = require('./ref_loader').load();
var elliptic = ref.elliptic;
var BN = ref.BN;
var hash = ref.breq(19);

var OUT = process.argv[2] || path.join(__dirname, '..', 'tests', 'golden');

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
function legendre(x, p) {
  var r = x.toRed(BN.red(p)).redPow(p.subn(1).ushrn(1)).fromRed();
  return r.cmpn(1) === 0 ? 1 : r.isZero() ? 0 : -1;
}

var HASHES = ['sha256', 'sha384', 'sha512'];
var TOP = new BN(1).ushln(256);

// ---- the toy domain, found by counting ------------------------------------------------------
function powmod(b, e, m) { var r = 1; b %= m; while (e) { if (e & 1) r = r * b % m; b = b * b % m; e >>>= 1; } return r; }
function toyDomain() {
  var p = 65521;
  function leg(v) { v = ((v % p) + p) % p; return v === 0 ? 0 : (powmod(v, (p - 1) / 2, p) === 1 ? 1 : -1); }
  for (var d = 2; d < p; d++) {
    if (leg(d) !== -1) continue;
    var order = 0;
    for (var x = 0; x < p; x++) {
      var x2 = x * x % p;
      var den = (1 - d * x2 % p + p) % p;                      // never 0: d is a non-residue
      order += 1 + leg((1 - x2 + p) % p * powmod(den, p - 2, p) % p);
    }
    for (var q = 257; q * 101 <= p; q += 2) {
      var prime = true;
      for (var f = 3; f * f <= q; f += 2) if (q % f === 0) prime = false;
      if (prime && order % q === 0) return { p: p, d: d, order: order, q: q };
    }
  }
  throw new Error('no toy domain');
}

var P1174 = new BN(1).ushln(251).subn(9);
var P25519 = new BN(1).ushln(255).subn(19);
var ED = elliptic.curves.ed25519.curve;
var DOMAINS = [
  { name: 'curve1174', p: P1174, a: new BN(1), d: P1174.subn(1174),
    n: new BN(1).ushln(249).sub(new BN('11332719920821432534773113288178349711', 10)),
    gx: new BN('1582619097725911541954547006453739763381091388846394833492296309729998839514', 10),
    gy: new BN('3037538013604154504764115728651437646519513534305223422754827055689195992590', 10), q: 4 },
  { name: 'e222', p: new BN(1).ushln(222).subn(117), a: new BN(1), d: new BN(160102),
    n: new BN('1684996666696914987166688442938726735569737456760058294185521417407', 10),
    gx: new BN('2705691079882681090389589001251962954446177367541711474502428610129', 10), gy: new BN(28), q: 4 },
  { name: 'ed25519_by_hand', p: P25519, a: P25519.subn(1), aconf: '-1', d: ED.d.fromRed(), n: ED.n.clone(),
    gx: ED.g.getX(), gy: ED.g.getY(), q: 7 },
];
(function() {
  var t = toyDomain();
  var p = new BN(t.p), d = new BN(t.d);
  var bare = new elliptic.curve.edwards({ p: p.toString(16), a: '1', c: '1', d: d.toString(16) });
  var G = null;
  for (var y = 2; !G; y++) {
    try { G = bare.pointFromY(new BN(y), false).mul(new BN(t.order / t.q)); } catch (e) { G = null; }
    if (G && G.isInfinity()) G = null;
  }
  DOMAINS.push({ name: 'toy_p65521', p: p, a: new BN(1), d: d, n: new BN(t.q), gx: G.getX(), gy: G.getY(), q: null,
    found: { order: t.order } });
})();

function build(dom, hname) {
  return new elliptic.ec(new elliptic.curves.PresetCurve({ type: 'edwards', prime: null, p: dom.p.toString(16),
    a: dom.aconf || dom.a.toString(16), c: '1', d: dom.d.toString(16), n: dom.n.toString(16), hash: hash[hname],
    gRed: false, g: [dom.gx.toString(16), dom.gy.toString(16)] }));
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
// a signature from the nonce k, whatever EC#sign's entropy check says
function signWith(ec, h, bits, d, k) {
  var sg = onePass(ec, h, bits, d, k, 0);
  if (!sg) throw new Error('nonce refused');
  return sg;
}

function gen(dom) {
  var rng = new Prng('ellgpu-golden-v1:custom-ed-ecdsa:' + dom.name);
  var p = dom.p;
  if (legendre(dom.a, p) !== 1 || legendre(dom.d, p) !== -1) throw new Error(dom.name + ': addition law not complete');
  var ecs = {};
  HASHES.forEach(function(hn) { ecs[hn] = build(dom, hn); });
  var ec = ecs.sha256, curve = ec.curve, n = ec.n, nb = n.byteLength(), nbits = n.bitLength();
  if (!curve.validate(ec.g) || ec.g.isInfinity() || !ec.g.mul(n).isInfinity()) throw new Error(dom.name + ': bad generator');
  var fl = p.div(n);
  if (dom.q !== null ? (!curve._maxwellTrick || fl.cmpn(dom.q) !== 0) : (curve._maxwellTrick || fl.cmpn(100) <= 0))
    throw new Error(dom.name + ': floor(p / n) = ' + fl.toString(10) + ', _maxwellTrick = ' + curve._maxwellTrick);
  if (!!curve.extended !== (dom.name === 'ed25519_by_hand')) throw new Error(dom.name + ': unexpected coordinate system');
  var small = nb < 24;
  var ver = [], det = [], sup = [];

  function xy(P) { return hex32(P.getX()) + hex32(P.getY()); }
  function recVer(tag, h, bits, r, s, qx, qy, offCurve) {
    var o = { tag: tag, h: Buffer.from(h).toString('hex'), bits: bits, r: hex32(r), s: hex32(s), q: hex32(qx) + hex32(qy) };
    if (!offCurve) {
      o.ok = ecs.sha256.verify(Buffer.from(h), { r: r.clone(), s: s.clone() }, { x: qx.toString(16), y: qy.toString(16) },
        undefined, { msgBitLength: bits || undefined }) ? 1 : 0;
    }
    ver.push(o);
    return o;
  }
  function expect(o, ok) { if (o.ok !== ok) throw new Error(dom.name + ': ' + o.tag + ' answered ' + o.ok); }

  // ---- EC#verify ----
  var d = rng.below(n), Q = ec.g.mul(d), qx = Q.getX(), qy = Q.getY();
  var h = rng.bytes(32);
  var sg = signWith(ec, h, 0, d, rng.below(n));
  expect(recVer('valid', h, 0, sg.r, sg.s, qx, qy), 1);
  expect(recVer('r_flipped', h, 0, sg.r.xor(new BN(2)), sg.s, qx, qy), 0);
  expect(recVer('s_flipped', h, 0, sg.r, sg.s.xor(new BN(2)), qx, qy), 0);
  var h2 = Buffer.from(h); h2[0] ^= 0x80;
  expect(recVer('digest_flipped', h2, 0, sg.r, sg.s, qx, qy), 0);
  var Q2 = ec.g.mul(rng.below(n));
  expect(recVer('other_key', h, 0, sg.r, sg.s, Q2.getX(), Q2.getY()), 0);
  expect(recVer('r_0', h, 0, new BN(0), sg.s, qx, qy), 0);
  expect(recVer('s_0', h, 0, sg.r, new BN(0), qx, qy), 0);
  expect(recVer('r_n', h, 0, n.clone(), sg.s, qx, qy), 0);
  expect(recVer('s_n', h, 0, sg.r, n.clone(), qx, qy), 0);
  recVer('r_n_minus_1', h, 0, n.subn(1), sg.s, qx, qy);
  recVer('s_n_minus_1', h, 0, sg.r, n.subn(1), qx, qy);
  // a key equal to -(u1 / u2) G: P is the identity
  (function() {
    var msg = ec._truncateToN(h, false);
    var sinv = sg.s.invm(n);
    var u1 = sinv.mul(msg).umod(n), u2 = sinv.mul(sg.r).umod(n);
    var K = ec.g.mul(n.sub(u1.mul(u2.invm(n)).umod(n)));
    if (!ec.g.mulAdd(u1, K, u2).isInfinity()) throw new Error(dom.name + ': the identity was not reached');
    expect(recVer('p_is_identity', h, 0, sg.r, sg.s, K.getX(), K.getY()), 0);
  })();
  recVer('key_identity', h, 0, sg.r, sg.s, new BN(0), new BN(1));
  recVer('key_order_2', h, 0, sg.r, sg.s, new BN(0), p.subn(1));
  if (dom.a.cmpn(1) === 0) recVer('key_order_4', h, 0, sg.r, sg.s, new BN(1), new BN(0));
  if (qx.add(p).cmp(TOP) < 0 && qy.add(p).cmp(TOP) < 0) expect(recVer('key_plus_p', h, 0, sg.r, sg.s, qx.add(p), qy.add(p)), 1);
  // an r whose match needs j >= 1 (x(k G) >= n), one with j = 0, and the largest j the domain has
  (function() {
    var seen = {}, want = dom.q === null ? 3 : Math.min(dom.q, 3), tries = 0;
    while (Object.keys(seen).length < want && tries++ < 4000) {
      var k = rng.below(n);
      var kt = ec._truncateToN(k.clone(), true);               // what EC#sign multiplies by
      if (kt.cmpn(1) <= 0 || kt.cmp(n.subn(1)) >= 0) continue;
      var x = ec.g.mul(kt).getX();
      var j = x.div(n);
      var cls = j.isZero() ? 'j_0' : (j.cmpn(1) === 0 ? 'j_1' : 'j_ge_2');
      if (seen[cls]) continue;
      seen[cls] = true;
      var hh = rng.bytes(32);
      var s2 = signWith(ec, hh, 0, d, k);
      if ((s2.j >> 1) !== (j.isZero() ? 0 : 1)) throw new Error('recovery bit');
      expect(recVer(cls, hh, 0, s2.r, s2.s, qx, qy), 1);
    }
    if (!seen.j_0 || !seen.j_1) throw new Error(dom.name + ': no j >= 1 case');
  })();
  // msgBitLength shorter and longer than n, and the digest lengths
  [['msg_bits_short', nb, Math.max(1, nbits - 5)], ['msg_bits_long', nb, 8 * nb + 4], ['digest_20', 20, 0],
    ['digest_as_n', nb, 0], ['digest_64', 64, 0]].forEach(function(t) {
    var hh = rng.bytes(t[1]);
    var s3 = signWith(ec, hh, t[2], d, rng.below(n.subn(3)).addn(1));
    expect(recVer(t[0], hh, t[2], s3.r, s3.s, qx, qy), 1);
    if (t[2]) recVer(t[0] + '_read_as_0', hh, 0, s3.r, s3.s, qx, qy);
  });
  // keys off the curve: the tag only
  recVer('off_curve', h, 0, sg.r, sg.s, qx, qy.addn(1).umod(p), true);
  recVer('off_curve_zero', h, 0, sg.r, sg.s, new BN(0), new BN(0), true);
  recVer('off_curve_r_0', h, 0, new BN(0), sg.s, qx, qy.addn(1).umod(p), true);

  // ---- EC#sign ----
  function recDet(tag, hn, hh, bits, dd, c) {
    var o = { tag: tag, hash: hn, h: Buffer.from(hh).toString('hex'), bits: bits, d: hex32(dd), c: c };
    try {
      var s4 = ecs[hn].sign(Buffer.from(hh), dd.clone(), { canonical: !!c, msgBitLength: bits || undefined });
      o.r = hex32(s4.r); o.s = hex32(s4.s); o.j = s4.recoveryParam;
      if (small) throw new Error('EC#sign was expected to throw on ' + dom.name);
    } catch (e) {
      if (!small || !/Not enough entropy/.test(e.message)) throw e;
      o.msg = e.message;
    }
    det.push(o);
  }
  function recSup(tag, hh, bits, dd, k, c) {
    var o = { tag: tag, h: Buffer.from(hh).toString('hex'), bits: bits, d: hex32(dd), k: hex32(k), c: c };
    var mine = onePass(ec, Buffer.from(hh), bits, dd, k, c);
    var got;
    if (small) {
      got = mine;
    } else {
      try {
        var s5 = ec.sign(Buffer.from(hh), dd.clone(), { canonical: !!c, msgBitLength: bits || undefined,
          k: function(iter) { if (iter > 0) throw STOP; return k.clone(); } });
        got = { r: s5.r, s: s5.s, j: s5.recoveryParam };
      } catch (e) {
        if (e !== STOP) throw e;
        got = null;
      }
      if ((got === null) !== (mine === null) ||
          (got && (got.r.cmp(mine.r) || got.s.cmp(mine.s) || got.j !== mine.j)))
        throw new Error('the restated pass differs from EC#sign: ' + dom.name + ' ' + tag);
    }
    o.ok = got ? 1 : 0;
    if (got) { o.r = hex32(got.r); o.s = hex32(got.s); o.j = got.j; }
    sup.push(o);
  }
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
        var dd = rng.below(n);
        recDet(kd[0], hn, kd[1], kd[2], dd, cnt & 1);
        if (kd[0] === 'digest_as_n') recDet(kd[0], hn, kd[1], kd[2], dd, (cnt & 1) ^ 1);
        cnt++;
      });
    });
    var privs = [['priv_one', new BN(1)], ['priv_n_minus_1', n.subn(1)], ['priv_ge_n', n.addn(5)], ['priv_32_bytes', TOP.subn(3)]];
    privs.forEach(function(pv, i) {
      var hh = rng.bytes(nb);
      recDet(pv[0], HASHES[i % 3], hh, 0, pv[1], 0);
      recDet(pv[0], HASHES[(i + 1) % 3], hh, 0, pv[1], 1);
    });
  }
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
    recSup(kv[0], kd[1], kd[2], i === 3 ? TOP.subn(7) : (i === 6 ? n.addn(9) : rng.below(n)), kv[1], i & 1);
  });
  for (var i = 0; i < 4; i++) {
    var hh = rng.bytes(nb), dd = rng.below(n), k = rng.below(n);
    recSup('k_ordinary', hh, 0, dd, k, 0);
    recSup('k_ordinary', hh, 0, dd, k, 1);
  }
  var o = { name: dom.name, p: hex32(p), a: hex32(dom.a), d: hex32(dom.d), n: hex32(n), gx: hex32(dom.gx), gy: hex32(dom.gy),
    nbits: nbits, nbytes: nb, maxwell: curve._maxwellTrick ? 1 : 0, p_div_n: fl.toString(10), verify: ver, det: det, sup: sup };
  if (dom.found) o.curve_order = dom.found.order;
  return o;
}

var out = DOMAINS.map(gen);
var file = path.join(OUT, 'custom_ed_ecdsa.json');
fs.writeFileSync(file, JSON.stringify(out).replace(/\{"tag"/g, '\n{"tag"') + '\n');
out.forEach(function(c) {
  console.log(c.name + ': floor(p / n) = ' + c.p_div_n + ', ' + c.verify.length + ' EC#verify cases (' +
    c.verify.filter(function(v) { return v.ok; }).length + ' true), ' + c.det.length + ' EC#sign cases, ' +
    c.sup.length + ' supplied nonces (' + c.sup.filter(function(d) { return d.ok; }).length + ' accepted)');
});
console.log('wrote ' + file);
