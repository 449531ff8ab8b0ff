'use strict';
// Golden vectors for EC#recoverPubKey on user-defined ECDSA domains (ellgpu_custom_recover): every
// status, point and thrown message from the reference itself.  Runs only where the reference is
// present (see tools/ref_loader.js); all randomness is SHA-256 counter mode over a fixed seed and
// the reference's signatures are its deterministic (RFC 6979) ones, so a rerun reproduces
// tests/golden/custom_recover.json byte for byte.
//
//   node tools/gen_golden_custom_recover.js [outdir]
//
// Domains: the six of custom_wire.json -- brainpoolP256r1, secp192k1, secp112r1 (p = 3 mod 4),
// secp224k1 (n > p, p = 5 mod 8), w25519_like (cofactor 8), p224_user (p - 1 = q 2^96).
//
// `recover`: h = the digest (hex, 1..64 bytes; e = new BN(h), not truncated), r, s (64 hex digits),
// j = the recovery parameter -> st:
//   0  a point, with x, y (64 hex digits)
//   1  the point at infinity
//   2  the reference throws, with msg
//   3  r = 0 or r >= n: outside the engine's domain whatever the reference does with it (BN#invm
//      of an unreduced value); nothing else is recorded
// tag = what the case exercises.

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
Prng.prototype.bits = function(b) { return new BN(this.bytes(Math.ceil(b / 8))).maskn(b); };
Prng.prototype.below = function(n) {            // uniform-ish in [1, n)
  for (;;) {
    var k = this.bits(n.bitLength()).umod(n);
    if (!k.isZero()) return k;
  }
};

function hex32(bn) { return bn.toString(16, 64); }

var W25519 = { p: '7fffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffed',
  a: '2aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa984914a144',
  b: '7b425ed097b425ed097b425ed097b425ed097b425ed097b4260b5e9c7710c864' };

var CURVES = [
  { name: 'brainpoolP256r1',
    p: 'a9fb57dba1eea9bc3e660a909d838d726e3bf623d52620282013481d1f6e5377',
    a: '7d5a0975fc2c3057eef67530417affe7fb8055c126dc5c6ce94a4b44f330b5d9',
    b: '26dc5c6ce94a4b44f330b5d9bbd77cbf958416295cf7e1ce6bccdc18ff8c07b6',
    g: ['8bd2aeb9cb7e57cb2c4b482ffc81b7afb9de27e1e3bd23c23a4453bd9ace3262',
      '547ef835c3dac4fd97f8461a14611dc9c27745132ded8e545c1d54c72f046997'],
    n: 'a9fb57dba1eea9bc3e660a909d838d718c397aa3b561a6f7901e0e82974856a7' },
  { name: 'secp192k1', p: 'fffffffffffffffffffffffffffffffffffffffeffffee37', a: '0', b: '3',
    g: ['db4ff10ec057e9ae26b07d0280b7f4341da5d1b1eae06c7d', '9b2f2f6d9c5628a7844163d015be86344082aa88d95e2f9d'],
    n: 'fffffffffffffffffffffffe26f2fc170f69466a74defd8d' },
  { name: 'secp112r1', p: 'db7c2abf62e35e668076bead208b', a: 'db7c2abf62e35e668076bead2088',
    b: '659ef8ba043916eede8911702b22', g: ['09487239995a5ee76b55f9c2f098', 'a89ce5af8724c0a23e0e0ff77500'],
    n: 'db7c2abf62e35e7628dfac6561c5' },
  { name: 'secp224k1', p: 'fffffffffffffffffffffffffffffffffffffffffffffffeffffe56d', a: '0', b: '5',
    g: ['a1455b334df099df30fc28a169a467e9e47075a90f7e650eb6b7a45c',
      '7e089fed7fba344282cafbd6f7e319f7c0b0bd59e2ca4bdb556d61a5'],
    n: '010000000000000000000000000001dce8d2ec6184caf0a971769fb1f7' },
  { name: 'w25519_like', p: W25519.p, a: W25519.a, b: W25519.b,
    n: new BN(1).ushln(252).add(new BN('27742317777372353535851937790883648493', 10)).toString(16) },
  // NIST P-224 (FIPS 186-4 D.1.2.2) given as a user-defined curve: the generic Mont context
  { name: 'p224_user', p: 'ffffffffffffffffffffffffffffffff000000000000000000000001',
    a: 'fffffffffffffffffffffffffffffffefffffffffffffffffffffffe',
    b: 'b4050a850c04b3abf54132565044b0b7d7bfd8ba270b39432355ffb4',
    g: ['b70e0cbd6bb4bf7f321390b94a03c1d356c21122343280d6115c1d21',
      'bd376388b5f723fb4c22dfe6cd4375a05a07476444d5819985007e34'],
    n: 'ffffffffffffffffffffffffffff16a2e0b8f03e13dd29455c5c2a3d' },
];

function build(spec) {
  var g = spec.g;
  if (!g) {
    // 8 * (the first point with a small x): a generator of the order-n subgroup
    var c = new elliptic.curve.short({ p: spec.p, a: spec.a, b: spec.b });
    var P;
    for (var x = 1; ; x++) {
      try { P = c.pointFromX(new BN(x), false); } catch (e) { continue; }
      P = P.mul(new BN(8));
      if (!P.isInfinity()) break;
    }
    g = [P.getX().toString(16), P.getY().toString(16)];
  }
  var pc = new elliptic.curves.PresetCurve({ type: 'short', prime: null, p: spec.p, a: spec.a, b: spec.b,
    n: spec.n, hash: hash.sha256, gRed: false, g: g });
  return new elliptic.ec(pc);
}

var THROWN = ['Unable to find sencond key candinate', 'invalid point', 'Assertion failed',
  'The recovery param is more than two bits'];

function genRecover(spec, ec, rng) {
  var curve = ec.curve, G = ec.g, n = ec.n, p = curve.p;
  var pmn = p.umod(n);
  var out = [];
  function rec(tag, h, r, s, j) {
    var c = { tag: tag, h: Buffer.from(h).toString('hex'), r: hex32(r), s: hex32(s), j: j };
    if (r.isZero() || r.cmp(n) >= 0) {
      c.st = 3;
    } else {
      try {
        var Q = ec.recoverPubKey(Buffer.from(h), { r: r.clone(), s: s.clone() }, j);
        if (Q.isInfinity()) {
          c.st = 1;
        } else {
          c.st = 0;
          c.x = hex32(Q.getX());
          c.y = hex32(Q.getY());
        }
      } catch (e) {
        if (THROWN.indexOf(e.message) < 0) throw e;
        c.st = 2;
        c.msg = e.message;
      }
    }
    out.push(c);
    return c;
  }
  function all4(tag, h, r, s) { for (var j = 0; j < 4; j++) rec(tag, h, r, s, j); }
  // the reference's own signatures over digests of at most n.bitLength() bits (signing truncates,
  // recovery does not: with such a digest both see the same e); every j, 4 and 5 included.  Where
  // the reference cannot sign (HmacDRBG wants 192 bits of key: secp112r1) the same equations with
  // a nonce from the seeded stream.
  var dlen = Math.floor(n.bitLength() / 8);
  function sign(kp, h) {
    try {
      var sg = kp.sign(h);
      return { r: sg.r, s: sg.s, j: sg.recoveryParam };
    } catch (e) {
      if (!/entropy/.test(e.message)) throw e;
      var m = new BN(h).umod(n);
      for (;;) {
        var k = rng.below(n);
        var R = G.mul(k);
        var r = R.getX().umod(n);
        var s = k.invm(n).mul(m.add(kp.getPrivate().mul(r))).umod(n);
        if (r.isZero() || s.isZero()) continue;
        return { r: r, s: s, j: (R.getY().isOdd() ? 1 : 0) | (R.getX().cmp(r) !== 0 ? 2 : 0) };
      }
    }
  }
  var i, j, found = 0;
  for (i = 0; i < 4; i++) {
    var kp = ec.keyFromPrivate(rng.below(n));
    var h = rng.bytes(dlen);
    var sg = sign(kp, h);
    for (j = 0; j < 6; j++) {
      var c = rec(j === sg.j ? 'signed' : 'signed_other_j', h, sg.r, sg.s, j);
      // on a cofactor curve x = r also belongs to points outside the subgroup, and pointFromX
      // may pick one of those: the signer's key then does not come back, in the reference either
      if (j === sg.j && c.st === 0 && c.x === hex32(kp.getPublic().getX()) && c.y === hex32(kp.getPublic().getY()))
        found++;
    }
    if (i === 0) {
      // s = 0 and s >= n: not range-checked, reduced by the arithmetic
      all4('s_zero', h, sg.r, new BN(0));
      rec('s_is_n', h, sg.r, n.clone(), sg.j);
      rec('s_plus_n', h, sg.r, sg.s.add(n).bitLength() <= 256 ? sg.s.add(n) : n.addn(5), sg.j);
      rec('s_all_ones', h, sg.r, new BN(1).ushln(256).subn(1), sg.j);
      // e = 0 (mod n), e = n, a 64-byte all-ones digest, a 1-byte digest
      rec('e_zero', [0], sg.r, sg.s, sg.j);
      rec('e_zero_32', Buffer.alloc(32), sg.r, sg.s, sg.j);
      rec('e_is_n', n.toArray('be', 32), sg.r, sg.s, sg.j);
      rec('e_is_2n_64', n.muln(2).toArray('be', 64), sg.r, sg.s, sg.j);
      all4('e_all_ones_64', Buffer.alloc(64, 0xff), sg.r, sg.s);
      rec('e_one_byte', [0xa7], sg.r, sg.s, sg.j);
      rec('e_one_byte', [0xa7], sg.r, sg.s, sg.j ^ 1);
      rec('e_sha512', rng.bytes(64), sg.r, sg.s, sg.j);
      rec('e_33_bytes', rng.bytes(33), sg.r, sg.s, sg.j ^ 1);
    }
  }
  // r out of range
  var h0 = rng.bytes(dlen), s0 = rng.below(n);
  [new BN(0), n.clone(), n.addn(1), new BN(1).ushln(256).subn(1)].forEach(function(r) {
    rec('r_range', h0, r, s0, 0);
    rec('r_range', h0, r, s0, 3);
    rec('r_range', h0, r, s0, 4);
  });
  // the second candidate, built on purpose (a random r never lands below a 128-bit p mod n):
  // r below p mod n, and around it
  for (i = 0; i < 4; i++) {
    var rs = rng.below(pmn);
    if (rs.cmp(n) >= 0) rs = rs.umod(n).iaddn(1);
    var hs = rng.bytes(dlen), ss = rng.below(n);
    rec('second_small_r', hs, rs, ss, 2);
    rec('second_small_r', hs, rs, ss, 3);
    rec('second_small_r', hs, rs, ss, i & 1);
  }
  [pmn.subn(1), pmn.clone(), pmn.addn(1), new BN(1), new BN(2), new BN(3), new BN(4)].forEach(function(r) {
    all4('r_near_p_mod_n', h0, r, s0);
  });
  // n > p: r in [p, n) stands for x = r - p; r + n needs two subtractions of p
  if (n.cmp(p) > 0) {
    [p.subn(1), p.clone(), p.addn(2), n.subn(1)].forEach(function(r) {
      all4('r_near_p', h0, r, s0);
    });
  }
  // random (r, s, j)
  for (i = 0; i < 8; i++) rec('random', rng.bytes(1 + (i * 9) % 64), rng.below(n), rng.below(n), i % 6);
  // infinity: R = k G with x(R) < n, s arbitrary and e = s k, so that s R - e G = 0
  for (i = 0; i < 2;) {
    var k = rng.below(n), R = G.mul(k);
    if (R.getX().cmp(n) >= 0 || R.getX().isZero()) continue;
    var si = rng.below(n);
    rec('infinity', si.mul(k).umod(n).toArray('be', 32), R.getX(), si, R.getY().isOdd() ? 1 : 0);
    i++;
  }
  return { rows: out, found: found };
}

function gen(spec) {
  var rng = new Prng('ellgpu-golden-v1:custom-recover:' + spec.name);
  var ec = build(spec);
  var curve = ec.curve;
  var o = { name: spec.name, p: hex32(curve.p), a: hex32(curve.a.fromRed()), b: hex32(curve.b.fromRed()),
    n: hex32(ec.n), g: { x: hex32(ec.g.getX()), y: hex32(ec.g.getY()) }, p_div_n: curve.p.div(ec.n).toNumber(),
    p_mod_n: hex32(curve.p.umod(ec.n)) };
  var g = genRecover(spec, ec, rng);
  o.recover = g.rows;
  return { o: o, found: g.found };
}

var res = CURVES.map(gen);
var out = res.map(function(r) { return r.o; });
var file = path.join(OUT, 'custom_recover.json');
fs.writeFileSync(file, JSON.stringify(out).replace(/\{"tag"/g, '\n{"tag"') + '\n');
res.forEach(function(r) {
  var c = r.o, st = [0, 0, 0, 0], msgs = {};
  c.recover.forEach(function(d) { st[d.st]++; if (d.msg) msgs[d.msg] = (msgs[d.msg] || 0) + 1; });
  console.log(c.name + ': ' + c.recover.length + ' cases (status 0/1/2/3: ' + st.join('/') + '), signer recovered ' +
    r.found + ' of 4; thrown: ' + JSON.stringify(msgs));
});
console.log('wrote ' + file);
