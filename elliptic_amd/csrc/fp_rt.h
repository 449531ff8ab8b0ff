// ellgpu -- prime field with a RUN-TIME modulus (any odd p < 2^256), Montgomery form, for
// user-defined short Weierstrass curves: `new elliptic.curve.short({p, a, b, ...})` with a prime
// and coefficients of the caller's choosing (lib/elliptic/curve/short.js:11-24; bn.js gives such
// curves its generic `Mont` / `Red` contexts, dist/elliptic.js:7078-7381).  The presets' fields
// (fp.h) have their moduli as compile-time constants; here the modulus, the Montgomery
// constants and the curve's a, b come from one parameter block:
//   device  `__constant__ RtField g_rt` of the translation unit that holds the custom-curve
//           kernels (inst.hip group 16), uploaded on the call's stream before the launches;
//           scalar loads, so the limbs of p sit in SGPRs like the presets' literals do
//   host    (tests/hostsim) a plain global.
// One block per DEVICE: a call on a user-defined curve takes that device's lock, uploads the
// curve's block, and waits for its own device work before releasing the lock (Engine::CustomScope,
// engine.h) -- such calls are synchronous and serialised per device, whatever stream they name.
//
// Square root (Red#sqrt, dist/elliptic.js:7177-7232), for ShortCurve#pointFromX and the
// compressed SEC1 encodings on user-defined curves: the block carries the constants that depend
// on the modulus alone -- p - 1 = q 2^s, the exponent, c = z^q for a quadratic non-residue z --
// computed on the host when the curve is defined (rt_define.h rt_sqrt_init).  p = 3 (mod 4): one
// exponentiation a^((p+1)/4).  Otherwise Tonelli-Shanks, with the reference's inner search for
// the order of t replaced by a schedule that s alone fixes: s - 1 rounds, round k squares t
// k - 1 times and applies the correction under a per-lane select.  Every loop bound is read from
// the block (wave-uniform), so the root terminates for any input and any modulus; a value without
// a root comes back as something whose square differs, which the caller's y^2 == rhs test
// (Work::lift_x) reports -- as 'invalid point' where p = 3 (mod 4), as the 'Assertion failed' of
// bn.js's own loop (assert(i < m), dist/elliptic.js:7217-7229) where Tonelli-Shanks runs.
#pragma once

#include "fp.h"

namespace ell {

struct RtField {
  u32 p[8];        // modulus
  u32 n0;          // -p^-1 mod 2^32
  u32 one[8];      // R mod p          (R = 2^256)
  u32 r2[8];       // R^2 mod p
  u32 pm2[8];      // p - 2            (Fermat inversion)
  u32 a_m[8];      // curve coefficient a, Montgomery form
  u32 b_m[8];      // curve coefficient b, Montgomery form
  u32 a_kind;      // 0: a == 0, 3: a == p - 3, 1: anything else
  u32 d_m[8];      // Edwards curves (edcustom.h): coefficient d, Montgomery form; a_m holds a
  u32 kind;        // 0: short Weierstrass (a_m, b_m), 1: (twisted) Edwards with c = 1 (a_m, d_m),
                   // 2: Montgomery (montcustom.h), which REUSES fields of the other kinds -- the
                   //    block's size and layout are pinned, and a Montgomery curve needs neither a
                   //    Weierstrass b nor a square root:
                   //      a_m         the curve's a, Montgomery form
                   //      b_m         a24 = (a + 2) / 4 mod p, Montgomery form (the curve's own b
                   //                  enters no formula of the reference and is not stored)
                   //      sqrt_e      (p - 1) / 2: Euler's criterion through pow_sqrt_e
                   //      sqrt_ebits  its bit length
                   //      sqrt_kind   0: p = 3 (mod 4), 1: p = 1 (mod 4) -- what MontCurve#validate
                   //                  answers on a non-residue (false / 'Assertion failed')
                   //      pbytes      p.byteLength()
                   //    a_kind, d_m, sqrt_s, sqrt_c and the domain fields stay zero
  // ECDSA domain (ellgpu_curve_define_short_domain): the order n and the generator G.  Zero for a
  // plain curve, so that a domain and the plain curve with the same (p, a, b) are different blocks.
  u32 domain;      // 1: the fields below are set
  u32 n[8];        // order
  u32 nn0;         // -n^-1 mod 2^32
  u32 n_one[8];    // R mod n
  u32 n_r2[8];     // R^2 mod n
  u32 nm2[8];      // n - 2            (Fermat inversion mod n)
  u32 nbits;       // n.bitLength()    (_truncateToN's shift is the host's)
  u32 n_p[8];      // n mod p, Montgomery form (JPoint#eqXToP's redN)
  u32 ncand;       // floor(p / n) when <= 100 (_maxwellTrick: eqXToP's further candidates), else RT_NO_MAXWELL
  u32 gx[8];       // G, plain
  u32 gy[8];
  // Red#sqrt (a function of p alone; zero for an Edwards curve, which never takes a root)
  u32 sqrt_kind;   // 0: p = 3 (mod 4), a^((p+1)/4); 1: Tonelli-Shanks
  u32 sqrt_s;      // 2-adicity of p - 1:  p - 1 = q 2^s, q odd
  u32 sqrt_ebits;  // bitLength of sqrt_e
  u32 sqrt_e[8];   // (p + 1) / 4  or  (q - 1) / 2
  u32 sqrt_c[8];   // z^q for a quadratic non-residue z, Montgomery form (Tonelli-Shanks only)
  u32 pbytes;      // p.byteLength(): the width of a SEC1 coordinate (BaseCurve#decodePoint)
};

constexpr u32 RT_NO_MAXWELL = 0xFFFFFFFFu;

#if defined(__HIP_DEVICE_COMPILE__)
// one block per code object: each translation unit that holds custom-curve kernels names its own
// (inst.hip; Engine::CustomScope uploads to every one)
#ifndef ELL_RT_SYMBOL
#define ELL_RT_SYMBOL g_rt
#endif
extern __constant__ RtField ELL_RT_SYMBOL;
#define ELL_RT (ELL_RT_SYMBOL)
#else
inline RtField& rt_host_block() { static RtField f; return f; }
#define ELL_RT (rt_host_block())
#endif

// MOD = 0: the base field (p); MOD = 1: the scalar field of an ECDSA domain (n) -- the same
// Montgomery arithmetic over the other modulus of the block
template <int MOD>
struct FpMontRTm {
  static constexpr int L = 8;
  typedef Fe<8> El;
  static constexpr bool HAS_SQRT = true;       // Red#sqrt of a generic prime: sqrt() below (base field only)

  ELL_HD static void get_p(u32 (&p)[8]) {
    ELL_UNROLL
    for (int i = 0; i < 8; i++) p[i] = MOD ? ELL_RT.n[i] : ELL_RT.p[i];
  }
  ELL_HD static El zero() { El r; bn_zero<8>(r.v); return r; }
  ELL_HD static El one() {
    El r;
    ELL_UNROLL
    for (int i = 0; i < 8; i++) r.v[i] = MOD ? ELL_RT.n_one[i] : ELL_RT.one[i];
    return r;
  }
  ELL_HD static El curve_a() {
    El r;
    ELL_UNROLL
    for (int i = 0; i < 8; i++) r.v[i] = ELL_RT.a_m[i];
    return r;
  }
  ELL_HD static El curve_b() {
    El r;
    ELL_UNROLL
    for (int i = 0; i < 8; i++) r.v[i] = ELL_RT.b_m[i];
    return r;
  }
  ELL_HD static bool is_zero(const El& a) { return bn_is_zero<8>(a.v); }
  ELL_HD static bool eq(const El& a, const El& b) { return bn_eq<8>(a.v, b.v); }
  ELL_HD static El add(const El& a, const El& b) {
    u32 p[8]; get_p(p);
    El r; mod_add<8>(r.v, a.v, b.v, p); return r;
  }
  ELL_HD static El sub(const El& a, const El& b) {
    u32 p[8]; get_p(p);
    El r; mod_sub<8>(r.v, a.v, b.v, p); return r;
  }
  ELL_HD static El neg(const El& a) { return sub(zero(), a); }
  ELL_HD static El dbl(const El& a) { return add(a, a); }
  template <int K>
  ELL_HD static El mul_pow2(const El& a) {
    El r = dbl(a);
    ELL_UNROLL
    for (int i = 1; i < K; i++) r = dbl(r);
    return r;
  }
  // Montgomery reduction of a 16-limb value (row-wise, explicit carry chains; FpMont::redc with the
  // modulus read from the parameter block)
  ELL_HD static El redc(u32 (&t)[16]) {
    u32 p[8]; get_p(p);
    const u32 n0 = MOD ? ELL_RT.nn0 : ELL_RT.n0;
    u32 top = 0;
    ELL_UNROLL
    for (int i = 0; i < 8; i++) {
      u32 m = t[i] * n0;
      u32 lo[8], hi[8];
      ELL_UNROLL
      for (int j = 0; j < 8; j++) {
        u64 x = (u64)m * p[j];
        lo[j] = (u32)x;
        hi[j] = (u32)(x >> 32);
      }
      u32 u[9];
      u32 c = 0;
      u[0] = lo[0];
      ELL_UNROLL
      for (int j = 1; j < 8; j++) u[j] = addc32(lo[j], hi[j - 1], c, c);
      u[8] = hi[7] + c;
      c = 0;
      ELL_UNROLL
      for (int j = 0; j < 8; j++) t[i + j] = addc32(t[i + j], u[j], c, c);
      u32 c1, c2;
      u32 y = addc32(t[i + 8], u[8], c, c1);
      t[i + 8] = addc32(y, 0, top, c2);
      top = c1 + c2;
    }
    u32 r[8], sres[8];
    ELL_UNROLL
    for (int i = 0; i < 8; i++) r[i] = t[8 + i];
    u32 br = bn_sub<8>(sres, r, p);
    El out;
    bn_select<8>(out.v, (top != 0) || (br == 0), sres, r);
    return out;
  }
  ELL_HD static El mul(const El& a, const El& b) {
    u32 t[16];
    fe_mul_wide<8>(t, a.v, b.v);
    return redc(t);
  }
  ELL_HD static El sqr(const El& a) {
    u32 t[16];
    fe_sqr_wide<8>(t, a.v);
    return redc(t);
  }
  ELL_HD static El sqr_n(El a, int n) {
    ELL_NOUNROLL
    for (int i = 0; i < n; i++) a = sqr(a);
    return a;
  }
  ELL_HD static El from_plain(const u32 (&a)[8]) {       // a < 2^256 (possibly >= p): a * R mod p
    El x, r2;
    bn_copy<8>(x.v, a);
    ELL_UNROLL
    for (int i = 0; i < 8; i++) r2.v[i] = MOD ? ELL_RT.n_r2[i] : ELL_RT.r2[i];
    return mul(x, r2);
  }
  ELL_HD static void to_plain(u32 (&r)[8], const El& a) {
    El o; bn_zero<8>(o.v); o.v[0] = 1;
    El x = mul(a, o);
    bn_copy<8>(r, x.v);
  }
  ELL_HD static bool is_odd(const El& a) { u32 r[8]; to_plain(r, a); return r[0] & 1; }
  // a^(p-2): a^-1, 0 for 0 (the exponent is wave-uniform: a scalar branch per bit).  inv_inl is
  // the loop itself, inlined into its caller: a kernel that calls inv pays a call frame in scratch
  // memory for the two elements passed by reference, one that is to run without scratch takes inv_inl.
  ELL_HD static El inv_inl(const El& a) {
    El r = one();
    ELL_NOUNROLL
    for (int i = 255; i >= 0; i--) {
      r = sqr(r);
      if (((MOD ? ELL_RT.nm2[i >> 5] : ELL_RT.pm2[i >> 5]) >> (i & 31)) & 1u) r = mul(r, a);
    }
    return r;
  }
  static ELL_HD_NOINLINE El inv(const El& a) { return inv_inl(a); }
  // a^e for the block's square-root exponent (wave-uniform: a scalar branch per bit)
  ELL_HD static El pow_sqrt_e(const El& a) {
    El r = one();
    ELL_NOUNROLL
    for (int i = (int)ELL_RT.sqrt_ebits - 1; i >= 0; i--) {
      r = sqr(r);
      if ((ELL_RT.sqrt_e[i >> 5] >> (i & 31)) & 1u) r = mul(r, a);
    }
    return r;
  }
  // Red#sqrt: a root of a where it has one (either of the two: pointFromX fixes the sign by
  // parity), 0 for 0, otherwise a value whose square is not a.  Base field only.
  static ELL_HD_NOINLINE El sqrt(const El& a) {
    static_assert(MOD == 0, "square roots are the base field's");
    El w = pow_sqrt_e(a);
    if (ELL_RT.sqrt_kind == 0) return w;                   // a^((p+1)/4)
    // Tonelli-Shanks: r = a^((q+1)/2), t = a^q, c = z^q of order 2^s.  Invariant of round k:
    // r^2 = a t, c has order 2^(k+1), and t^(2^k) = 1 when a is a residue -- so t^(2^(k-1)) is 1
    // or -1, and in the second case r c, t c^2 restore the invariant for k - 1.
    El r = mul(a, w);
    El t = mul(r, w);
    El c;
    ELL_UNROLL
    for (int i = 0; i < 8; i++) c.v[i] = ELL_RT.sqrt_c[i];
    const El o = one();
    ELL_NOUNROLL
    for (int k = (int)ELL_RT.sqrt_s - 1; k >= 1; k--) {
      El u = t;
      ELL_NOUNROLL
      for (int j = 1; j < k; j++) u = sqr(u);
      const bool fix = !eq(u, o);
      const El rc = mul(r, c);
      c = sqr(c);
      const El tc = mul(t, c);
      bn_select<8>(r.v, fix, rc.v, r.v);
      bn_select<8>(t.v, fix, tc.v, t.v);
    }
    return r;
  }
};
typedef FpMontRTm<0> FpMontRT;       // base field of a user-defined curve
typedef FpMontRTm<1> FpMontRTn;      // order field of a user-defined ECDSA domain

}  // namespace ell
