// ellgpu -- definition of a user-defined curve: host arithmetic modulo any odd m < 2^256 and the
// parameter block (fp_rt.h RtField) of a short curve, an ECDSA domain on it, an Edwards curve or a
// Montgomery curve.
// Host only, no engine: Engine::define_* forward a refusal to fail() and register the block.
// Engine::register_custom compares blocks byte for byte (same parameters, same id): every builder
// starts from a zeroed block and writes each member as a function of the parameters alone.
#pragma once

#include <string.h>

#include "fp.h"
#include "fp_rt.h"

namespace ell {

enum { E_OK = 0, E_NODEVICE = -1, E_ARG = -2, E_HIP = -3, E_NOMEM = -4, E_UNSUPPORTED = -5 };

struct RtStatus { int code; const char* msg; };   // E_OK, or a refusal and its message (a literal)

// bit by bit: a definition is rare; these are not hot
inline void mod_times_r(const u32 (&m)[8], u32 (&r)[8]) {        // r * 2^256 mod m, r < m
  for (int i = 0; i < 256; i++) {
    u32 t[8];
    mod_add<8>(t, r, r, m);
    bn_copy<8>(r, t);
  }
}
// out = x mod m for any x < 2^256
inline void mod_reduce(const u32 (&m)[8], u32 (&out)[8], const u32 (&x)[8]) {
  u32 r[8];
  bn_zero<8>(r);
  for (int i = 255; i >= 0; i--) {
    u32 t[8];
    mod_add<8>(t, r, r, m);
    bn_copy<8>(r, t);
    if ((x[i >> 5] >> (i & 31)) & 1u) {
      u32 o[8];
      bn_zero<8>(o);
      o[0] = 1;
      mod_add<8>(t, r, o, m);
      bn_copy<8>(r, t);
    }
  }
  bn_copy<8>(out, r);
}
// out = x * 2^256 mod m for any x < 2^256 (reduced bit by bit first)
inline void mod_to_mont(const u32 (&m)[8], u32 (&out)[8], const u32 (&x)[8]) {
  u32 r[8];
  mod_reduce(m, r, x);
  mod_times_r(m, r);
  bn_copy<8>(out, r);
}
// out = a * b mod m, a and b < m
inline void mod_mul(const u32 (&m)[8], u32 (&out)[8], const u32 (&a)[8], const u32 (&b)[8]) {
  u32 r[8];
  bn_zero<8>(r);
  for (int i = 255; i >= 0; i--) {
    u32 t[8];
    mod_add<8>(t, r, r, m);
    bn_copy<8>(r, t);
    if ((b[i >> 5] >> (i & 31)) & 1u) {
      mod_add<8>(t, r, a, m);
      bn_copy<8>(r, t);
    }
  }
  bn_copy<8>(out, r);
}
// out = a^e mod m, a < m
inline void mod_pow(const u32 (&m)[8], u32 (&out)[8], const u32 (&a)[8], const u32 (&e)[8]) {
  u32 r[8], o[8];
  bn_zero<8>(o);
  o[0] = 1;
  mod_reduce(m, r, o);
  for (int i = 255; i >= 0; i--) {
    mod_mul(m, r, r, r);
    if ((e[i >> 5] >> (i & 31)) & 1u) mod_mul(m, r, r, a);
  }
  bn_copy<8>(out, r);
}
// the Montgomery constants of a modulus m: -m^-1 mod 2^32, R mod m, R^2 mod m, m - 2
inline void mont_consts(const u32 (&m)[8], u32& n0, u32 (&one)[8], u32 (&r2)[8], u32 (&mm2)[8]) {
  u32 inv = 1;                                          // m^-1 mod 2^32 (Newton)
  for (int i = 0; i < 5; i++) inv *= 2u - m[0] * inv;
  n0 = 0u - inv;
  u32 o[8];
  bn_zero<8>(o);
  o[0] = 1;
  mod_to_mont(m, one, o);
  bn_copy<8>(r2, one);
  mod_times_r(m, r2);
  u32 two[8];
  bn_zero<8>(two);
  two[0] = 2;
  bn_sub<8>(mm2, m, two);
}
inline int bit_length(const u32 (&x)[8]) {
  int nb = 256;
  while (nb > 0 && !((x[(nb - 1) >> 5] >> ((nb - 1) & 31)) & 1u)) nb--;
  return nb;
}

// modulus-dependent constants of a parameter block
inline RtStatus rt_field_init(RtField& f, const u8* p_be) {
  memset(&f, 0, sizeof(f));
  load_be<8>(f.p, p_be, 32);
  if (!(f.p[0] & 1u)) return {E_ARG, "user-defined curve: the modulus must be odd"};
  bool small = true;
  for (int i = 1; i < 8; i++) small = small && f.p[i] == 0;
  if (small && f.p[0] < 5) return {E_ARG, "user-defined curve: the modulus must be a prime > 3"};
  mont_consts(f.p, f.n0, f.one, f.r2, f.pm2);
  return {E_OK, nullptr};
}
// Red#sqrt's constants of a block's modulus (fp_rt.h) and p.byteLength().  Deterministic: z is
// the LEAST quadratic non-residue (Euler's criterion, candidates 2 .. 255), so that the same
// parameters always give the same block.  A modulus without such a z is no prime; its block gets
// c = 0 and its roots are outside the documented domain, like its inverses.
inline void rt_sqrt_init(RtField& f) {
  f.pbytes = (u32)((bit_length(f.p) + 7) / 8);
  auto shr = [](u32 (&x)[8], int k) {
    for (int i = 0; i < 8; i++) x[i] = (x[i] >> k) | (i + 1 < 8 ? x[i + 1] << (32 - k) : 0u);
  };
  u32 one[8];
  bn_zero<8>(one);
  one[0] = 1;
  bn_copy<8>(f.sqrt_e, f.p);
  if ((f.p[0] & 3u) == 3u) {
    f.sqrt_kind = 0;
    f.sqrt_s = 1;
    shr(f.sqrt_e, 2);                                   // (p + 1) / 4 = (p >> 2) + 1
    bn_add<8>(f.sqrt_e, f.sqrt_e, one);
  } else {
    f.sqrt_kind = 1;
    u32 q[8], half[8], pm1[8];
    bn_sub<8>(pm1, f.p, one);
    bn_copy<8>(q, pm1);
    f.sqrt_s = 0;
    while (!(q[0] & 1u)) { shr(q, 1); f.sqrt_s++; }
    bn_copy<8>(f.sqrt_e, q);
    shr(f.sqrt_e, 1);                                   // (q - 1) / 2
    bn_copy<8>(half, pm1);
    shr(half, 1);
    for (u32 z = 2; z < 256; z++) {
      u32 zz[8], t[8];
      bn_zero<8>(zz);
      zz[0] = z;
      if (bn_geq<8>(zz, f.p)) break;
      mod_pow(f.p, t, zz, half);
      if (!bn_eq<8>(t, pm1)) continue;
      mod_pow(f.p, t, zz, q);
      mod_to_mont(f.p, f.sqrt_c, t);
      break;
    }
  }
  f.sqrt_ebits = (u32)bit_length(f.sqrt_e);
}

// The block of a Montgomery curve (kind 2; fp_rt.h documents the fields it reuses): a24 =
// (a + 2) / 4 where the short curve's b sits, (p - 1) / 2 and p mod 4 where Red#sqrt's constants sit
inline void rt_mont_init(RtField& f, const u32 (&a_m)[8]) {
  u32 two[8], t[8];
  bn_zero<8>(two);
  two[0] = 2;
  mod_to_mont(f.p, two, two);
  mod_add<8>(t, a_m, two, f.p);
  for (int h = 0; h < 2; h++) {                         // t / 2 mod p, twice: (t + p) / 2 for an odd t
    u32 c = 0;
    if (t[0] & 1u) c = bn_add<8>(t, t, f.p);
    for (int i = 0; i < 8; i++) t[i] = (t[i] >> 1) | ((i + 1 < 8 ? t[i + 1] : c) << 31);
  }
  bn_copy<8>(f.b_m, t);
  bn_copy<8>(f.sqrt_e, f.p);
  for (int i = 0; i < 8; i++) f.sqrt_e[i] = (f.p[i] >> 1) | (i + 1 < 8 ? f.p[i + 1] << 31 : 0u);   // (p - 1) / 2
  f.sqrt_ebits = (u32)bit_length(f.sqrt_e);
  f.sqrt_kind = (f.p[0] & 3u) == 1u ? 1u : 0u;
  f.pbytes = (u32)((bit_length(f.p) + 7) / 8);
  f.kind = 2;
}
// parameter block of a user-defined curve (edwards = 0: short Weierstrass, b; 1: Edwards, d; 2:
// Montgomery, bd_be unused): p an odd prime < 2^256 (primality is the caller's business, as it is
// the reference's), a and b / d any residues
inline RtStatus rt_build_custom(int edwards, const u8* p_be, const u8* a_be, const u8* bd_be, RtField& f) {
  if (!p_be || !a_be || (!bd_be && edwards != 2)) return {E_ARG, "null pointer"};
  if (edwards == 2) {
    const RtStatus st = rt_field_init(f, p_be);
    if (st.code) return st;
    u32 a[8];
    load_be<8>(a, a_be, 32);
    mod_to_mont(f.p, f.a_m, a);
    rt_mont_init(f, f.a_m);
    return {E_OK, nullptr};
  }
  const RtStatus st = rt_field_init(f, p_be);
  if (st.code) return st;
  u32 a[8], b[8];
  load_be<8>(a, a_be, 32);
  load_be<8>(b, bd_be, 32);
  mod_to_mont(f.p, f.a_m, a);
  if (!edwards) {
    mod_to_mont(f.p, f.b_m, b);
    u32 three[8], m3[8];
    bn_zero<8>(three);
    three[0] = 3;
    bn_sub<8>(m3, f.p, three);
    mod_to_mont(f.p, m3, m3);
    f.a_kind = bn_is_zero<8>(f.a_m) ? 0u : (bn_eq<8>(f.a_m, m3) ? 3u : 1u);
    f.kind = 0;
    rt_sqrt_init(f);
  } else {
    mod_to_mont(f.p, f.d_m, b);
    if (bn_is_zero<8>(f.a_m) || bn_is_zero<8>(f.d_m) || bn_eq<8>(f.a_m, f.d_m))
      return {E_ARG, "user-defined Edwards curve: a and d must be non-zero and distinct"};
    f.kind = 1;
  }
  return {E_OK, nullptr};
}
// the domain fields of a block whose curve is built: the order n (odd, >= 3) and the generator
// (coordinates < p), the same for a short and an Edwards domain
inline bool rt_order_ok(const u32 (&n)[8]) {
  bool small = true;
  for (int i = 1; i < 8; i++) small = small && n[i] == 0;
  return (n[0] & 1u) && !(small && n[0] < 3);
}
inline void rt_fill_domain(RtField& f, const u32 (&n)[8], const u32 (&gx)[8], const u32 (&gy)[8]) {
  f.domain = 1;
  bn_copy<8>(f.n, n);
  mont_consts(n, f.nn0, f.n_one, f.n_r2, f.nm2);
  f.nbits = (u32)bit_length(n);
  mod_to_mont(f.p, f.n_p, n);
  // floor(p / n), as far as 101 (base.js:33-40: the Maxwell trick for <= 100)
  u32 q = 0, rem[8];
  bn_copy<8>(rem, f.p);
  while (q <= 100 && bn_geq<8>(rem, n)) {
    bn_sub<8>(rem, rem, n);
    q++;
  }
  f.ncand = q <= 100 ? q : RT_NO_MAXWELL;
  bn_copy<8>(f.gx, gx);
  bn_copy<8>(f.gy, gy);
}
// An ECDSA domain on a user-defined short curve (ellgpu_curve_define_short_domain): the curve's
// block plus the order n and the generator G -- EC#verify, k*G and mulAdd with G on the device.
// Refused: n even or < 3, G not on the curve (coordinates >= p included), 4a^3 + 27b^2 = 0.
// n's primality is not checked (s^-1 is Fermat's s^(n-2) on the device).
inline RtStatus rt_build_domain(const u8* p_be, const u8* a_be, const u8* b_be, const u8* n_be, const u8* gx_be,
                                const u8* gy_be, RtField& f) {
  if (!n_be || !gx_be || !gy_be) return {E_ARG, "null pointer"};
  const RtStatus st = rt_build_custom(0, p_be, a_be, b_be, f);
  if (st.code) return st;
  u32 a[8], b[8], n[8], gx[8], gy[8];
  load_be<8>(a, a_be, 32);
  load_be<8>(b, b_be, 32);
  mod_reduce(f.p, a, a);
  mod_reduce(f.p, b, b);
  load_be<8>(n, n_be, 32);
  load_be<8>(gx, gx_be, 32);
  load_be<8>(gy, gy_be, 32);
  if (!rt_order_ok(n)) return {E_ARG, "ECDSA domain: the order must be odd and >= 3"};
  // 4 a^3 + 27 b^2 != 0 (mod p): a curve, not a singular cubic
  u32 t[8], u[8], k[8];
  mod_mul(f.p, t, a, a);
  mod_mul(f.p, t, t, a);
  bn_zero<8>(k);
  k[0] = 4;
  mod_reduce(f.p, k, k);
  mod_mul(f.p, t, t, k);
  mod_mul(f.p, u, b, b);
  bn_zero<8>(k);
  k[0] = 27;
  mod_reduce(f.p, k, k);
  mod_mul(f.p, u, u, k);
  mod_add<8>(k, t, u, f.p);
  if (bn_is_zero<8>(k)) return {E_ARG, "ECDSA domain: singular curve (4a^3 + 27b^2 = 0 mod p)"};
  // G on the curve: y^2 == x^3 + a x + b, with x, y < p
  if (bn_geq<8>(gx, f.p) || bn_geq<8>(gy, f.p)) return {E_ARG, "ECDSA domain: G is not on the curve"};
  mod_mul(f.p, t, gx, gx);
  mod_add<8>(t, t, a, f.p);
  mod_mul(f.p, t, t, gx);
  mod_add<8>(t, t, b, f.p);
  mod_mul(f.p, u, gy, gy);
  if (!bn_eq<8>(t, u)) return {E_ARG, "ECDSA domain: G is not on the curve"};
  rt_fill_domain(f, n, gx, gy);
  return {E_OK, nullptr};
}
// An ECDSA domain on a user-defined Edwards curve (ellgpu_curve_define_edwards_domain): the curve's
// block (rt_build_custom(1, ...)) plus the same domain fields.  Refused: n even or < 3, a
// coordinate of G >= p, G off the curve a x^2 + y^2 = 1 + d x^2 y^2, G = (0, 1).  Neither p nor n
// is tested for primality and n * G = O is not tested, as on a short domain.
inline RtStatus rt_build_edwards_domain(const u8* p_be, const u8* a_be, const u8* d_be, const u8* n_be,
                                        const u8* gx_be, const u8* gy_be, RtField& f) {
  if (!n_be || !gx_be || !gy_be) return {E_ARG, "null pointer"};
  const RtStatus st = rt_build_custom(1, p_be, a_be, d_be, f);
  if (st.code) return st;
  u32 a[8], d[8], n[8], gx[8], gy[8];
  load_be<8>(a, a_be, 32);
  load_be<8>(d, d_be, 32);
  mod_reduce(f.p, a, a);
  mod_reduce(f.p, d, d);
  load_be<8>(n, n_be, 32);
  load_be<8>(gx, gx_be, 32);
  load_be<8>(gy, gy_be, 32);
  if (!rt_order_ok(n)) return {E_ARG, "ECDSA domain: the order must be odd and >= 3"};
  if (bn_geq<8>(gx, f.p) || bn_geq<8>(gy, f.p)) return {E_ARG, "ECDSA domain: G is not on the curve"};
  u32 x2[8], y2[8], l[8], r[8], one[8];
  bn_zero<8>(one);
  one[0] = 1;
  mod_mul(f.p, x2, gx, gx);
  mod_mul(f.p, y2, gy, gy);
  mod_mul(f.p, l, a, x2);
  mod_add<8>(l, l, y2, f.p);
  mod_mul(f.p, r, d, x2);
  mod_mul(f.p, r, r, y2);
  mod_add<8>(r, r, one, f.p);
  if (!bn_eq<8>(l, r)) return {E_ARG, "ECDSA domain: G is not on the curve"};
  if (bn_is_zero<8>(gx) && bn_eq<8>(gy, one)) return {E_ARG, "ECDSA domain: G is the identity (0, 1)"};
  rt_fill_domain(f, n, gx, gy);
  return {E_OK, nullptr};
}

// p mod n of a domain's block, for EC#recoverPubKey's second-candidate test (ec/index.js:243:
// r.cmp(p.umod(n)) >= 0).  A reduction, not p - n: n may exceed p, and p / n may be 8.  Kept beside
// the block, not in it (the block's bytes are compared when a definition is registered); zero
// for a curve without a domain.
inline void rt_p_mod_n(const RtField& f, u32 (&out)[8]) {
  bn_zero<8>(out);
  if (f.domain) mod_reduce(f.n, out, f.p);
}

}  // namespace ell
