// ellgpu -- user-defined Montgomery curves  b y^2 = x^3 + a x^2 + x  over a run-time prime
// p < 2^256: `new elliptic.curve.mont({p, a, b})` with parameters that are not curve25519's
// (lib/elliptic/curve/mont.js).  x-only, as the reference's model is:
//   dbl      <- Point#dbl     (mont.js:82-101,  dbl-1987-m-3,  2M + 2S + 1 a24)
//   diffadd  <- Point#diffAdd (mont.js:107-128, dadd-1987-m-3, 4M + 2S)
//   ladder   <- Point#mul     (mont.js:130-153): k as it stands, neither reduced nor clamped
//   getx     <- Point#getX    (mont.js:167-178): X / Z, one inversion per K items
//   status   <- MontCurve#validate (mont.js:23-32): is x^3 + a x^2 + x a square?
// Field: FpMontRT (fp_rt.h).  a24 = (a + 2) / 4 is a full-width residue here (a 256-bit a over a
// brainpool prime has an eight-limb a24): a field product where mont.h has a 1 x 8 limb one.
// The constants come from the curve's parameter block, kind 2 (fp_rt.h: a_m = a, b_m = a24,
// sqrt_e = (p - 1) / 2, sqrt_kind = [p = 1 (mod 4)]); the curve's b enters no formula.
// The ladder is mont.h's: every lane walks all 256 bits with two selects per bit; under leading
// zero bits the pair stays (~P, O), so the result is projectively the reference's.
#pragma once

#include "fp_rt.h"

namespace ell {

struct MontcWork {
  typedef FpMontRT F;
  typedef F::El El;

  struct XZ {
    El x, z;
  };
  ELL_HD static XZ sel(bool c, const XZ& a, const XZ& b) {
    XZ r;
    bn_select<8>(r.x.v, c, a.x.v, b.x.v);
    bn_select<8>(r.z.v, c, a.z.v, b.z.v);
    return r;
  }
  ELL_HD static El a24() { return F::curve_b(); }          // kind 2: b_m holds (a + 2) / 4
  ELL_HD static El load_fe(const u8* p) {                  // toRed: a value >= p is reduced
    u32 t[8];
    load_be<8>(t, p, 32);
    return F::from_plain(t);
  }
  ELL_HD static XZ dbl(const XZ& p) {
    El aa = F::sqr(F::add(p.x, p.z));
    El bb = F::sqr(F::sub(p.x, p.z));
    El c = F::sub(aa, bb);
    XZ r;
    r.x = F::mul(aa, bb);
    r.z = F::mul(c, F::add(bb, F::mul(c, a24())));
    return r;
  }
  // p + q given their difference (dx : 1)
  ELL_HD static XZ diffadd(const XZ& p, const XZ& q, const El& dx) {
    El a = F::add(p.x, p.z), b = F::sub(p.x, p.z);
    El c = F::add(q.x, q.z), d = F::sub(q.x, q.z);
    El da = F::mul(d, a), cb = F::mul(c, b);
    XZ r;
    r.x = F::sqr(F::add(da, cb));                 // * diff.z, which is 1
    r.z = F::mul(dx, F::sqr(F::sub(da, cb)));
    return r;
  }

  // xz: 16 limb planes of n words, X then Z, Montgomery form
  ELL_HD static void ladder(size_t i, size_t n, const u8* ks, const u8* xs, u32* xz) {
    u32 k[8];
    load_be<8>(k, ks + i * 32, 32);
    El x = load_fe(xs + i * 32);
    XZ a, b;
    a.x = x; a.z = F::one();                      // (N/2)*Q + Q
    b.x = F::one(); b.z = F::zero();              // (N/2)*Q
    ELL_NOUNROLL
    for (int w = 0; w < 256; w++) {
      bool bit = (k[7] >> 31) != 0;
      ELL_UNROLL
      for (int l = 7; l > 0; l--) k[l] = (k[l] << 1) | (k[l - 1] >> 31);
      k[0] <<= 1;
      XZ s = diffadd(a, b, x);
      XZ d = dbl(sel(bit, a, b));
      a = sel(bit, d, s);
      b = sel(bit, s, d);
    }
    ELL_UNROLL
    for (int l = 0; l < 8; l++) {
      xz[(size_t)(0 * 8 + l) * n + i] = b.x.v[l];
      xz[(size_t)(1 * 8 + l) * n + i] = b.z.v[l];
    }
  }

  // MontCurve#validate by Euler's criterion: rhs = x^3 + a x^2 + x, rhs^((p-1)/2) == 1 or rhs == 0.
  // The reference takes Red#sqrt and squares it back: on a non-residue that answers false where
  // p = 3 (mod 4) and throws 'Assertion failed' (bn.js's Tonelli-Shanks loop) where p = 1 (mod 4).
  // 0: valid, 1: false, 3: 'Assertion failed' (the numbering of ellgpu_custom_decompress).  The
  // exponent's length is the block's, so the loop is wave-uniform.
  ELL_HD static void validate(size_t i, const u8* xs, u8* out_status) {
    const El x = load_fe(xs + i * 32);
    const El rhs = F::mul(x, F::add(F::mul(x, F::add(x, F::curve_a())), F::one()));
    const El e = F::pow_sqrt_e(rhs);
    const bool ok = F::eq(e, F::one()) || F::is_zero(rhs);
    out_status[i] = ok ? 0 : (ELL_RT.sqrt_kind ? 3 : 1);
  }

  // getX: X / Z with one inversion per K items.  vst == null (Point#mul + getX): flag = 1 where
  // Z == 0.  vst != null (KeyPair#derive): flag = vst[i] where validate refused the abscissa, else
  // 2 where Z == 0, else 0.  out_x is zeroed wherever the flag is set.
  ELL_HD static void normalize(size_t t, size_t T, size_t n, int K, const u32* xz, u32* pre, const u8* vst,
                               u8* out_x, u8* out_flag) {
    inv_share<F>(InvShare(t, T, n, K), pre,
      [&](size_t i) {
        El z = load_limbs<El>(xz, n, i, 8);
        bn_select<8>(z.v, F::is_zero(z), F::one().v, z.v);
        return z;
      },
      [&](size_t i, const El& zinv) {
        El z = load_limbs<El>(xz, n, i, 8);
        const bool inf = F::is_zero(z);
        bn_select<8>(z.v, inf, F::one().v, z.v);
        El x = F::mul(load_limbs<El>(xz, n, i, 0), zinv);
        u8 flag = inf ? 1 : 0;
        if (vst) flag = vst[i] ? vst[i] : (inf ? 2 : 0);
        if (flag) x = F::zero();
        u32 w[8];
        F::to_plain(w, x);
        store_be<8>(out_x + i * 32, w, 32);
        out_flag[i] = flag;
        return z;
      });
  }
};

}  // namespace ell
