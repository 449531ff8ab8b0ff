// ellgpu -- user-defined (twisted) Edwards curves  a x^2 + y^2 = 1 + d x^2 y^2  over a run-time
// prime p < 2^256 (c = 1): `new elliptic.curve.edwards({p, a, c: 1, d, ...})` with parameters
// that are not ed25519's.  For a != -1 the reference works in projective coordinates
// (lib/elliptic/curve/edwards.js: _projDbl :207-266, _projAdd :311-348, normalize :377-390); the
// same formulas are used here for every a (the extended a = -1 forms of the reference compute the
// same group law, and only the affine image is canonical):
//   add   add-2008-bbjlp   10M + 1S + 1a + 1d     (unified: also doubles; complete when a is a
//                                                  square and d is not -- the reference's results
//                                                  on the exceptional inputs of other curves
//                                                  are whatever these formulas give, here too)
//   dbl   dbl-2008-bbjlp   3M + 4S + 1a
//   madd  add-2008-bbjlp with Z2 = 1   9M + 1S + 1a + 1d   (the comb walks: affine table entries)
// Field: FpMontRT (fp_rt.h), a and d from the curve's parameter block.  Ladder: signed 4-bit
// fixed windows over the table P..8P, as edwards.h / ladder.h.  Fixed-base tables of caller-chosen
// points (Engine::define_ed_base): an unsigned comb of 8- or 16-bit windows over affine entries.
#pragma once

#include "fp_rt.h"
#include "ladder.h"
#include "edsum.h"

namespace ell {

struct EdcWork : EdSum<EdcWork> {
  typedef FpMontRT F;
  typedef F::El El;
  static constexpr int L = 8;
  static constexpr int BYTES = 32;
  static constexpr int NNIB = 64;
  static constexpr int NWIN = 65;              // 64 signed windows + the carry window

  struct P {
    El X, Y, Z;
  };
  // an entry of a fixed-base table: affine, Montgomery form.  The slot in front of entry 0 is the
  // table's header: x.v[0] holds the window width (8 or 16).
  struct A {
    El x, y;
  };

  ELL_HD static El ca() { return F::curve_a(); }
  ELL_HD static El cd() {
    El r;
    ELL_UNROLL
    for (int i = 0; i < 8; i++) r.v[i] = ELL_RT.d_m[i];
    return r;
  }
  ELL_HD static P identity() {
    P r; r.X = F::zero(); r.Y = F::one(); r.Z = F::one(); return r;
  }
  ELL_HD static P select(bool c, const P& x, const P& y) {
    P r;
    r.X = fe_select<F>(c, x.X, y.X);
    r.Y = fe_select<F>(c, x.Y, y.Y);
    r.Z = fe_select<F>(c, x.Z, y.Z);
    return r;
  }
  ELL_HD static P cneg(const P& p, bool neg) {
    P r = p;
    r.X = fe_select<F>(neg, F::neg(p.X), p.X);
    return r;
  }
  ELL_HD static P dbl(const P& p) {
    El B = F::sqr(F::add(p.X, p.Y));
    El C = F::sqr(p.X);
    El D = F::sqr(p.Y);
    El E = F::mul(ca(), C);
    El Ff = F::add(E, D);
    El H = F::sqr(p.Z);
    El J = F::sub(F::sub(Ff, H), H);
    P r;
    r.X = F::mul(F::sub(F::sub(B, C), D), J);
    r.Y = F::mul(Ff, F::sub(E, D));
    r.Z = F::mul(Ff, J);
    return r;
  }
  ELL_HD static P add(const P& p, const P& q, bool do_add = true) {
    El A = F::mul(p.Z, q.Z);
    El B = F::sqr(A);
    El C = F::mul(p.X, q.X);
    El D = F::mul(p.Y, q.Y);
    El E = F::mul(F::mul(cd(), C), D);
    El Ff = F::sub(B, E);
    El G = F::add(B, E);
    El t = F::sub(F::sub(F::mul(F::add(p.X, p.Y), F::add(q.X, q.Y)), C), D);
    P r;
    r.X = F::mul(F::mul(A, Ff), t);
    r.Y = F::mul(F::mul(A, G), F::sub(D, F::mul(ca(), C)));
    r.Z = F::mul(Ff, G);
    return select(do_add, r, p);
  }

  // p + q for an affine q: `add` with Z2 = 1 written out (A = Z1), one multiplication fewer and the
  // same values on every input, the exceptional ones included
  ELL_HD static P madd(const P& p, const A& q, bool do_add = true) {
    El B = F::sqr(p.Z);
    El C = F::mul(p.X, q.x);
    El D = F::mul(p.Y, q.y);
    El E = F::mul(F::mul(cd(), C), D);
    El Ff = F::sub(B, E);
    El G = F::add(B, E);
    El t = F::sub(F::sub(F::mul(F::add(p.X, p.Y), F::add(q.x, q.y)), C), D);
    P r;
    r.X = F::mul(F::mul(p.Z, Ff), t);
    r.Y = F::mul(F::mul(p.Z, G), F::sub(D, F::mul(ca(), C)));
    r.Z = F::mul(Ff, G);
    return select(do_add, r, p);
  }

  ELL_HD static El load_fe(const u8* p) {
    u32 t[8];
    load_be<8>(t, p, 32);
    return F::from_plain(t);
  }
  ELL_HD static P load_affine(const u8* xy, size_t i) {
    P r;
    r.X = load_fe(xy + i * 64);
    r.Y = load_fe(xy + i * 64 + 32);
    r.Z = F::one();
    return r;
  }
  ELL_HD static void store_proj(u32* out, size_t n, size_t i, const P& p) {
    ELL_UNROLL
    for (int l = 0; l < 8; l++) {
      out[(size_t)(0 * 8 + l) * n + i] = p.X.v[l];
      out[(size_t)(1 * 8 + l) * n + i] = p.Y.v[l];
      out[(size_t)(2 * 8 + l) * n + i] = p.Z.v[l];
    }
  }

  // tbl[j-1] = j*P, j = 1..8
  ELL_HD static void build_table8(P* tbl, const P& p) {
    tbl[0] = p;
    ELL_NOUNROLL
    for (int j = 2; j <= 8; j++) {
      P t;
      if (j & 1) t = add(tbl[j - 2], p);
      else t = dbl(tbl[j / 2 - 1]);
      tbl[j - 1] = t;
    }
  }
  template <int NS>
  ELL_HD static P run_w4(const DigitStore& ds, const P* tbl) {
    P acc = identity();
    ELL_NOUNROLL
    for (int w = NWIN - 1; w >= 0; w--) {
      if (w != NWIN - 1) {
        ELL_NOUNROLL
        for (int j = 0; j < 4; j++) acc = dbl(acc);
      }
      ELL_NOUNROLL
      for (int s = 0; s < NS; s++) {
        int d = ds.get(w * NS + s);
        int ad = d < 0 ? -d : d;
        int e = ad ? ad - 1 : 0;
        acc = add(acc, cneg(tbl[s * 8 + e], d < 0), ad != 0);
      }
    }
    return acc;
  }

  // ---- work items: Point#mul (edwards.js:362-367 -> base.js:86-126), mulAdd, Point#add -------
  ELL_HD static void mul_var(size_t i, size_t n, const u8* ks, const u8* xy, P* tbl_all,
                             const DigitStore& ds, u32* out) {
    u32 k[8];
    load_be<8>(k, ks + i * 32, 32);
    P* tbl = tbl_all + i * 8;
    build_table8(tbl, load_affine(xy, i));
    recode_w4<8, NNIB, true>(k, ds, 0, 1);
    store_proj(out, n, i, run_w4<1>(ds, tbl));
  }
  ELL_HD static void mul_add2(size_t i, size_t n, const u8* k1s, const u8* xy1, const u8* k2s,
                              const u8* xy2, P* tbl_all, const DigitStore& ds, u32* out) {
    u32 k1[8], k2[8];
    load_be<8>(k1, k1s + i * 32, 32);
    load_be<8>(k2, k2s + i * 32, 32);
    P* tbl = tbl_all + i * 16;
    build_table8(tbl, load_affine(xy1, i));
    build_table8(tbl + 8, load_affine(xy2, i));
    recode_w4<8, NNIB, true>(k1, ds, 0, 2);
    recode_w4<8, NNIB, true>(k2, ds, 1, 2);
    store_proj(out, n, i, run_w4<2>(ds, tbl));
  }
  // ---- sums of many k * P terms: what EdSum (edsum.h) asks of a work class.  An entry of the
  // partial sums is the projective (X, Y, Z) that `add` takes: three planes, no T.
  static constexpr int SUM_PLANES = 3;
  ELL_HD static void store_sum(u32* out, size_t n, size_t i, const P& p) { store_proj(out, n, i, p); }
  ELL_HD static P load_sum(const u32* proj, size_t n, size_t i) {
    P r;
    r.X = load_limbs<El>(proj, n, i, 0 * 8);
    r.Y = load_limbs<El>(proj, n, i, 1 * 8);
    r.Z = load_limbs<El>(proj, n, i, 2 * 8);
    return r;
  }
  ELL_HD static P sum_add(const P& p, const P& q) { return add(p, q); }
  ELL_HD static bool sum_on_curve(const P& p) { return on_curve(p.X, p.Y); }      // load_affine: (x, y, 1)
  // ---- fixed-base tables of caller-chosen points (BasePoint#precompute; Engine::define_ed_base) ----
  // acc + k * B over B's table: an unsigned comb of 256 / bits windows x (2^bits - 1) entries,
  // entry (w, d) = (d << (bits w)) * B, the width read from the header slot (8 or 16: one walk serves
  // both).  Branch-free: a zero digit adds entry 0 of its window and keeps the accumulator by
  // select.  The identity and points of small order are ordinary entries of a unified law.
  ELL_HD static P comb_add(P acc, const u32 (&k)[8], const A* tbl) {
    const int bits = (int)tbl[-1].x.v[0];
    const u32 dig = (1u << bits) - 1u;
    const int nw = 256 / bits;
    u32 kk[8];
    bn_copy<8>(kk, k);
    ELL_NOUNROLL
    for (int w = 0; w < nw; w++) {
      const u32 d = kk[0] & dig;
      ELL_UNROLL
      for (int i = 0; i < 7; i++) kk[i] = (kk[i] >> bits) | (kk[i + 1] << (32 - bits));
      kk[7] >>= bits;
      const u32 e = d ? d - 1 : 0;
      acc = madd(acc, tbl[(size_t)w * dig + e], d != 0);
    }
    return acc;
  }
  // P.precompute(); P.mul(k): k as it stands
  ELL_HD static void mul_base(size_t i, size_t n, const u8* ks, const A* tbl, u32* out) {
    u32 k[8];
    load_be<8>(k, ks + i * 32, 32);
    store_proj(out, n, i, comb_add(identity(), k, tbl));
  }
  // k1 * B1 + k2 * B2 (mulAdd on two precomputed operands): two walks, each at its own table's
  // width, into one accumulator
  ELL_HD static void mul_base2(size_t i, size_t n, const u8* k1s, const A* t1, const u8* k2s, const A* t2,
                               u32* out) {
    u32 k[8];
    load_be<8>(k, k1s + i * 32, 32);
    P acc = comb_add(identity(), k, t1);
    load_be<8>(k, k2s + i * 32, 32);
    store_proj(out, n, i, comb_add(acc, k, t2));
  }
  // a base before its table is built: x, y < p and on the curve (x || y big-endian at pt)
  ELL_HD static bool base_ok(const u8* pt) {
    u32 x[8], y[8], pp[8];
    load_be<8>(x, pt, 32);
    load_be<8>(y, pt + 32, 32);
    F::get_p(pp);
    if (bn_geq<8>(x, pp) || bn_geq<8>(y, pp)) return false;
    return on_curve(F::from_plain(x), F::from_plain(y));
  }

  // a x^2 + y^2 == 1 + d x^2 y^2 (EdwardsCurve#validate, edwards.js:99-112, c = 1)
  ELL_HD static bool on_curve(const El& x, const El& y) {
    El x2 = F::sqr(x), y2 = F::sqr(y);
    El lhs = F::add(F::mul(ca(), x2), y2);
    El rhs = F::add(F::one(), F::mul(F::mul(cd(), x2), y2));
    return F::eq(lhs, rhs);
  }
  // operands that are not on the curve are outside the engine's domain (edwards.h domain_mark)
  ELL_HD static void domain_mark(size_t i, const u8* xy1, const u8* xy2, u8* out_xy, u8* out_inf) {
    bool on = true;
    if (xy1) on = on_curve(load_fe(xy1 + i * 64), load_fe(xy1 + i * 64 + 32));
    if (xy2) on = on && on_curve(load_fe(xy2 + i * 64), load_fe(xy2 + i * 64 + 32));
    if (on) return;
    out_inf[i] = 2;
    if (out_xy) {
      ELL_NOUNROLL
      for (int b = 0; b < 64; b++) out_xy[i * 64 + b] = 0;
    }
  }
  // a set inf flag stands for the identity (0, 1)
  ELL_HD static void point_add(size_t i, size_t n, const u8* xy1, const u8* inf1, const u8* xy2,
                               const u8* inf2, u32* out) {
    P p = load_affine(xy1, i);
    P q = load_affine(xy2, i);
    p = select(inf1 && inf1[i], identity(), p);
    q = select(inf2 && inf2[i], identity(), q);
    store_proj(out, n, i, add(p, q));
  }
  // Point#normalize (edwards.js:377-390): x = X / Z, y = Y / Z, one inversion per K items.
  // RAW: the affine point goes to raw[i] as a table entry, left in Montgomery form, and nowhere else.
  template <bool RAW = false>
  ELL_HD static void normalize(size_t t, size_t T, size_t n, int K, const u32* proj, u32* pre,
                               u8* out_xy, u8* out_inf, A* raw = nullptr) {
    inv_share<F>(InvShare(t, T, n, K), pre,
      [&](size_t i) {
        const El z = load_limbs<El>(proj, n, i, 2 * 8);
        return fe_select<F>(F::is_zero(z), F::one(), z);
      },
      [&](size_t i, const El& zinv) {
        const El Z = load_limbs<El>(proj, n, i, 2 * 8);
        const bool zz = F::is_zero(Z);                // only off the curve / on incomplete curves
        const El z = fe_select<F>(zz, F::one(), Z);
        El x = F::mul(load_limbs<El>(proj, n, i, 0 * 8), zinv);
        El y = F::mul(load_limbs<El>(proj, n, i, 1 * 8), zinv);
        if (zz) { x = F::zero(); y = F::zero(); }
        if constexpr (RAW) {
          A e;
          e.x = x;
          e.y = y;
          raw[i] = e;
        } else {
          u32 w[8];
          F::to_plain(w, x);
          store_be<8>(out_xy + i * 64, w, 32);
          F::to_plain(w, y);
          store_be<8>(out_xy + i * 64 + 32, w, 32);
          if (out_inf) out_inf[i] = 0;
        }
        return z;
      });
  }
};

}  // namespace ell
