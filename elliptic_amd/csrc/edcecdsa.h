// ellgpu -- ECDSA on a user-defined Edwards domain (ellgpu_curve_define_edwards_domain): the `EC`
// class over `new elliptic.curve.edwards({p, a, c: 1, d, n, g})` with parameters that are not
// ed25519's -- EC#verify (lib/elliptic/ec/index.js:188-229) and the k*G of EC#sign (:110-186) on the
// projective formulas of edcustom.h.
//   g_table        once per domain, one thread: G .. 8G normalised to Z = 1, Montgomery form
//                  (GT_WORDS words: 512 B); the ladders stage it in LDS per workgroup
//   verify_ladder  one item per lane: the key (reduced, tested against the curve equation, the
//                  identity in its place where it fails -- what EdcKey::front_xy arranges), its
//                  window table Q .. 8Q, then u1*G + u2*Q over signed 4-bit windows of both scalars
//                  in one interleaved loop; additions with an entry of G's table are MIXED
//   eq_maxwell     Point#isInfinity (edwards.js:167-172) and Point#eqXToP (:415-431): X == (r + j n) Z
//                  for j = 0, 1, ... while r + j n < p -- no inversion
//   eq_affine      floor(p / n) > 100 (no _maxwellTrick): getX().umod(n) == r, X / Z with one
//                  inversion per K items, then a general reduction mod n
//   sign_mul       k*G over G's table alone (65 signed windows, four doublings between them)
//   sign_norm      EdcWork::normalize and Point#isInfinity of k*G, for Work::rt_sign_finish
// The scalar halves -- Work::ecdsa_prep, rt_sign_nonce, rt_sign_finish -- are the short domain's
// kernels: they read n and its constants from the block and never the curve.
#pragma once

#include "edckey.h"
#include "work.h"

namespace ell {

struct EdcEcdsa {
  typedef FpMontRT F;
  typedef FpMontRTn Fn;
  typedef F::El El;
  typedef EdcWork::P P;
  typedef Work<CvCustomDomain> WD;
  static constexpr int NWIN = EdcWork::NWIN;
  // G's table: word (c * 8 + l) * 8 + e is limb l of coordinate c (0: x, 1: y) of (e + 1) * G -- the
  // eight entries of one limb are neighbours, so the lanes of a wave, each with a digit of its own,
  // read eight consecutive LDS banks
  static constexpr int GT_WORDS = 2 * 8 * 8;

  ELL_HD static void g_table(u32* gt) {
    u32 gx[8], gy[8];
    WD::generator_words(gx, gy);
    P g;
    g.X = F::from_plain(gx);
    g.Y = F::from_plain(gy);
    g.Z = F::one();
    P tbl[8];
    EdcWork::build_table8(tbl, g);
    El pre[8];
    El acc = F::one();
    ELL_NOUNROLL
    for (int e = 0; e < 8; e++) {
      pre[e] = acc;
      acc = F::mul(acc, fe_select<F>(F::is_zero(tbl[e].Z), F::one(), tbl[e].Z));
    }
    El inv = F::inv(acc);
    ELL_NOUNROLL
    for (int e = 7; e >= 0; e--) {
      const El zinv = F::mul(inv, pre[e]);
      inv = F::mul(inv, fe_select<F>(F::is_zero(tbl[e].Z), F::one(), tbl[e].Z));
      const El x = F::mul(tbl[e].X, zinv), y = F::mul(tbl[e].Y, zinv);
      ELL_UNROLL
      for (int l = 0; l < 8; l++) {
        gt[(0 * 8 + l) * 8 + e] = x.v[l];
        gt[(1 * 8 + l) * 8 + e] = y.v[l];
      }
    }
  }
  ELL_HD static El gt_coord(const u32* gt, int c, int e) {
    El r;
    ELL_UNROLL
    for (int l = 0; l < 8; l++) r.v[l] = gt[(c * 8 + l) * 8 + e];
    return r;
  }
  // add-2008-bbjlp with Z2 = 1: A = Z1, one product fewer than EdcWork::add (9M + 1S + 1a + 1d)
  ELL_HD static P madd(const P& p, const El& x2, const El& y2, bool do_add) {
    El B = F::sqr(p.Z);
    El C = F::mul(p.X, x2);
    El D = F::mul(p.Y, y2);
    El E = F::mul(F::mul(EdcWork::cd(), C), D);
    El Ff = F::sub(B, E);
    El G = F::add(B, E);
    El t = F::sub(F::sub(F::mul(F::add(p.X, p.Y), F::add(x2, y2)), C), D);
    P r;
    r.X = F::mul(F::mul(p.Z, Ff), t);
    r.Y = F::mul(F::mul(p.Z, G), F::sub(D, F::mul(EdcWork::ca(), C)));
    r.Z = F::mul(Ff, G);
    return EdcWork::select(do_add, r, p);
  }
  // acc + d * G for a signed digit d in [-8, 8]
  ELL_HD static P add_g(const P& acc, const u32* gt, int d) {
    const int ad = d < 0 ? -d : d;
    const int e = ad ? ad - 1 : 0;
    const El x = gt_coord(gt, 0, e);
    return madd(acc, fe_select<F>(d < 0, F::neg(x), x), gt_coord(gt, 1, e), ad != 0);
  }
  ELL_HD static bool is_infinity(const El& X, const El& Y, const El& Z) { return F::is_zero(X) && F::eq(Y, Z); }

  // u12: the planes Work::ecdsa_prep wrote (u1 then u2, plain, zero where r or s is out of range)
  ELL_HD static void verify_ladder(size_t i, size_t n, const u32* u12, const u8* pub, const u32* gt, P* tbl_all,
                                   const DigitStore& ds, u32* proj, u8* on_curve) {
    const El x = EdcKey::load_fe_n(pub + i * 64, 32), y = EdcKey::load_fe_n(pub + i * 64 + 32, 32);
    const bool on = EdcWork::on_curve(x, y);
    on_curve[i] = on ? 1 : 0;
    P q;
    q.X = fe_select<F>(on, x, F::zero());
    q.Y = fe_select<F>(on, y, F::one());
    q.Z = F::one();
    P* tbl = tbl_all + i * 8;
    EdcWork::build_table8(tbl, q);
    u32 u1[8], u2[8];
    ELL_UNROLL
    for (int l = 0; l < 8; l++) {
      u1[l] = u12[(size_t)(0 * 8 + l) * n + i];
      u2[l] = u12[(size_t)(1 * 8 + l) * n + i];
    }
    recode_w4<8, EdcWork::NNIB, true>(u1, ds, 0, 2);
    recode_w4<8, EdcWork::NNIB, true>(u2, ds, 1, 2);
    P acc = EdcWork::identity();
    ELL_NOUNROLL
    for (int w = NWIN - 1; w >= 0; w--) {
      if (w != NWIN - 1) {
        ELL_NOUNROLL
        for (int j = 0; j < 4; j++) acc = EdcWork::dbl(acc);
      }
      acc = add_g(acc, gt, ds.get(w * 2));
      const int d = ds.get(w * 2 + 1);
      const int ad = d < 0 ? -d : d;
      acc = EdcWork::add(acc, EdcWork::cneg(tbl[ad ? ad - 1 : 0], d < 0), ad != 0);
    }
    EdcWork::store_proj(proj, n, i, acc);
  }
  // EC#verify's last lines with _maxwellTrick: false for the identity, else eqXToP(r)
  ELL_HD static void eq_maxwell(size_t i, size_t n, const u32* proj, const u8* valid, const u8* on_curve,
                                const u8* rs, u8* out_ok, u8* out_st) {
    const El X = load_limbs<El>(proj, n, i, 0), Y = load_limbs<El>(proj, n, i, 8),
             Z = load_limbs<El>(proj, n, i, 16);
    u32 r[8], nn[8], pp[8], xc[8];
    load_be<8>(r, rs + i * 32, 32);
    El rx = F::mul(F::from_plain(r), Z);                  // r.toRed(red): r mod p
    bool hit = F::eq(X, rx);
    WD::order_words(nn);
    F::get_p(pp);
    bn_copy<8>(xc, r);
    El np;
    ELL_UNROLL
    for (int l = 0; l < 8; l++) np.v[l] = ELL_RT.n_p[l];
    const El t = F::mul(np, Z);
    bool live = true;
    const u32 ncand = ELL_RT.ncand;                        // wave-uniform
    ELL_NOUNROLL
    for (u32 k = 0; k < ncand; k++) {
      const u32 cy = bn_add<8>(xc, xc, nn);
      live = live && !cy && !bn_geq<8>(xc, pp);
      rx = F::add(rx, t);
      hit = hit || (live && F::eq(X, rx));
    }
    WD::store_verdict(i, valid[i], on_curve[i] != 0, hit && !is_infinity(X, Y, Z), out_ok, out_st);
  }
  // ... without it: getX().umod(n) == r, thread t: items t, t + T, ...
  ELL_HD static void eq_affine(size_t t, size_t T, size_t n, int K, const u32* proj, const u8* valid,
                               const u8* on_curve, const u8* rs, u32* pre, u8* out_ok, u8* out_st) {
    inv_share<F>(InvShare(t, T, n, K), pre,
      [&](size_t i) {
        const El z = load_limbs<El>(proj, n, i, 16);
        return fe_select<F>(F::is_zero(z), F::one(), z);
      },
      [&](size_t i, const El& zinv) {
        const El X = load_limbs<El>(proj, n, i, 0), Y = load_limbs<El>(proj, n, i, 8),
                 Z = load_limbs<El>(proj, n, i, 16);
        u32 x[8], xn[8], r[8];
        F::to_plain(x, F::mul(X, zinv));
        Fn::to_plain(xn, Fn::from_plain(x));                // x mod n: into the order field and out
        load_be<8>(r, rs + i * 32, 32);
        WD::store_verdict(i, valid[i], on_curve[i] != 0, bn_eq<8>(xn, r) && !is_infinity(X, Y, Z), out_ok, out_st);
        return fe_select<F>(F::is_zero(Z), F::one(), Z);
      });
  }

  // k*G for EC#sign: k = _truncateToN(nonce, true) as the short domain loads it
  ELL_HD static void sign_mul(size_t i, size_t n, const u8* nonces, const u32* gt, const DigitStore& ds, u32* proj) {
    u32 k[8];
    WD::rt_load_nonce(k, nonces + i * 32);
    recode_w4<8, EdcWork::NNIB, true>(k, ds, 0, 1);
    P acc = EdcWork::identity();
    ELL_NOUNROLL
    for (int w = NWIN - 1; w >= 0; w--) {
      if (w != NWIN - 1) {
        ELL_NOUNROLL
        for (int j = 0; j < 4; j++) acc = EdcWork::dbl(acc);
      }
      acc = add_g(acc, gt, ds.get(w));
    }
    EdcWork::store_proj(proj, n, i, acc);
  }
  // affine k*G and kp.isInfinity() for Work::rt_sign_finish
  ELL_HD static void sign_norm(size_t t, size_t T, size_t n, int K, const u32* proj, u32* pre, u8* kg_xy, u8* kg_inf) {
    EdcWork::normalize(t, T, n, K, proj, pre, kg_xy, nullptr);
    const InvShare g(t, T, n, K);
    ELL_NOUNROLL
    for (int j = 0; j < g.cnt; j++) {
      const size_t i = g.item(j);
      kg_inf[i] = is_infinity(load_limbs<El>(proj, n, i, 0), load_limbs<El>(proj, n, i, 8),
                              load_limbs<El>(proj, n, i, 16)) ? 1 : 0;
    }
  }
};

}  // namespace ell
