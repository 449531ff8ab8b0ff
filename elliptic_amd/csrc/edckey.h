// ellgpu -- the key side of user-defined (twisted) Edwards curves (edcustom.h): pointFromX /
// pointFromY (lib/elliptic/curve/edwards.js:50-97), BaseCurve#decodePoint (base.js:270-293),
// KeyPair#validate and KeyPair#derive (ec/key.js:40-51, 101-107) over the run-time field.
//   front_coord / front_enc   one item per lane: the raw coordinate or the SEC1 decoder, reduction
//                             mod p, numerator and denominator of the missing coordinate's square
//                               from x:  y^2 = (1 - a x^2) / (1 - d x^2)
//                               from y:  x^2 = (y^2 - 1) / (d y^2 - a)
//   quotient                  num / den with ONE inversion per K items (the prefix products of
//                             EdcWork::normalize); a zero denominator enters the shared product as
//                             one and yields 0 for its own item, as redInvm(0) = 0 does
//   root                      one item per lane: Red#sqrt (fp_rt.h), the parity, the statuses, the
//                             curve equation of the finished point
//   front_xy                  raw x || y: reduction, Point#isInfinity, the curve equation, and the
//                             order as every item's scalar for KeyPair#validate's n * P
//   derive_finish             X / Z with one inversion per K items and the status fold
//   validate_fold             KeyPair#validate's tests in its order
// The ladder between them is EdcWork::mul_var, unchanged.  These kernels read the square-root
// constants of the parameter block; an Edwards curve's registered block has none (its bytes are
// pinned), so the calls that launch them upload the curve's AUGMENTED copy (Engine::custom_aug_).
#pragma once

#include "edcustom.h"

namespace ell {

struct EdcKey {
  typedef FpMontRT F;
  typedef F::El El;
  // statuses of the decoder (Work::DECODE_*), of derive (Work::DERIVE_*) and of validate
  enum { ST_OK = 0, ST_FORMAT = 1, ST_INVALID = 2, ST_ASSERT = 3 };
  enum { DERIVE_OK = 0, DERIVE_NOT_VALIDATED = 1, DERIVE_Z0 = 2, DERIVE_UNDECODED = 3 };
  enum { VAL_OK = 0, VAL_INF = 1, VAL_NOT_POINT = 2, VAL_ORDER = 3 };
  // what the root pass owes an item: nothing, y from x, x from y; bit 2: the parity asked for
  enum { NEED_NONE = 0, NEED_Y = 1, NEED_X = 2, NEED_ODD = 4 };

  ELL_HD static El load_fe_n(const u8* p, int pl) {        // pl <= 32 bytes, reduced mod p
    u32 t[8];
    load_be<8>(t, p, pl);
    return F::from_plain(t);
  }
  ELL_HD static void store_fe(u8* p, const El& a) {
    u32 w[8];
    F::to_plain(w, a);
    store_be<8>(p, w, 32);
  }
  // nd: 16 limb planes of n words, the numerator then the denominator, Montgomery form
  ELL_HD static void put_fraction(u32* nd, size_t n, size_t i, const El& v, bool from_y) {
    const El v2 = F::sqr(v);
    El num, den;
    if (from_y) {
      num = F::sub(v2, F::one());
      den = F::sub(F::mul(EdcWork::cd(), v2), EdcWork::ca());
    } else {
      num = F::sub(F::one(), F::mul(EdcWork::ca(), v2));
      den = F::sub(F::one(), F::mul(EdcWork::cd(), v2));
    }
    store_limbs(nd, n, i, 0, num);
    store_limbs(nd, n, i, 8, den);
  }
  // pointFromX (from_y == 0) / pointFromY: the known coordinate into pts, the fraction into nd
  ELL_HD static void front_coord(size_t i, size_t n, const u8* vs, const u8* odd, int from_y, u8* pts, u8* st,
                                 u8* need, u32* nd) {
    const El v = load_fe_n(vs + i * 32, 32);
    store_fe(pts + i * 64 + (from_y ? 32 : 0), v);
    store_fe(pts + i * 64 + (from_y ? 0 : 32), F::zero());
    put_fraction(nd, n, i, v, from_y != 0);
    st[i] = ST_OK;
    need[i] = (u8)((from_y ? NEED_X : NEED_Y) | (odd[i] ? NEED_ODD : 0));
  }
  // decodePoint: 04 / 06 / 07 || x || y as they stand (not tested against the curve), 02 / 03 || x
  // for pointFromX; every other prefix or length is 'Unknown point format'
  ELL_HD static void front_enc(size_t i, size_t n, const u8* enc, size_t len, int pl, u8* pts, u8* st, u8* need,
                               u32* nd) {
    const u8* e = enc + i * len;
    const u32 tag = len ? e[0] : 0u;
    El x = F::zero(), y = F::zero();
    u32 s = ST_FORMAT, nk = NEED_NONE;
    if ((tag == 4 || tag == 6 || tag == 7) && len == 1 + 2 * (size_t)pl) {
      const u32 last = e[len - 1] & 1u;
      if ((tag == 6 && last != 0) || (tag == 7 && last != 1)) s = ST_ASSERT;
      else {
        x = load_fe_n(e + 1, pl);
        y = load_fe_n(e + 1 + pl, pl);
        s = ST_OK;
      }
    } else if ((tag == 2 || tag == 3) && len == 1 + (size_t)pl) {
      x = load_fe_n(e + 1, pl);
      s = ST_OK;
      nk = NEED_Y | (tag == 3 ? NEED_ODD : 0);
    }
    store_fe(pts + i * 64, x);
    store_fe(pts + i * 64 + 32, y);
    if (nk) put_fraction(nd, n, i, x, false);
    else {
      store_limbs(nd, n, i, 0, F::zero());
      store_limbs(nd, n, i, 8, F::zero());
    }
    st[i] = (u8)s;
    need[i] = (u8)nk;
  }
  // num / den into the numerator's planes, thread t: items t, t + T, ...
  ELL_HD static void quotient(size_t t, size_t T, size_t n, int K, u32* nd, u32* pre) {
    inv_share<F>(InvShare(t, T, n, K), pre,
      [&](size_t i) {
        const El z = load_limbs<El>(nd, n, i, 8);
        return fe_select<F>(F::is_zero(z), F::one(), z);
      },
      [&](size_t i, const El& dinv) {
        const El q = F::mul(load_limbs<El>(nd, n, i, 0), dinv);
        const El den = load_limbs<El>(nd, n, i, 8);
        const bool dz = F::is_zero(den);
        store_limbs(nd, n, i, 0, fe_select<F>(dz, F::zero(), q));
        return fe_select<F>(dz, F::one(), den);
      });
  }
  // a x^2 + y^2 == 1 + d x^2 y^2
  ELL_HD static bool on_curve(const El& x, const El& y) { return EdcWork::on_curve(x, y); }
  // The missing coordinate of an item that needs one: Red#sqrt of the quotient, squared back
  // ('invalid point' where p = 3 mod 4, bn.js's 'Assertion failed' where Tonelli-Shanks runs), then
  // the parity.  pointFromY answers x^2 = 0 before any root: (0, y) for an even request, 'invalid
  // point' for an odd one.  out_xy is zeroed unless the status is 0.  valid (may be null): the
  // curve equation of a point that decoded.
  ELL_HD static void root(size_t i, size_t n, const u32* nd, const u8* pts, const u8* st_in, const u8* need,
                          u8* out_xy, u8* out_st, u8* valid) {
    El x = load_fe_n(pts + i * 64, 32), y = load_fe_n(pts + i * 64 + 32, 32);
    u32 s = st_in[i];
    const u32 nk = need[i];
    if (nk & 3u) {
      const El q = load_limbs<El>(nd, n, i, 0);
      El r = F::sqrt(q);
      const bool ok = F::eq(F::sqr(r), q);
      const bool want_odd = (nk & NEED_ODD) != 0;
      r = fe_select<F>(F::is_odd(r) != want_odd, F::neg(r), r);
      s = ok ? (u32)ST_OK : (ELL_RT.sqrt_kind ? (u32)ST_ASSERT : (u32)ST_INVALID);
      if ((nk & 3u) == NEED_X) {
        if (F::is_zero(q) && want_odd) s = ST_INVALID;
        x = r;
      } else {
        y = r;
      }
    }
    const bool good = s == ST_OK;
    x = fe_select<F>(good, x, F::zero());
    y = fe_select<F>(good, y, F::zero());
    if (valid) {
      const bool on = good && on_curve(x, y);
      valid[i] = on ? 1 : 0;
      // what the ladder runs on where the key is refused: the identity
      y = fe_select<F>(on, y, F::one());
      x = fe_select<F>(on, x, F::zero());
    }
    store_fe(out_xy + i * 64, x);
    store_fe(out_xy + i * 64 + 32, y);
    out_st[i] = (u8)s;
  }
  // raw x || y: the reduced point for the ladder (the identity where it is not on the curve),
  // valid = the curve equation, inf (may be null) = Point#isInfinity, i.e. (0, 1); scal (may be
  // null): `order` as the item's scalar
  struct Scalar { u8 b[32]; };
  ELL_HD static void front_xy(size_t i, const u8* xy, u8* pts, u8* valid, u8* inf, u8* scal, const Scalar& order) {
    const El x = load_fe_n(xy + i * 64, 32), y = load_fe_n(xy + i * 64 + 32, 32);
    const bool on = on_curve(x, y);
    valid[i] = on ? 1 : 0;
    if (inf) inf[i] = (F::is_zero(x) && F::eq(y, F::one())) ? 1 : 0;
    if (pts) {
      store_fe(pts + i * 64, fe_select<F>(on, x, F::zero()));
      store_fe(pts + i * 64 + 32, fe_select<F>(on, y, F::one()));
    }
    if (scal) {
      ELL_NOUNROLL
      for (int b = 0; b < 32; b++) scal[i * 32 + b] = order.b[b];
    }
  }
  // derive's last pass: getX() = X / Z of priv * pub with one inversion per K items, and the status
  // fold -- 3 the key did not decode (dec_st, null for raw keys), 1 'public point not validated',
  // 2 Z = 0 (the reference's getX() returns 0 there), else 0.  An item that is not 0 enters the
  // shared product as one and gets a zeroed x.  err (may be null): the decoder's own status.
  ELL_HD static void derive_finish(size_t t, size_t T, size_t n, int K, const u32* proj, const u8* dec_st,
                                   const u8* valid, u32* pre, u8* out_x, u8* status, u8* err) {
    inv_share<F>(InvShare(t, T, n, K), pre,
      [&](size_t i) {
        const El z = load_limbs<El>(proj, n, i, 16);
        const u32 ds = dec_st ? dec_st[i] : (u32)ST_OK;
        int st = DERIVE_OK;
        if (ds != ST_OK) st = DERIVE_UNDECODED;
        else if (!valid[i]) st = DERIVE_NOT_VALIDATED;
        else if (F::is_zero(z)) st = DERIVE_Z0;
        status[i] = (u8)st;
        if (err) err[i] = (u8)ds;
        return fe_select<F>(st == DERIVE_OK, z, F::one());
      },
      [&](size_t i, const El& zinv) {
        const bool ok = status[i] == DERIVE_OK;
        const El z = fe_select<F>(ok, load_limbs<El>(proj, n, i, 16), F::one());
        const El x = F::mul(load_limbs<El>(proj, n, i, 0), zinv);
        store_fe(out_x + i * 32, fe_select<F>(ok, x, F::zero()));
        return z;
      });
  }
  // KeyPair#validate in its order: 1 'Invalid public key' ((0, 1)), 2 'Public key is not a point',
  // 3 'Public key * N != O' (proj, the ladder's order * P: null without the order test; the
  // identity is X = 0 and Y = Z), else 0
  ELL_HD static void validate_fold(size_t i, size_t n, const u8* inf, const u8* valid, const u32* proj, u8* status) {
    int st = VAL_OK;
    if (inf[i]) st = VAL_INF;
    else if (!valid[i]) st = VAL_NOT_POINT;
    else if (proj) {
      const bool id = F::is_zero(load_limbs<El>(proj, n, i, 0)) && F::eq(load_limbs<El>(proj, n, i, 8), load_limbs<El>(proj, n, i, 16));
      if (!id) st = VAL_ORDER;
    }
    status[i] = (u8)st;
  }
};

}  // namespace ell
