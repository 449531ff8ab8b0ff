// ellgpu -- sums of many k * P terms on the Edwards work classes (ellgpu_ed_mul_sum):
// curve._wnafMulAdd(1, points, coeffs, len) on any number of points (edwards.js:369-375, jmulAdd /
// mulAdd, into base.js:128-253).  Work::sum_pair / sum_fold / sum_mark (work.h) over a unified
// addition law: the three routines are the same text for ed25519 (EdWork, extended coordinates) and
// the user-defined curves (EdcWork, projective), so they are written once here and each work class
// inherits them (struct EdWork : EdSum<EdWork>).  What a work class provides:
//   P, build_table8, run_w4<2>, load_affine    its mul_add2's ladder
//   SUM_PLANES                                  planes of 8 words in an entry of the partial sums
//   store_sum / load_sum                        an entry, every coordinate the addition reads
//   sum_add(p, q)                               the full addition of two partial sums
//   sum_on_curve(p)                             the curve test of load_affine's point
#pragma once

#include "ladder.h"

namespace ell {

template <class EW>
struct EdSum {
  // The terms of a sum are taken two at a time through mul_add2's ladder.  One lane per pair.  A
  // launch covers `rows` sums (or one slice of one sum) of `len` pairs each: lane idx is pair
  // q0 + idx % len of sum idx / len, i.e. the terms 2 q and 2 q + 1 of that sum's m; ks / xys are the
  // scalars and points of the first of the rows.  A lone last term (m odd) fills its second slot
  // with the scalar 0 on its own point.  flag[idx]: 1 where one of the two points is not on the
  // curve (the sum is then outside the engine's domain, see EdWork::domain_mark).
  template <class P>
  ELL_HD static void sum_pair(size_t idx, size_t rows, size_t len, size_t m, size_t q0, const u8* ks,
                              const u8* xys, P* tbl_all, const DigitStore& ds, u32* ext, u8* flag) {
    const size_t j = idx / len;
    const size_t q = q0 + (idx - j * len);
    const size_t t1 = j * m + 2 * q;
    const bool lone = 2 * q + 1 >= m;
    const size_t t2 = lone ? t1 : t1 + 1;
    u32 k1[8], k2[8];
    load_be<8>(k1, ks + t1 * 32, 32);
    load_be<8>(k2, ks + t2 * 32, 32);
    if (lone) {
      ELL_UNROLL
      for (int l = 0; l < 8; l++) k2[l] = 0;
    }
    P* tbl = tbl_all + idx * 16;
    EW::build_table8(tbl, EW::load_affine(xys, t1));
    EW::build_table8(tbl + 8, EW::load_affine(xys, t2));
    recode_w4<8, EW::NNIB, true>(k1, ds, 0, 2);
    recode_w4<8, EW::NNIB, true>(k2, ds, 1, 2);
    EW::store_sum(ext, rows * len, idx, EW::template run_w4<2>(ds, tbl));
    // the curve test behind the ladder, on the points read again: nothing of it is live while the
    // ladder runs, so the kernel keeps mul_add2's registers
    flag[idx] = (EW::sum_on_curve(EW::load_affine(xys, t1)) && EW::sum_on_curve(EW::load_affine(xys, t2))) ? (u8)0 : (u8)1;
  }
  // One halving step of every row at once, in place.  The planes hold `rows` rows of `stride`
  // entries, of which the first `len` of each row are live partial sums; h = ceil(len / 2).  Lane
  // idx is entry i = idx % h of row idx / h: P[i] += P[i + h] where i + h < len, and the flags are
  // ORed.  Reads come from entries >= h and the lane's own, writes go to entries < h: no hazard
  // within a launch.  (The idle lanes of the launch's last wave repeat its last entry, common.h
  // fill_lane: they are lanes of that entry's own wave, whose loads all precede its first store --
  // every word of the sum depends on every word of both operands -- so they store what it stores.)
  // The law is unified: two equal partials, P + (-P) and the identity are ordinary operands.  The
  // step that leaves one partial (h == 1; len == 1 is the copy step of a row that starts with one)
  // writes it to entry c0 + row of the compact planes cext / cflag of cn entries.
  ELL_HD static void sum_fold(size_t idx, size_t rows, size_t stride, size_t len, u32* ext, u8* flag,
                              u32* cext, u8* cflag, size_t cn, size_t c0) {
    const size_t h = (len + 1) / 2;
    const size_t row = idx / h;
    const size_t i = idx - row * h;
    const size_t a = row * stride + i;
    const size_t N = rows * stride;
    auto p = EW::load_sum(ext, N, a);
    u8 f = flag[a];
    const bool pair = i + h < len;
    if (pair) {
      p = EW::sum_add(p, EW::load_sum(ext, N, a + h));
      f |= flag[a + h];
    }
    if (h == 1) {
      EW::store_sum(cext, cn, c0 + row, p);
      cflag[c0 + row] = f;
    } else if (pair) {
      EW::store_sum(ext, N, a, p);
      flag[a] = f;
    }
  }
  // behind the normalisation of the compact results: a set flag is out_inf = 2
  // (ELLGPU_STATUS_OFF_CURVE) and a zeroed result
  ELL_HD static void sum_mark(size_t i, const u8* cflag, u8* out_xy, u8* out_inf) {
    if (!cflag[i]) return;
    out_inf[i] = 2;
    ELL_NOUNROLL
    for (int b = 0; b < 64; b++) out_xy[i * 64 + b] = 0;
  }
};

}  // namespace ell
