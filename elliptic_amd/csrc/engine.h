// ellgpu -- host-side engine: batch orchestration above the per-item work
// functions.  Templated on a backend BK that supplies memory and launches:
//
//   HipBackend  (capi.hip)          hipMalloc / hipMemcpyAsync / kernel launches on
//                                   one stream of one MI355X -- the product.
//   LoopBackend (tests/hostsim)     malloc / memcpy / a for-loop over thread ids --
//                                   CPU-only unit tests of the same code; never
//                                   shipped, never selected at run time.
//
// A launch is `bk.launch(functor, nthreads)`: the functor's operator()(tid, ds)
// runs once per thread id with a DigitStore of Fn::DS_PER_LANE bytes per lane.
#pragma once

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "edwards.h"
#include "edcustom.h"
#include "edckey.h"
#include "montcustom.h"
#include "mont.h"
#include "rt_define.h"
#include "work.h"
#include "edcecdsa.h"
#include "coop_ed.h"

#ifndef ELL_INV_BATCH
#define ELL_INV_BATCH 16
#endif
// p521 (one wave per SIMD, 256 VGPRs + AGPRs, spill-free) issues at the lone-wave half rate.  A
// second instantiation held to 256 registers runs two waves per SIMD: each wave is 1.6x slower
// (spills), the pair 1.26x faster -- but only batches of more than one full single-wave round
// (256 CUs x 4 SIMDs x 64 lanes) have a second wave to pair.
#define ELL_P521_PAIR_MIN ((size_t)256 * 4 * 64 + 4096)
#ifndef ELL_MULVAR_MIN_WAVES
#define ELL_MULVAR_MIN_WAVES 4
#endif
#ifndef ELL_CUSTOM_MIN_WAVES
#define ELL_CUSTOM_MIN_WAVES 3      // user-defined curves (Jacobian window table, generic-a doubling)
#endif
// secp256k1's verify / k1*G + k2*P kernels: 4 waves/SIMD (128 VGPRs).  With beta re-materialised
// at each lookup, zg parked in a free table slot and u1 / r loaded behind compiler barriers
// (common.h: ELL_BETA_REMAT, ELL_SPILL_ZG, ELL_LATE_LOADS) the ladder loop holds no spills at 128
// registers: ecdsa_main 8.43 -> 8.20 ms per 2^20 (3 waves, 168 VGPRs before; 5 waves = 96 VGPRs
// spills 304 B and is 13 % slower), profiles/r02_four_waves_ab.jsonl
#ifndef ELL_ENDO_MIN_WAVES
#define ELL_ENDO_MIN_WAVES 4
#endif
#ifndef ELL_PIPE_STEP_DEFAULT
#ifdef ELL_PIPE_STEP
#define ELL_PIPE_STEP_DEFAULT ELL_PIPE_STEP
#else
#define ELL_PIPE_STEP_DEFAULT 3      // hip_backend.h documents the sweep
#endif
#endif
#ifndef ELL_FIXED_MIN_WAVES
#define ELL_FIXED_MIN_WAVES 4       // fixed-base comb kernels (mul_fixed, sign_mul) of the <= 256-bit curves: 128 VGPRs, -2..3.5 % on secp256k1, neutral elsewhere
#endif
#ifndef ELL_ECDSA_MIN_WAVES
#define ELL_ECDSA_MIN_WAVES 3
#endif
// (batches of at most three waves on every SIMD take the WIDE ecdsa_main: Engine::Tuning)
// ecdsa_table (the window table of the small-grid verify, built beside ecdsa_prep): waves per
// SIMD its register budget leaves room for
#ifndef ELL_ECDSA_TABLE_MIN_WAVES
#define ELL_ECDSA_TABLE_MIN_WAVES 4
#endif
// 1 (default): small-grid secp256k1 verifies run as prep || table -> ladder; 0: prep -> main
#ifndef ELL_SPLIT_SMALL_VERIFY
#define ELL_SPLIT_SMALL_VERIFY 1
#endif
// entries per slice of the fixed-base table build (Engine::build_table); the CPU unit-test build
// of these headers passes a small value so that its narrow combs are built in several slices too
#ifndef ELL_COMB_SLICE
#define ELL_COMB_SLICE (1u << 20)
#endif
#ifndef ELL_P521_MIN_WAVES
#define ELL_P521_MIN_WAVES 1        // (the p521 ladders take 232-234 VGPRs: two waves either way; 3 waves spill 560 B)
#endif
// p384 (12 limbs): waves per SIMD the ladder kernels leave room for
#ifndef ELL_P384_MIN_WAVES
#define ELL_P384_MIN_WAVES 3        // 168 VGPRs: +2..3 % over 2 waves since the leaner add / sub (profiles/r02_p384_waves_ab.txt)
#endif

namespace ell {

// ---- functors (one per kernel) ------------------------------------------------
// WIDE: the small-grid tuning of the secp256k1 ladder (see FnEcdsaMain)
template <class CV, int MW = 0, bool WIDE = false>
struct FnMulVar {
  static constexpr const char* NAME = "mul_var";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = W::NWIN * W::NSV;
  static constexpr int MIN_WAVES = MW ? MW : (W::L <= 8 ? (CV::JTABLE ? ELL_CUSTOM_MIN_WAVES : ELL_MULVAR_MIN_WAVES) : (W::L == 12 ? ELL_P384_MIN_WAVES : ELL_P521_MIN_WAVES));   // <= 128 VGPRs for 256-bit curves: +2..4 % despite ~50 B of spills
  size_t n; const u8* k; const u8* xy; typename W::VT* tbl; u32* jac;
  ELL_HD void operator()(size_t i, const DigitStore& ds) const {
    if (i < n) W::template mul_var<WIDE>(i, n, k, xy, tbl, ds, jac);
  }
};
template <class CV>
struct FnMulAdd2 {
  static constexpr const char* NAME = "mul_add2";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = W::NWIN * W::NSV * 2;
  static constexpr int MIN_WAVES = W::L <= 8 ? 3 : (W::L == 12 ? 2 : 1);   // <= 168 VGPRs for the 256-bit curves, <= 256 for p384
  size_t n; const u8* k1; const u8* xy1; const u8* k2; const u8* xy2; typename W::J* tbl; u32* jac;
  ELL_HD void operator()(size_t i, const DigitStore& ds) const {
    if (i < n) W::mul_add2(i, n, k1, xy1, k2, xy2, tbl, ds, jac);
  }
};
// sums of many k * P terms (Work::sum_pair, sum_fold, sum_mark): mul_add2's ladder over the pairs of
// neighbouring terms, the halving steps over the partial sums, the off-curve mark on the results
template <class CV>
struct FnSumPairs {
  static constexpr const char* NAME = "sum_pairs";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = FnMulAdd2<CV>::DS_PER_LANE;
  static constexpr int MIN_WAVES = FnMulAdd2<CV>::MIN_WAVES;
  size_t rows, len, m, q0; const u8* k; const u8* xy; typename W::J* tbl; u32* jac; u8* flag;
  ELL_HD void operator()(size_t i, const DigitStore& ds) const {
    if (i < rows * len) W::sum_pair(i, rows, len, m, q0, k, xy, tbl, ds, jac, flag);
  }
};
template <class CV>
struct FnSumFold {
  static constexpr const char* NAME = "sum_fold";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t rows, stride, len; u32* jac; u8* flag; u32* cjac; u8* cflag; size_t cn, c0;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < rows * ((len + 1) / 2)) W::sum_fold(i, rows, stride, len, jac, flag, cjac, cflag, cn, c0);
  }
};
template <class CV>
struct FnSumMark {
  static constexpr const char* NAME = "sum_mark";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* cflag; u8* out_xy; u8* out_inf;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::sum_mark(i, cflag, out_xy, out_inf);
  }
};
template <class CV, int MW = 0>
struct FnMulAddG {
  static constexpr const char* NAME = "mul_add_g";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = W::NWIN * W::NSV;
  static constexpr int MIN_WAVES = MW ? MW : (W::L <= 8 ? (CV::ENDO ? ELL_ENDO_MIN_WAVES : ELL_ECDSA_MIN_WAVES) : (W::L == 12 ? ELL_P384_MIN_WAVES : ELL_P521_MIN_WAVES));      // p384: 2 waves/SIMD (<= 256 registers) beats a spill-free single wave
  size_t n; const u8* k1; const u8* k2; const u8* xy2; const typename W::A* comb;
  typename W::VT* tbl; u32* jac;
  ELL_HD void operator()(size_t i, const DigitStore& ds) const {
    if (i < n) W::mul_add_g_item(i, n, k1, k2, xy2, comb, tbl, ds, jac);
  }
};
template <class CV, int MW = 0>
struct FnMulFixed {
  static constexpr const char* NAME = "mul_fixed";
  typedef Work<CV> W;
  static constexpr int MIN_WAVES = MW ? MW : (W::L <= 8 ? ELL_FIXED_MIN_WAVES : 1);
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* k; const typename W::A* comb; u32* jac;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::mul_fixed(i, n, k, comb, jac);
  }
};
// comb construction: entry idx = w * PER + (d - 1) of the fixed-base table is (d << (CB w)) * B.
// comb_entry_scalar gives that scalar for entry idx (cb: window bits of a SIGNED comb, else
// W::COMB_BITS): reduced mod n on the presets -- every point of a preset has the prime order n, so
// ((d << sh) mod n) * B is exact and never O -- and left as it stands on a user-defined curve: the
// unsigned comb's values stay below 2^256, n need not be the order of G (curves.h CvCustomDomain)
// and a caller's base has no known order (an entry that comes out O refuses the base)
template <class CV>
ELL_HD void comb_entry_scalar(size_t idx, int cb, u32* kk) {
  typedef Work<CV> W;
  const size_t per = W::COMB_SIGNED ? ((size_t)1 << (cb - 1)) : (size_t)W::COMB_DIG;
  const int w = (int)(idx / per);
  const u32 d = (u32)(idx % per) + 1u;
  const int sh = w * (W::COMB_SIGNED ? cb : W::COMB_BITS);
  // (d << sh) mod n: the value can exceed the scalar's byte length in the top window (the
  // signed recoding's carry window of a narrow comb: 2^256 * G), so it goes through the order
  // field like any over-long byte string (Work::bytes_mod_n)
  constexpr int LN = W::LN;
  u32 v[2 * LN];
  ELL_UNROLL
  for (int l = 0; l < 2 * LN; l++) v[l] = 0;
  const int li = sh >> 5, bs = sh & 31;
  ELL_UNROLL
  for (int l = 0; l < 2 * LN; l++) {
    if (l == li) v[l] = d << bs;
    if (l == li + 1 && bs) v[l] = d >> (32 - bs);
  }
  if constexpr (CV::RT_ORDER) {
    ELL_UNROLL
    for (int l = 0; l < W::L; l++) kk[l] = v[l];
  } else {
    u8 vb[8 * LN];
    store_be<2 * LN>(vb, v, 8 * LN);
    typename W::Nl km = W::bytes_mod_n(vb, 8 * LN);
    u32 kn[LN];
    W::Fn::to_plain(kn, km);
    ELL_UNROLL
    for (int l = 0; l < W::L; l++) kk[l] = l < LN ? kn[l] : 0u;
  }
}
// the scalars and the generator for entries [first, first + n)
template <class CV>
struct FnCombGen {
  static constexpr const char* NAME = "comb_gen";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; size_t first; u8* k; u8* xy; int cb;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i >= n) return;
    u32 kk[W::L], gx[W::L], gy[W::L];
    comb_entry_scalar<CV>(first + i, cb, kk);
    if constexpr (CV::RT_ORDER) {
      W::generator_words(gx, gy);
    } else {
      ELL_UNROLL
      for (int l = 0; l < W::L; l++) { gx[l] = W::C::gx_plain[l]; gy[l] = W::C::gy_plain[l]; }
    }
    store_be<W::L>(k + i * W::BYTES, kk, W::BYTES);
    store_be<W::L>(xy + i * 2 * W::BYTES, gx, W::BYTES);
    store_be<W::L>(xy + i * 2 * W::BYTES + W::BYTES, gy, W::BYTES);
  }
};
// ... of a caller-chosen base (Engine::define_base): the point is read from a device buffer,
// x || y big-endian
template <class CV>
struct FnBaseCombGen {
  static constexpr const char* NAME = "base_comb_gen";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; size_t first; const u8* pt; u8* k; u8* xy; int cb;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i >= n) return;
    u32 kk[W::L];
    comb_entry_scalar<CV>(first + i, cb, kk);
    store_be<W::L>(k + i * W::BYTES, kk, W::BYTES);
    ELL_NOUNROLL
    for (int b = 0; b < 2 * W::BYTES; b++) xy[i * 2 * W::BYTES + b] = pt[b];
  }
};
// the test of a base before its table is built: flag[0] = 1 where a coordinate is >= p or the
// point is not on the curve
template <class CV>
struct FnBaseCheck {
  static constexpr const char* NAME = "base_check";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  const u8* pt; u8* flag;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i) return;
    flag[0] = W::base_ok(pt) ? 0 : 1;
  }
};
// k1 * B1 + k2 * B2 over two fixed-base tables, one item per lane (Work::mul_base2)
template <class CV, int MW = 0>
struct FnMulBase2 {
  static constexpr const char* NAME = "mul_base2";
  typedef Work<CV> W;
  static constexpr int MIN_WAVES = MW ? MW : (W::L <= 8 ? ELL_FIXED_MIN_WAVES : 1);
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* k1; const typename W::A* t1; const u8* k2; const typename W::A* t2; u32* jac;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::mul_base2(i, n, k1, t1, k2, t2, jac);
  }
};
template <class CV>
struct FnNormalize {
  static constexpr const char* NAME = "normalize";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t T; size_t n; int K; const u32* jac; u32* pre; u8* out_xy; u8* out_inf;
  typename W::A* raw;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) W::normalize(t, T, n, K, jac, pre, out_xy, out_inf, raw);
  }
};
// post-pass of the point-valued calls: operands that are not on the curve are outside the
// engine's domain -> out_inf = 2, result zeroed (Work::domain_mark)
template <class CV>
struct FnDomainMark {
  static constexpr const char* NAME = "domain_mark";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* xy1; const u8* xy2; u8* out_xy; u8* out_inf;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::domain_mark(i, xy1, xy2, out_xy, out_inf);
  }
};
struct FnEdDomainMark {
  static constexpr const char* NAME = "ed_domain_mark";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* xy1; const u8* xy2; u8* out_xy; u8* out_inf;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdWork::domain_mark(i, xy1, xy2, out_xy, out_inf);
  }
};
struct FnEdcDomainMark {
  static constexpr const char* NAME = "edc_domain_mark";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* xy1; const u8* xy2; u8* out_xy; u8* out_inf;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdcWork::domain_mark(i, xy1, xy2, out_xy, out_inf);
  }
};
// MW != 0: a second instantiation held to 512 / MW registers (default scheduling strategy): the
// one that runs BESIDE ecdsa_table in the small-grid verify (FnEcdsaPrepTable) -- at 216
// registers two waves of ecdsa_prep leave a SIMD no room for anything else, and the two jobs
// would take turns instead of sharing it (profiles/r04_split_verify_ab.txt)
template <class CV, int MW = 0>
struct FnEcdsaPrep {
  static constexpr const char* NAME = "ecdsa_prep";
  typedef Work<CV> W;
  static constexpr int MIN_WAVES = MW ? MW : 1;
  static constexpr int DS_PER_LANE = 0;
  size_t T; size_t n; int K; const u8* hash; int hash_len; int shift; const u8* r; const u8* s;
  u32* pre; u32* u12; u8* valid;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) W::ecdsa_prep(t, T, n, K, hash, hash_len, shift, r, s, pre, u12, valid);
  }
};
// WIDE: the small-grid tuning (secp256k1 only; Engine::ecdsa_chunk picks it for batches of at most
// ELL_SMALL_GRID items): 3 waves/SIMD worth of registers, beta / zg / u1 resident, table and comb
// entries requested one step ahead.  Same results; 3 % faster where only two waves per SIMD are
// resident and gather latency is exposed, 0.6 % slower on a full grid (profiles/r03_small_grid_ab.jsonl).
template <class CV, int MW = 0, bool WIDE = false>
struct FnEcdsaMain {
  static constexpr const char* NAME = "ecdsa_main";
  typedef Work<CV> W;
  static constexpr int MIN_WAVES = MW ? MW : (W::L <= 8 ? (CV::ENDO ? ELL_ENDO_MIN_WAVES : ELL_ECDSA_MIN_WAVES) : (W::L == 12 ? ELL_P384_MIN_WAVES : ELL_P521_MIN_WAVES));   // 128 VGPRs for secp256k1, <= 168 for the other 256-bit curves, <= 256 for p384
  static constexpr int DS_PER_LANE = W::NWIN * W::NSV;
  size_t n; const u32* u12; const u8* valid; const u8* r; const u8* pub;
  const typename W::A* comb; typename W::VT* tbl; u8* ok; u8* st;
  ELL_HD void operator()(size_t i, const DigitStore& ds) const {
    if (i < n) W::template ecdsa_main<WIDE>(i, n, u12, valid, r, pub, comb, tbl, ds, ok, st);
  }
};
// pass 2 of a verify against a fixed-base table of the signer's key: two comb walks, one item per
// lane (Work::ecdsa_base_main).  FnMulBase2's register budget where the kernel fits it without
// scratch (p192, p224, p256: 90 / 102 / 122 VGPRs); secp256k1 and the run-time field do not (the x
// test with its second candidate behind the two walks: 84 and 112 bytes of scratch per lane at
// 128 registers) and get ELL_ECDSA_BASE_MIN_WAVES = 3 waves' worth, 168 registers.
#ifndef ELL_ECDSA_BASE_MIN_WAVES
#define ELL_ECDSA_BASE_MIN_WAVES 3
#endif
template <class CV, int MW = 0>
struct FnEcdsaBase {
  static constexpr const char* NAME = "ecdsa_base";
  typedef Work<CV> W;
  static constexpr int MIN_WAVES = MW ? MW : (W::L <= 8 ? ((CV::ENDO || CV::RT_ORDER) ? ELL_ECDSA_BASE_MIN_WAVES : ELL_FIXED_MIN_WAVES) : 1);
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u32* u12; const u8* valid; const u8* r;
  const typename W::A* tg; const typename W::A* tq; u8* ok;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::ecdsa_base_main(i, n, u12, valid, r, tg, tq, ok);
  }
};
// the small-grid verify in two kernels (Work::ecdsa_table / ecdsa_ladder): the tables are built
// beside ecdsa_prep (FnEcdsaPrepTable), the ladder after both
template <class CV, bool WIDE = true>
struct FnEcdsaTable {
  static constexpr const char* NAME = "ecdsa_table";
  typedef Work<CV> W;
  static constexpr int MIN_WAVES = ELL_ECDSA_TABLE_MIN_WAVES;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* pub; typename W::VT* tbl;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::template ecdsa_table<WIDE>(i, n, pub, tbl);
  }
};
template <class CV, bool WIDE = true>
struct FnEcdsaLadder {
  static constexpr const char* NAME = "ecdsa_main";      // the timing name of pass 2 in either form
  typedef Work<CV> W;
  static constexpr int MIN_WAVES = WIDE ? 3 : ELL_ENDO_MIN_WAVES;
  static constexpr int DS_PER_LANE = W::NWIN * W::NSV;
  size_t n; const u32* u12; const u8* valid; const u8* r; const u8* pub;
  const typename W::A* comb; const typename W::VT* tbl; u8* ok; u8* st;
  ELL_HD void operator()(size_t i, const DigitStore& ds) const {
    if (i < n) W::template ecdsa_ladder<WIDE>(i, n, u12, valid, r, pub, comb, tbl, ds, ok, st);
  }
};

// ecdsa_prep and ecdsa_table in ONE launch (horizontal fusion): workgroups below `tpad` threads
// run the prep (the 104-register instantiation: at 216 registers two waves of prep would leave a
// SIMD no room for the table workgroups), the others build window tables -- the two jobs share the
// SIMDs without a second stream, without events and without a cross-queue wait before the ladder
template <class CV>
struct FnEcdsaPrepTable {
  static constexpr const char* NAME = "ecdsa_prep_table";
  typedef Work<CV> W;
  static constexpr int MIN_WAVES = ELL_ECDSA_TABLE_MIN_WAVES;
  static constexpr int DS_PER_LANE = 0;
  FnEcdsaPrep<CV, ELL_ECDSA_TABLE_MIN_WAVES> prep; size_t tpad; FnEcdsaTable<CV, true> table;
  ELL_HD void operator()(size_t tid, const DigitStore& ds) const {
    if (tid < tpad) {
      if (fill_lane(tid, prep.T)) prep(tid, ds);
    } else {
      table(tid - tpad, ds);                     // (the launch ends with this range: k_run fills its last wave)
    }
  }
};

// The parted verify (Work::ecdsa_half / ecdsa_fixed / ecdsa_join): batches that leave most SIMDs
// without a wave.  One launch of three regions of `npad` threads -- whole workgroups each, so a
// wave belongs to ONE part -- runs the two half ladders and the comb of every item in different
// waves; the join adds up.  256 registers per lane: a lone chain has no neighbour to make room for.
template <class CV>
struct FnEcdsaParts {
  static constexpr const char* NAME = "ecdsa_parts";
  typedef Work<CV> W;
  static constexpr int MIN_WAVES = 2;
  static constexpr int DS_PER_LANE = W::template Endo<true>::NW;
  size_t n; size_t npad; const u32* u12; const typename W::A* comb; const typename W::VT* tbl; u32* jac;
  ELL_HD void operator()(size_t tid, const DigitStore& ds) const {
    const int part = tid >= 2 * npad ? 2 : (tid >= npad ? 1 : 0);
    size_t i = tid - (size_t)part * npad;
    if (!fill_lane(i, n)) return;
    u32* out = jac + (size_t)part * 3 * W::NS * n;
    if (part == 2) W::ecdsa_fixed(i, n, u12, comb, out);
    else W::template ecdsa_half<true>(i, n, part, u12, tbl, ds, out);
  }
};
template <class CV>
struct FnEcdsaJoin {
  static constexpr const char* NAME = "ecdsa_join";
  typedef Work<CV> W;
  static constexpr int MIN_WAVES = 2;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* valid; const u8* r; const u8* pub; const typename W::VT* tbl; const u32* jac; u8* ok; u8* st;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::template ecdsa_join<true>(i, n, valid, r, pub, tbl, jac, ok, st);
  }
};

// The parts of the parted verify / Point#mul on the LANES-PER-ITEM layer (coop.h, coop_work.h):
// one unit = one part of one item on a wave of its own, its field elements spread over a 16-lane
// row -- 2.2 x fewer instructions on the item's critical path.  Launched through BK::launch_coop
// (k_run_coop: one unit per workgroup) for batches of at most Tuning::coop_grid items; the join
// kernels are the one-lane ones.
// PR: the same parts with ONE ITEM PER ROW of the wave (coop.h FpK256R, coop_work.h CoopK256R): four
// items per unit, for batches between Tuning::row_from and Tuning::row_grid -- too many for a wave
// per part (that layer holds 1 365 verifies at four waves per SIMD), too few for the
// one-item-per-lane kernels, whose chain is 4.4x longer (one 128-bit ladder: 573 us on a lone
// one-lane wave, 130 us on the row layer; 4 096 verifies used 192 of the 1 024 SIMDs).
// Unit u of a part takes items 4 u .. 4 u + 3; rows past the end redo the last item.
ELL_HD size_t row_item(size_t group, int row, size_t n) {
  const size_t i = group * 4 + (size_t)row;
  return i < n ? i : n - 1;
}
// secp256k1's: the two half ladders and the comb of every item
template <bool PR>
struct FnEcdsaPartsK256 {
  static constexpr const char* NAME = PR ? "ecdsa_parts_r" : "ecdsa_parts_c";
  typedef Work<CvSecp256k1> W;
  typedef CoopK256T<PR> CW;
  static constexpr int DS_PER_LANE = CW::E::NW;
  static constexpr int ROW_BYTES = CW::ROW_BYTES;
  size_t n; const u32* u12; const typename W::A* comb; const typename W::VT* tbl; u32* jac;
  ELL_HD void item(int part, size_t i, const DigitStore& ds, u32* out, void* row_mem) const {
    if (part == 2) CW::ecdsa_fixed(i, n, u12, comb, out);
    else CW::ecdsa_half(i, n, part, u12, tbl, ds, out, row_mem);
  }
  ELL_HD void operator()(size_t unit, const DigitStore& ds, void* row_mem) const {
    const size_t groups = PR ? (n + 3) / 4 : n;              // units per part
    const int part = (int)(unit / groups);
    const size_t g = unit - (size_t)part * groups;
    u32* out = jac + (size_t)part * 3 * W::NS * n;
    if constexpr (PR) {
      ELL_FOR_ROWS(row) item(part, row_item(g, row, n), ds, out, row_mem);
    } else {
      item(part, g, ds, out, row_mem);
    }
  }
};
// ... and in front of them, ONE launch: unit i < n runs the scalar-field prep of item i (the
// one-lane code on a wave of its own: range checks, s^-1, u1, u2), unit n + i builds the window
// table of Q_i on the row layer (coop_work.h CoopK256::ecdsa_table) -- the one-lane
// FnEcdsaPrepTable took as long as its table build (86 us against the prep's 55).
struct FnEcdsaPrepTableC {
  static constexpr const char* NAME = "ecdsa_prep_table_c";
  typedef Work<CvSecp256k1> W;
  static constexpr int DS_PER_LANE = 0;
  static constexpr int ROW_BYTES = CoopK256::ROW_BYTES;
  size_t n; const u8* hash; int hash_len; int shift; const u8* r; const u8* s;
  u32* pre; u32* u12; u8* valid; const u8* pub; typename W::VT* tbl;
  ELL_HD void operator()(size_t unit, const DigitStore&, void* row_mem) const {
    // (every lane of the prep's wave runs the one-lane code on the same item and stores the same values)
    if (unit < n) W::ecdsa_prep(unit, n, n, 1, hash, hash_len, shift, r, s, pre, u12, valid);
    else CoopK256::ecdsa_table(unit - n, pub, tbl, row_mem);
  }
};
// ... one item per row: the first units run the scalar-field prep one item per LANE (the one-lane
// code: 64 items per wave, one inversion each -- the chain counts), the others build the window
// tables of the keys four per wave.  (Its prep half is per lane, FnEcdsaPrepTableC's per wave: the
// two stay apart.)
struct FnEcdsaPrepTableR {
  static constexpr const char* NAME = "ecdsa_prep_table_r";
  typedef Work<CvSecp256k1> W;
  static constexpr int DS_PER_LANE = 0;
  static constexpr int ROW_BYTES = CoopK256R::ROW_BYTES;
  size_t n; size_t prep_units; const u8* hash; int hash_len; int shift; const u8* r; const u8* s;
  u32* pre; u32* u12; u8* valid; const u8* pub; typename W::VT* tbl;
  ELL_HD void operator()(size_t unit, const DigitStore&, void* row_mem) const {
    if (unit < prep_units) {
      ELL_FOR_WAVE_LANES(lane) {
        size_t t = unit * 64 + (size_t)lane;
        if (fill_lane(t, n)) W::ecdsa_prep(t, n, n, 1, hash, hash_len, shift, r, s, pre, u12, valid);
      }
    } else {
      ELL_FOR_ROWS(row) CoopK256R::ecdsa_table(row_item(unit - prep_units, row, n), pub, tbl, row_mem);
    }
  }
};
template <bool PR>
struct FnMulPartsK256 {
  static constexpr const char* NAME = PR ? "mul_parts_r" : "mul_parts_c";
  typedef Work<CvSecp256k1> W;
  typedef CoopK256T<PR> CW;
  static constexpr int DS_PER_LANE = CW::E::NW;
  static constexpr int ROW_BYTES = CW::ROW_BYTES;
  // kg != null: k*P + kg*G -- the units of a third range run the comb of kg
  size_t n; const u8* k; const u8* xy; u32* jac; const u8* kg; const typename W::A* comb;
  ELL_HD void item(int part, size_t i, const DigitStore& ds, u32* out, void* row_mem) const {
    if (part == 2) CW::mul_fixed_part(i, n, kg, comb, out);
    else CW::mul_half(i, n, part, k, xy, ds, out, row_mem);
  }
  ELL_HD void operator()(size_t unit, const DigitStore& ds, void* row_mem) const {
    const size_t groups = PR ? (n + 3) / 4 : n;              // units per part
    const int part = (int)(unit / groups);
    const size_t g = unit - (size_t)part * groups;
    u32* out = jac + (size_t)part * 3 * W::NS * n;
    if constexpr (PR) {
      ELL_FOR_ROWS(row) item(part, row_item(g, row, n), ds, out, row_mem);
    } else {
      item(part, g, ds, out, row_mem);
    }
  }
};

// ... and for the NIST curves up to 256 bits (coop_mont.h, coop_work.h CoopNist): a verify is two
// units (u2*Q ladder, u1*G comb), a Point#mul one, k1*G + k2*P two
template <class CV>
struct FnEcdsaPartsN {
  static constexpr const char* NAME = "ecdsa_parts_c";
  typedef Work<CV> W;
  typedef CoopNist<CV> CW;
  static constexpr int DS_PER_LANE = CW::NW;
  static constexpr int ROW_BYTES = CW::ROW_BYTES;
  size_t n; const u32* u12; const u8* pub; const typename W::A* comb; u32* jac; const typename CW::A* gtbl;
  ELL_HD void operator()(size_t unit, const DigitStore& ds, void* row_mem) const {
    const int part = (int)(unit / n);
    const size_t i = unit - (size_t)part * n;
    u32* out = jac + (size_t)part * 3 * W::NS * n;
    if (part == 1) CW::ecdsa_fixed(i, n, u12, comb, out);
    else CW::ecdsa_var(i, n, u12, pub, ds, out, row_mem, gtbl);
  }
};
// ... in front of them, ONE launch: unit i < n runs the scalar-field prep of item i (the one-lane
// code on a wave), unit n + i builds the window table of Q_i -- co-Z chain, the inversion that maps
// it back to the curve, 60 us of the ladder's chain that do not depend on s^-1 -- and leaves it in
// global memory in the row's own format (CoopNist::ecdsa_table)
template <class CV>
struct FnEcdsaPrepTableN {
  static constexpr const char* NAME = "ecdsa_prep_table_c";
  typedef Work<CV> W;
  typedef CoopNist<CV> CW;
  static constexpr int DS_PER_LANE = 0;
  static constexpr int ROW_BYTES = CW::ROW_BYTES;
  size_t n; const u8* hash; int hash_len; int shift; const u8* r; const u8* s;
  u32* pre; u32* u12; u8* valid; const u8* pub; typename CW::A* gtbl;
  ELL_HD void operator()(size_t unit, const DigitStore&, void* row_mem) const {
    if (unit < n) W::ecdsa_prep(unit, n, n, 1, hash, hash_len, shift, r, s, pre, u12, valid);
    else CW::ecdsa_table(unit - n, pub, gtbl, row_mem);
  }
};
template <class CV>
struct FnMulPartsN {
  static constexpr const char* NAME = "mul_parts_c";
  typedef Work<CV> W;
  typedef CoopNist<CV> CW;
  static constexpr int DS_PER_LANE = CW::NW;
  static constexpr int ROW_BYTES = CW::ROW_BYTES;
  // kg != null: k*P + kg*G -- the units of a second range run the comb of kg
  size_t n; const u8* k; const u8* xy; u32* jac; const u8* kg; const typename W::A* comb;
  ELL_HD void operator()(size_t unit, const DigitStore& ds, void* row_mem) const {
    const int part = (int)(unit / n);
    const size_t i = unit - (size_t)part * n;
    u32* out = jac + (size_t)part * 3 * W::NS * n;
    if (part == 1) CW::mul_fixed_part(i, n, kg, comb, out);
    else CW::mul_var(i, n, k, xy, ds, out, row_mem);
  }
};
template <class CV>
struct FnEcdsaJoin2 {
  static constexpr const char* NAME = "ecdsa_join";
  typedef Work<CV> W;
  static constexpr int MIN_WAVES = 2;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* valid; const u8* r; const u8* pub; const u32* jac; u8* ok; u8* st;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::ecdsa_join2(i, n, valid, r, pub, jac, ok, st);
  }
};

// Point#mul in the parted form (Work::mul_half / mul_join)
template <class CV>
struct FnMulParts {
  static constexpr const char* NAME = "mul_parts";
  typedef Work<CV> W;
  static constexpr int MIN_WAVES = 2;
  static constexpr int DS_PER_LANE = W::template Endo<true>::NW;
  // kg != null: k*P + kg*G -- a third range of lanes runs the comb of kg
  size_t n; size_t npad; const u8* k; const u8* xy; typename W::VT* tbl; u32* jac;
  const u8* kg; const typename W::A* comb;
  ELL_HD void operator()(size_t tid, const DigitStore& ds) const {
    const int part = tid >= 2 * npad ? 2 : (tid >= npad ? 1 : 0);
    size_t i = tid - (size_t)part * npad;
    if (!fill_lane(i, n)) return;
    u32* out = jac + (size_t)part * 3 * W::NS * n;
    if (part == 2) W::mul_fixed_part(i, n, kg, comb, out);
    else W::template mul_half<true>(i, n, part, k, xy, tbl + (size_t)part * n * W::template stride<true>(), ds, out);
  }
};
template <class CV>
struct FnMulJoin {
  static constexpr const char* NAME = "mul_join";
  typedef Work<CV> W;
  static constexpr int MIN_WAVES = 2;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u32* jac; bool with_g; const u8* xy; u8* out_xy; u8* out_inf; typename W::A* raw;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::mul_join(i, n, jac, with_g, xy, out_xy, out_inf, raw);
  }
};

template <class CV, int MW = 0>
struct FnSignMul {
  static constexpr const char* NAME = "sign_mul";
  typedef Work<CV> W;
  static constexpr int MIN_WAVES = MW ? MW : (W::L <= 8 ? ELL_FIXED_MIN_WAVES : 1);
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* nonces; const typename W::A* comb; u32* jac;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::sign_mul(i, n, nonces, comb, jac);
  }
};
template <class CV>
struct FnSignFinish {
  static constexpr const char* NAME = "sign_finish";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t T; size_t n; int K; const u8* hash; int hash_len; int shift; const u8* priv;
  const u8* nonces; const u8* kg_xy; const u8* kg_inf; int canonical; u32* pre;
  u8* out_r; u8* out_s; u8* out_recid; u8* out_ok; const u32* kinv;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) W::sign_finish(t, T, n, K, hash, hash_len, shift, priv, nonces, kg_xy, kg_inf, canonical,
                              pre, out_r, out_s, out_recid, out_ok, kinv);
  }
};
// EC#sign's middle for a handful of items, ONE launch of the row layer (k_run_coop): unit i < n
// computes k_i*G on a wave of its own and leaves it affine (coop_work.h coop_sign_point), unit
// n + i inverts k_i mod n beside it (Work::sign_kinv) -- sign_mul, normalize and the inversion of
// sign_finish were three dependent one-lane launches.  CW: CoopK256 / CoopNist<CV>.
template <class CV, class CW>
struct FnSignPartsC {
  static constexpr const char* NAME = "sign_parts_c";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  static constexpr int ROW_BYTES = 16;
  size_t n; const u8* nonces; const typename W::A* comb; u8* kg_xy; u8* kg_inf; u32* kinv;
  ELL_HD void operator()(size_t unit, const DigitStore&, void*) const {
    if (unit < n) coop_sign_point<CW>(unit, nonces, comb, kg_xy, kg_inf);
    else W::sign_kinv(unit - n, n, nonces, kinv, CW::writer());
  }
};
// Point#mul on G / KeyPair#getPublic for a handful of items on the row layer: the comb and the
// item's own inversion on a wave (coop_work.h coop_sign_point -- the point half of sign_parts_c);
// mul_fixed + normalize were two dependent one-lane launches.  The scalar is any BYTES-byte value
// (the comb's windows cover 8 BYTES bits and their carry, as in the one-lane mul_fixed).
template <class CV, class CW>
struct FnMulFixedC {
  static constexpr const char* NAME = "mul_fixed_c";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  static constexpr int ROW_BYTES = 16;
  size_t n; const u8* k; const typename W::A* comb; u8* out_xy; u8* out_inf;
  ELL_HD void operator()(size_t unit, const DigitStore&, void*) const {
    if (unit < n) coop_sign_point<CW, false>(unit, k, comb, out_xy, out_inf);
  }
};
// ShortCurve#pointFromX of a handful of secp256k1 abscissas: the square root's 266 products on a
// wave per item (coop_work.h CoopK256::decompress); FnDecompress is the one-lane form.
struct FnDecompressC {
  static constexpr const char* NAME = "decompress_c";
  static constexpr int DS_PER_LANE = 0;
  static constexpr int ROW_BYTES = 16;
  size_t n; const u8* xs; const u8* odd; u8* out_xy; u8* out_ok;
  ELL_HD void operator()(size_t unit, const DigitStore&, void*) const {
    if (unit < n) CoopK256::decompress(unit, xs, odd, out_xy, out_ok);
  }
};
// EC#recoverPubKey's front for a handful of items, ONE launch: unit i < n lifts R from (r, j) on
// a wave (the square root), unit n + i runs recover_prep for item i beside it (range checks, r^-1,
// both scalars) -- recover_prep and decompress were two dependent one-lane launches, 62 + 103 us.
struct FnRecoverPartsC {
  static constexpr const char* NAME = "recover_parts_c";
  typedef Work<CvSecp256k1> W;
  static constexpr int DS_PER_LANE = 0;
  static constexpr int ROW_BYTES = 16;
  size_t n; const u8* hash; int hash_len; const u8* r; const u8* s; const u8* recid;
  u32* pre; u8* xs; u8* odd; u8* s1; u8* s2; u8* status; u8* rxy; u8* dec_ok;
  ELL_HD void operator()(size_t unit, const DigitStore&, void*) const {
    if (unit < n) CoopK256::recover_point(unit, r, recid, rxy, dec_ok);
    // (every lane of the wave runs the one-lane code on the same item and stores the same values)
    else W::recover_prep(unit - n, n, n, 1, hash, hash_len, r, s, recid, pre, xs, odd, s1, s2, status);
  }
};
template <class CV>
struct FnDetNonce {
  static constexpr const char* NAME = "det_nonce";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* hash; int hash_len; int shift; const u8* priv; u8* nonces;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::det_nonce(i, hash, hash_len, shift, priv, nonces);
  }
};
template <class CV>
struct FnRecoverPrep {
  static constexpr const char* NAME = "recover_prep";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t T, n; int K; const u8* hash; int hash_len; const u8* r; const u8* s; const u8* recid;
  u32* pre; u8* xs; u8* odd; u8* s1; u8* s2; u8* status;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) W::recover_prep(t, T, n, K, hash, hash_len, r, s, recid, pre, xs, odd, s1, s2, status);
  }
};
template <class CV>
struct FnRecoverFinish {
  static constexpr const char* NAME = "recover_finish";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* dec_ok; const u8* inf; u8* out_xy; u8* status;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::recover_finish(i, dec_ok, inf, out_xy, status);
  }
};
// EC#getKeyRecoveryParam in one pass (Work::recid_*): the scalar-field pass before u1 * G + u2 * Q
// and the comparison of the sum's x with r and r + n behind it
template <class CV>
struct FnRecidPrep {
  static constexpr const char* NAME = "recid_prep";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t T, n; int K; const u8* hash; int hash_len; const u8* r; const u8* s;
  u32* pre; u8* u1; u8* u2; u8* status;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) W::recid_prep(t, T, n, K, hash, hash_len, r, s, pre, u1, u2, status);
  }
};
template <class CV>
struct FnRecidFinish {
  static constexpr const char* NAME = "recid_finish";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* r; const u8* xy; const u8* inf; u8* out_recid; u8* status;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::recid_finish(i, r, xy, inf, out_recid, status);
  }
};
template <class CV>
struct FnDecompress {
  static constexpr const char* NAME = "decompress";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* x; const u8* odd; u8* out_xy; u8* out_ok;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if constexpr (CV::F::HAS_SQRT) { if (i < n) W::decompress(i, x, odd, out_xy, out_ok); }
  }
};
struct FnEdDecompress {
  static constexpr const char* NAME = "ed_decompress";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* y; const u8* odd; u8* out_xy; u8* out_ok;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdWork::decompress(i, y, odd, out_xy, out_ok);
  }
};

template <class CV>
struct FnDecodePoint {
  static constexpr const char* NAME = "decode_point";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* enc; size_t len; u8* out_xy; u8* status;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::decode_point(i, enc, len, out_xy, status);
  }
};
template <class CV>
struct FnEncodePoint {
  static constexpr const char* NAME = "encode_point";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* xy; int compact; u8* out;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::encode_point(i, xy, compact, out);
  }
};
template <class CV>
struct FnValidatePoint {
  static constexpr const char* NAME = "validate_point";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* xy; const u8* inf; u8* status; u8* scal;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) {
      W::validate_point(i, xy, inf, status);
      if (scal) W::fill_order(i, scal);
    }
  }
};
template <class CV>
struct FnSigFromDer {
  static constexpr const char* NAME = "sig_from_der";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* der; size_t stride; const u32* der_len; u8* r; u8* s; u8* status;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::sig_from_der(i, der, stride, der_len, r, s, status);
  }
};
template <class CV>
struct FnSigToDer {
  static constexpr const char* NAME = "sig_to_der";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* r; const u8* s; u8* out; size_t stride; u32* out_len;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::sig_to_der(i, r, s, out, stride, out_len);
  }
};
template <class CV>
struct FnWireStatus {
  static constexpr const char* NAME = "wire_status";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* key_st; const u8* sig_st; const u8* ver_st; u8* ok; u8* err;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::wire_status(i, key_st, sig_st, ver_st, ok, err);
  }
};
// user-defined curves: pointFromX and decodePoint over the run-time modulus (Work::rt_*)
struct FnRtDecompress {
  static constexpr const char* NAME = "rt_decompress";
  typedef Work<CvCustom> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* x; const u8* odd; u8* out_xy; u8* status;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::rt_decompress(i, x, odd, out_xy, status);
  }
};
struct FnRtDecodePoint {
  static constexpr const char* NAME = "rt_decode_point";
  typedef Work<CvCustom> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* enc; size_t len; int pl; u8* out_xy; u8* status;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::rt_decode_point(i, enc, len, pl, out_xy, status);
  }
};
// KeyPair#derive, KeyPair#validate and BasePoint#encode on a user-defined short curve
// (Work::rt_ecdh_front / rt_derive_finish / rt_validate_fold / rt_encode_point): the passes in
// front of and behind the variable-base ladder (FnMulVar<CvCustom>, as Point#mul runs it)
struct FnRtEcdhFront {
  static constexpr const char* NAME = "rt_ecdh_front";
  typedef Work<CvCustom> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* pub; size_t len; int pl; u8* pts; u8* dec_st; u8* valid; u8* scal;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::rt_ecdh_front(i, pub, len, pl, pts, dec_st, valid, scal);
  }
};
struct FnRtDeriveFinish {
  static constexpr const char* NAME = "rt_derive_finish";
  typedef Work<CvCustom> W;
  static constexpr int DS_PER_LANE = 0;
  size_t T; size_t n; int K; const u32* jac; const u8* dec_st; const u8* valid; u32* pre; u8* out_x; u8* status;
  u8* err;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) W::rt_derive_finish(t, T, n, K, jac, dec_st, valid, pre, out_x, status, err);
  }
};
struct FnRtValidateFold {
  static constexpr const char* NAME = "rt_validate_fold";
  typedef Work<CvCustom> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* inf; const u8* valid; const u32* jac; u8* status;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::rt_validate_fold(i, n, inf, valid, jac, status);
  }
};
struct FnRtEncodePoint {
  static constexpr const char* NAME = "rt_encode_point";
  typedef Work<CvCustom> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* xy; int compact; int pl; u8* out;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::rt_encode_point(i, xy, compact, pl, out);
  }
};
// EC#recoverPubKey on a user-defined ECDSA domain (Work::rt_recover_*): the scalar-field pass
// (range checks, one inversion of r per K items, s1 = -e/r, s2 = s/r, the x of R) and the status
// fold behind the double-scalar multiplication.  pmn = p mod n travels as an argument: the
// parameter block's bytes are pinned (Engine::register_custom compares them).
struct RtPmodN { u32 w[8]; };
struct FnRtRecoverPrep {
  static constexpr const char* NAME = "rt_recover_prep";
  typedef Work<CvCustomDomain> W;
  static constexpr int DS_PER_LANE = 0;
  size_t T, n; int K; RtPmodN pmn; const u8* hash; int hash_len; const u8* r; const u8* s; const u8* recid;
  u32* pre; u8* xs; u8* odd; u8* s1; u8* s2; u8* status;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) W::rt_recover_prep(t, T, n, K, pmn.w, hash, hash_len, r, s, recid, pre, xs, odd, s1, s2, status);
  }
};
struct FnRtRecoverFinish {
  static constexpr const char* NAME = "rt_recover_finish";
  typedef Work<CvCustomDomain> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* dec_st; const u8* inf; u8* out_xy; u8* status;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::rt_recover_finish(i, dec_st, inf, out_xy, status);
  }
};
// EC#sign on a user-defined ECDSA domain (Work::rt_sign_*): the nonce draw (HmacDRBG over the
// caller's hash H, run-time n.byteLength() and n.bitLength()), k*G over the domain's comb, and the
// scalar-field pass over the run-time n behind the affine conversion.  Everything per-domain they
// need is in the parameter block already (n, nbits).
// candidates per item before ellgpu_custom_sign_det gives up (ELLGPU_CUSTOM_SIGN_MAX_DRAWS): where n lies
// just above a power of two half of all candidates are rejected, so the presets' 16 would not do
constexpr int CUSTOM_SIGN_MAX_DRAWS = 64;
template <class H>
struct FnRtSignNonce {
  static constexpr const char* NAME = "rt_sign_nonce";
  typedef Work<CvCustomDomain> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* hash; int hash_len; int shift; const u8* priv; int draws; u8* nonces;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::template rt_sign_nonce<H>(i, hash, hash_len, shift, priv, draws, nonces);
  }
};
struct FnRtSignMul {
  static constexpr const char* NAME = "rt_sign_mul";
  typedef Work<CvCustomDomain> W;
  static constexpr int MIN_WAVES = ELL_FIXED_MIN_WAVES;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* nonces; const W::A* comb; u32* jac;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::rt_sign_mul(i, n, nonces, comb, jac);
  }
};
struct FnRtSignFinish {
  static constexpr const char* NAME = "rt_sign_finish";
  typedef Work<CvCustomDomain> W;
  static constexpr int DS_PER_LANE = 0;
  size_t T; size_t n; int K; const u8* hash; int hash_len; int shift; const u8* priv;
  const u8* nonces; const u8* kg_xy; const u8* kg_inf; int canonical; u32* pre;
  u8* out_r; u8* out_s; u8* out_recid; u8* out_ok;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) W::rt_sign_finish(t, T, n, K, hash, hash_len, shift, priv, nonces, kg_xy, kg_inf, canonical,
                                 pre, out_r, out_s, out_recid, out_ok);
  }
};
template <class CV>
struct FnPointAdd {
  static constexpr const char* NAME = "point_add";
  typedef Work<CV> W;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* xy1; const u8* inf1; const u8* xy2; const u8* inf2; u32* jac;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) W::point_add(i, n, xy1, inf1, xy2, inf2, jac);
  }
};
struct FnEdPointAdd {
  static constexpr const char* NAME = "ed_point_add";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* xy1; const u8* inf1; const u8* xy2; const u8* inf2; u32* ext;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdWork::point_add(i, n, xy1, inf1, xy2, inf2, ext);
  }
};
struct FnEdDecodePoint {
  static constexpr const char* NAME = "ed_decode_point";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* enc; u8* out_xy; u8* status;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdWork::decode_points(i, enc, out_xy, status);
  }
};
struct FnEdEncodePoint {
  static constexpr const char* NAME = "ed_encode_point";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* xy; u8* out;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdWork::encode_points(i, xy, out);
  }
};
struct FnEdValidatePoint {
  static constexpr const char* NAME = "ed_validate_point";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* xy; const u8* inf; u8* status; u8* scal;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) {
      EdWork::validate_point(i, xy, inf, status);
      if (scal) EdWork::fill_order(i, scal);
    }
  }
};
// third test of KeyPair#validate: status 0 stays 0 only when n * P came out as infinity
struct FnOrderStatus {
  static constexpr const char* NAME = "order_status";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* mul_inf; u8* status;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n && status[i] == 0 && !mul_inf[i]) status[i] = 3;
  }
};

struct FnEddsaVerify {
  static constexpr const char* NAME = "eddsa_verify";
  static constexpr int DS_PER_LANE = EdWork::NWIN;
  static constexpr int MIN_WAVES = 3;          // <= 168 VGPRs (unconstrained it takes 170: 2 waves/SIMD)
  size_t n; const u8* msgs; const u64* off; size_t msg_len; const u8* sigs; const u8* pubs;
  const EdWork::P* comb; EdWork::P* tbl; u8* ok; u8* err;
  ELL_HD void operator()(size_t i, const DigitStore& ds) const {
    if (i >= n) return;
    const u8* m = off ? msgs + off[i] : msgs + i * msg_len;
    u64 len = off ? off[i + 1] - off[i] : (u64)msg_len;
    EdWork::eddsa_verify(i, m, len, sigs + i * 64, pubs + i * 32, comb, tbl, ds, ok, err);
  }
};

// EDDSA#verify against the comb of the signer's key (EdWork::eddsa_verify_base): one item per lane
// at every n, no digit store, no scratch memory.  aw: encodePoint(A) as sha512_prefixed's words,
// computed once per call on the host -- the kernel never loads a key per item.  Launch bounds as
// FnEdMulBase2's (none of its own): 158 VGPRs, three waves per SIMD, no scratch memory.
// ELL_EDDSA_BASE_ONE_ACC: S*G - h*A in one accumulator against the affine R (1), or R + h*A against
// S*G as the reference writes it (0: 166 VGPRs) -- the same bytes, the first 3 % faster
// (docs/EXPERIMENTS.md A10d).
#ifndef ELL_EDDSA_BASE_ONE_ACC
#define ELL_EDDSA_BASE_ONE_ACC 1
#endif
struct FnEddsaBase {
  static constexpr const char* NAME = "eddsa_base";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* msgs; const u64* off; size_t msg_len; const u8* sigs; u64 aw[4];
  const EdWork::P* tg; const EdWork::P* tq; u8* ok; u8* err;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i >= n) return;
    const u8* m = off ? msgs + off[i] : msgs + i * msg_len;
    u64 len = off ? off[i + 1] - off[i] : (u64)msg_len;
    EdWork::eddsa_verify_base<ELL_EDDSA_BASE_ONE_ACC != 0>(i, m, len, sigs + i * 64, aw, tg, tq, ok, err);
  }
};

// EDDSA#verify for a handful of items: the two sides of the equation on a wave each (coop_ed.h),
// then the one-lane comparison
struct FnEddsaPartsC {
  static constexpr const char* NAME = "eddsa_parts_c";
  static constexpr int DS_PER_LANE = EdWork::NWIN;
  static constexpr int ROW_BYTES = CoopEd::ROW_BYTES2;      // (lane_table strides by sixteen entries)
  size_t n; const u8* msgs; const u64* off; size_t msg_len; const u8* sigs; const u8* pubs;
  const EdWork::P* comb; u32* ext; u8* flags;
  ELL_HD void operator()(size_t unit, const DigitStore& ds, void* row_mem) const {
    const int part = (int)(unit / n);
    const size_t i = unit - (size_t)part * n;
    const u8* m = off ? msgs + off[i] : msgs + i * msg_len;
    const u64 len = off ? off[i + 1] - off[i] : (u64)msg_len;
    CoopEd::verify_part(i, n, part, m, len, sigs + i * 64, pubs + i * 32, comb, ds, ext, flags, row_mem);
  }
};
// edwards Point#mul / mulAdd for a handful of items: one item per wave (coop_ed.h), then the
// one-lane normalisation
struct FnEdMulC {
  static constexpr const char* NAME = "ed_mul_c";
  static constexpr int DS_PER_LANE = 2 * EdWork::NWIN;
  static constexpr int ROW_BYTES = CoopEd::ROW_BYTES2;
  // k1 == null: k2*P2; xy1 == null: k1*G + k2*P2
  size_t n; const u8* k1; const u8* xy1; const u8* k2; const u8* xy2; const EdWork::P* comb; u32* ext;
  ELL_HD void operator()(size_t i, const DigitStore& ds, void* row_mem) const {
    if (!k1) CoopEd::mul_var(i, n, k2, xy2, ds, ext, row_mem);
    else CoopEd::mul_add(i, n, k1, xy1, k2, xy2, comb, ds, ext, row_mem);
  }
};
// edwards Point#mul on G for a handful of items: the comb and the inversion on a wave, one launch
struct FnEdMulFixedC {
  static constexpr const char* NAME = "ed_mul_fixed_c";
  static constexpr int DS_PER_LANE = 0;
  static constexpr int ROW_BYTES = 16;
  size_t n; const u8* k; const EdWork::P* comb; u8* out_xy; u8* out_inf;
  ELL_HD void operator()(size_t i, const DigitStore&, void*) const {
    if (i < n) CoopEd::mul_fixed(i, k, comb, out_xy, out_inf);
  }
};
struct FnX25519C {
  static constexpr const char* NAME = "x25519_c";
  static constexpr int DS_PER_LANE = 0;
  static constexpr int ROW_BYTES = CoopX25519::ROW_BYTES;
  // bad != null (KeyPair#derive): units n .. 2 n - 1 test the abscissas beside the ladders
  size_t n; const u8* k; const u8* x; u32* xz; u8* bad;
  ELL_HD void operator()(size_t i, const DigitStore&, void*) const {
    if (i < n) CoopX25519::ladder(i, n, k, x, xz);
    else CoopX25519::validate(i - n, x, bad);
  }
};
struct FnX25519Validate {
  static constexpr const char* NAME = "x25519_validate";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* x; u8* bad;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) MontWork::validate(i, x, bad);
  }
};
struct FnEddsaJoin {
  static constexpr const char* NAME = "eddsa_join";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u32* ext; const u8* flags; u8* ok; u8* err;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdWork::eddsa_join(i, n, ext, flags, ok, err);
  }
};

// Edwards / Montgomery functors
struct FnEddsaSignPre {
  static constexpr const char* NAME = "eddsa_sign_pre";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* secrets; const u8* msgs; const u64* off; size_t msg_len; u8* scal;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i >= n) return;
    const u8* m = off ? msgs + off[i] : msgs + i * msg_len;
    u64 len = off ? off[i + 1] - off[i] : (u64)msg_len;
    EdWork::sign_pre(i, n, secrets + i * 32, m, len, scal);
  }
};
struct FnEddsaSignPost {
  static constexpr const char* NAME = "eddsa_sign_post";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* msgs; const u64* off; size_t msg_len; const u8* scal; const u8* xy;
  u8* sig; u8* pub;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i >= n) return;
    const u8* m = off ? msgs + off[i] : msgs + i * msg_len;
    u64 len = off ? off[i + 1] - off[i] : (u64)msg_len;
    EdWork::sign_post(i, n, m, len, scal, xy, sig, pub);
  }
};
struct FnEdMulVar {
  static constexpr const char* NAME = "ed_mul_var";
  static constexpr int DS_PER_LANE = EdWork::NWIN;
  static constexpr int MIN_WAVES = 4;          // <= 128 VGPRs
  size_t n; const u8* k; const u8* xy; EdWork::P* tbl; u32* ext;
  ELL_HD void operator()(size_t i, const DigitStore& ds) const {
    if (i < n) EdWork::mul_var(i, n, k, xy, tbl, ds, ext);
  }
};
struct FnEdMulFixed {
  static constexpr const char* NAME = "ed_mul_fixed";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* k; const EdWork::P* comb; u32* ext;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdWork::mul_fixed(i, n, k, comb, ext);
  }
};
struct FnEdMulAddG {
  static constexpr const char* NAME = "ed_mul_add_g";
  static constexpr int DS_PER_LANE = EdWork::NWIN;
  size_t n; const u8* k1; const u8* k2; const u8* xy2; const EdWork::P* comb; EdWork::P* tbl;
  u32* ext;
  ELL_HD void operator()(size_t i, const DigitStore& ds) const {
    if (i < n) EdWork::mul_add_g(i, n, k1, k2, xy2, comb, tbl, ds, ext);
  }
};
struct FnEdMulAdd2 {
  static constexpr const char* NAME = "ed_mul_add2";
  static constexpr int DS_PER_LANE = EdWork::NWIN * 2;
  size_t n; const u8* k1; const u8* xy1; const u8* k2; const u8* xy2; EdWork::P* tbl; u32* ext;
  ELL_HD void operator()(size_t i, const DigitStore& ds) const {
    if (i < n) EdWork::mul_add2(i, n, k1, xy1, k2, xy2, tbl, ds, ext);
  }
};
// k1 * B1 + k2 * B2 over the tables of two caller-chosen bases (EdWork::mul_base2)
struct FnEdMulBase2 {
  static constexpr const char* NAME = "ed_mul_base2";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* k1; const EdWork::P* t1; const u8* k2; const EdWork::P* t2; u32* ext;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdWork::mul_base2(i, n, k1, t1, k2, t2, ext);
  }
};
// the comb of a caller-chosen base on an Edwards curve, ed25519 and user-defined alike (32-byte
// scalars, 64-byte points): entry idx = (w, d) gets the scalar d << (bits w), as it stands, and the
// point at pt (x || y big-endian, a device buffer)
// (RT: the user-defined curves' instance, so that each of the two code objects holds its own kernel)
template <bool RT>
struct FnEdBaseCombGen {
  static constexpr const char* NAME = "ed_base_comb_gen";
  static constexpr int DS_PER_LANE = 0;
  size_t n; size_t first; const u8* pt; u8* k; u8* xy; int bits;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i >= n) return;
    const size_t idx = first + i;
    const size_t per = ((size_t)1 << bits) - 1;
    const int w = (int)(idx / per);
    const u32 d = (u32)(idx % per) + 1u;
    const int byte0 = w * (bits / 8);             // bits is 8 or 16: a window is whole bytes
    ELL_NOUNROLL
    for (int b = 0; b < 32; b++) {
      const int j = 31 - b - byte0;                // byte b counts from the big end
      k[i * 32 + b] = (j == 0 || (j == 1 && bits == 16)) ? (u8)(d >> (8 * j)) : (u8)0;
    }
    ELL_NOUNROLL
    for (int b = 0; b < 64; b++) xy[i * 64 + b] = pt[b];
  }
};
// the test of a base before its table is built: flag[0] = 1 where a coordinate is >= p or the
// point is not on the curve
struct FnEdBaseCheck {
  static constexpr const char* NAME = "ed_base_check";
  static constexpr int DS_PER_LANE = 0;
  const u8* pt; u8* flag;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i) return;
    flag[0] = EdWork::base_ok(pt) ? 0 : 1;
  }
};
struct FnEdNormalize {
  static constexpr const char* NAME = "ed_normalize";
  static constexpr int DS_PER_LANE = 0;
  size_t T; size_t n; int K; const u32* ext; u32* pre; u8* out_xy; u8* out_inf; EdWork::P* raw;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) EdWork::normalize(t, T, n, K, ext, pre, out_xy, out_inf, raw);
  }
};
struct FnX25519 {
  static constexpr const char* NAME = "x25519_ladder";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* k; const u8* x; u32* xz;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) MontWork::ladder(i, n, k, x, xz);
  }
};
struct FnX25519Normalize {
  static constexpr const char* NAME = "x25519_normalize";
  static constexpr int DS_PER_LANE = 0;
  size_t T; size_t n; int K; const u32* xz; u32* pre; u8* out_x; u8* out_inf;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) MontWork::normalize(t, T, n, K, xz, pre, out_x, out_inf);
  }
};

// user-defined Edwards curves (edcustom.h)
struct FnEdcMulVar {
  static constexpr const char* NAME = "edc_mul_var";
  static constexpr int DS_PER_LANE = EdcWork::NWIN;
  static constexpr int MIN_WAVES = 3;
  size_t n; const u8* k; const u8* xy; EdcWork::P* tbl; u32* out;
  ELL_HD void operator()(size_t i, const DigitStore& ds) const {
    if (i < n) EdcWork::mul_var(i, n, k, xy, tbl, ds, out);
  }
};
struct FnEdcMulAdd2 {
  static constexpr const char* NAME = "edc_mul_add2";
  static constexpr int DS_PER_LANE = EdcWork::NWIN * 2;
  static constexpr int MIN_WAVES = 3;
  size_t n; const u8* k1; const u8* xy1; const u8* k2; const u8* xy2; EdcWork::P* tbl; u32* out;
  ELL_HD void operator()(size_t i, const DigitStore& ds) const {
    if (i < n) EdcWork::mul_add2(i, n, k1, xy1, k2, xy2, tbl, ds, out);
  }
};
struct FnEdcPointAdd {
  static constexpr const char* NAME = "edc_point_add";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* xy1; const u8* inf1; const u8* xy2; const u8* inf2; u32* out;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdcWork::point_add(i, n, xy1, inf1, xy2, inf2, out);
  }
};
struct FnEdcNormalize {
  static constexpr const char* NAME = "edc_normalize";
  static constexpr int DS_PER_LANE = 0;
  size_t T; size_t n; int K; const u32* proj; u32* pre; u8* out_xy; u8* out_inf;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) EdcWork::normalize(t, T, n, K, proj, pre, out_xy, out_inf);
  }
};
// sums of many k * P terms on the Edwards curves (edsum.h: sum_pair, sum_fold, sum_mark), over the
// work class EW = EdWork (ed25519) or EdcWork (user-defined ids): the pair kernel with the LDS
// columns and the register budget of that family's mul_add2 kernel
template <class EW>
struct EdSumKernels;
template <>
struct EdSumKernels<EdWork> {
  typedef FnEdMulAdd2 MulAdd2;
  static constexpr int MIN_WAVES = 1;
  static constexpr const char* PAIRS = "ed_sum_pairs";
  static constexpr const char* FOLD = "ed_sum_fold";
  static constexpr const char* MARK = "ed_sum_mark";
};
template <>
struct EdSumKernels<EdcWork> {
  typedef FnEdcMulAdd2 MulAdd2;
  static constexpr int MIN_WAVES = FnEdcMulAdd2::MIN_WAVES;
  static constexpr const char* PAIRS = "edc_sum_pairs";
  static constexpr const char* FOLD = "edc_sum_fold";
  static constexpr const char* MARK = "edc_sum_mark";
};
template <class EW>
struct FnEdSumPairs {
  static constexpr const char* NAME = EdSumKernels<EW>::PAIRS;
  static constexpr int DS_PER_LANE = EdSumKernels<EW>::MulAdd2::DS_PER_LANE;
  static constexpr int MIN_WAVES = EdSumKernels<EW>::MIN_WAVES;
  size_t rows, len, m, q0; const u8* k; const u8* xy; typename EW::P* tbl; u32* ext; u8* flag;
  ELL_HD void operator()(size_t i, const DigitStore& ds) const {
    if (i < rows * len) EW::sum_pair(i, rows, len, m, q0, k, xy, tbl, ds, ext, flag);
  }
};
// (the fold is left to the register allocator: 176 VGPRs on ed25519, 168 on user-defined ids, no
// scratch; held to 168 / 128 registers the ed25519 fold spills 44 / 228 bytes)
template <class EW>
struct FnEdSumFold {
  static constexpr const char* NAME = EdSumKernels<EW>::FOLD;
  static constexpr int DS_PER_LANE = 0;
  size_t rows, stride, len; u32* ext; u8* flag; u32* cext; u8* cflag; size_t cn, c0;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < rows * ((len + 1) / 2)) EW::sum_fold(i, rows, stride, len, ext, flag, cext, cflag, cn, c0);
  }
};
template <class EW>
struct FnEdSumMark {
  static constexpr const char* NAME = EdSumKernels<EW>::MARK;
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* cflag; u8* out_xy; u8* out_inf;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EW::sum_mark(i, cflag, out_xy, out_inf);
  }
};
// fixed-base tables of caller-chosen points on user-defined Edwards curves (EdcWork::comb_add)
struct FnEdcMulBase {
  static constexpr const char* NAME = "edc_mul_base";
  static constexpr int DS_PER_LANE = 0;
  static constexpr int MIN_WAVES = 3;
  size_t n; const u8* k; const EdcWork::A* tbl; u32* out;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdcWork::mul_base(i, n, k, tbl, out);
  }
};
struct FnEdcMulBase2 {
  static constexpr const char* NAME = "edc_mul_base2";
  static constexpr int DS_PER_LANE = 0;
  static constexpr int MIN_WAVES = 3;
  size_t n; const u8* k1; const EdcWork::A* t1; const u8* k2; const EdcWork::A* t2; u32* out;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdcWork::mul_base2(i, n, k1, t1, k2, t2, out);
  }
};
struct FnEdcBaseCheck {
  static constexpr const char* NAME = "edc_base_check";
  static constexpr int DS_PER_LANE = 0;
  const u8* pt; u8* flag;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i) return;
    flag[0] = EdcWork::base_ok(pt) ? 0 : 1;
  }
};
// the entries of a table under construction: affine, Montgomery form (EdcWork::normalize<true>)
struct FnEdcBaseNormalize {
  static constexpr const char* NAME = "edc_base_normalize";
  static constexpr int DS_PER_LANE = 0;
  size_t T; size_t n; int K; const u32* proj; u32* pre; EdcWork::A* raw;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) EdcWork::normalize<true>(t, T, n, K, proj, pre, nullptr, nullptr, raw);
  }
};

// the key side of user-defined Edwards curves (edckey.h): the passes in front of and behind the
// ladder (FnEdcMulVar, as Point#mul runs it)
struct FnEdcKeyFrontCoord {
  static constexpr const char* NAME = "edc_key_front_coord";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* v; const u8* odd; int from_y; u8* pts; u8* st; u8* need; u32* nd;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdcKey::front_coord(i, n, v, odd, from_y, pts, st, need, nd);
  }
};
struct FnEdcKeyFrontEnc {
  static constexpr const char* NAME = "edc_key_front_enc";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* enc; size_t len; int pl; u8* pts; u8* st; u8* need; u32* nd;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdcKey::front_enc(i, n, enc, len, pl, pts, st, need, nd);
  }
};
struct FnEdcKeyFrontXy {
  static constexpr const char* NAME = "edc_key_front_xy";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* xy; u8* pts; u8* valid; u8* inf; u8* scal; EdcKey::Scalar order;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdcKey::front_xy(i, xy, pts, valid, inf, scal, order);
  }
};
struct FnEdcKeyQuotient {
  static constexpr const char* NAME = "edc_key_quotient";
  static constexpr int DS_PER_LANE = 0;
  size_t T; size_t n; int K; u32* nd; u32* pre;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) EdcKey::quotient(t, T, n, K, nd, pre);
  }
};
struct FnEdcKeyRoot {
  static constexpr const char* NAME = "edc_key_root";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u32* nd; const u8* pts; const u8* st; const u8* need; u8* out_xy; u8* out_st; u8* valid;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdcKey::root(i, n, nd, pts, st, need, out_xy, out_st, valid);
  }
};
struct FnEdcKeyDeriveFinish {
  static constexpr const char* NAME = "edc_key_derive_finish";
  static constexpr int DS_PER_LANE = 0;
  size_t T; size_t n; int K; const u32* proj; const u8* dec_st; const u8* valid; u32* pre; u8* out_x; u8* status;
  u8* err;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) EdcKey::derive_finish(t, T, n, K, proj, dec_st, valid, pre, out_x, status, err);
  }
};
struct FnEdcKeyValidateFold {
  static constexpr const char* NAME = "edc_key_validate_fold";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* inf; const u8* valid; const u32* proj; u8* status;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdcKey::validate_fold(i, n, inf, valid, proj, status);
  }
};

// ECDSA on a user-defined Edwards domain (edcecdsa.h).  The ladders read G's table through
// STAGE_WORDS / stage_src(): the device backend copies that many words into LDS once per workgroup
// and calls the three-argument form with the copy; a backend without LDS calls the two-argument
// form, which reads the table where it lives.
struct FnEdcEcdsaGTable {
  static constexpr const char* NAME = "edc_ecdsa_gtable";
  static constexpr int DS_PER_LANE = 0;
  u32* gt;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i == 0) EdcEcdsa::g_table(gt);
  }
};
struct FnEdcEcdsaLadder {
  static constexpr const char* NAME = "edc_ecdsa_ladder";
  static constexpr int DS_PER_LANE = EdcWork::NWIN * 2;
  static constexpr int MIN_WAVES = 3;
  static constexpr int STAGE_WORDS = EdcEcdsa::GT_WORDS;
  size_t n; const u32* u12; const u8* pub; const u32* gt; EdcWork::P* tbl; u32* proj; u8* on_curve;
  ELL_HD const u32* stage_src() const { return gt; }
  ELL_HD void operator()(size_t i, const DigitStore& ds, const u32* staged) const {
    if (i < n) EdcEcdsa::verify_ladder(i, n, u12, pub, staged, tbl, ds, proj, on_curve);
  }
  ELL_HD void operator()(size_t i, const DigitStore& ds) const { (*this)(i, ds, gt); }
};
struct FnEdcEcdsaEq {
  static constexpr const char* NAME = "edc_ecdsa_eq";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u32* proj; const u8* valid; const u8* on_curve; const u8* r; u8* ok; u8* st;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) EdcEcdsa::eq_maxwell(i, n, proj, valid, on_curve, r, ok, st);
  }
};
struct FnEdcEcdsaEqAffine {
  static constexpr const char* NAME = "edc_ecdsa_eq_affine";
  static constexpr int DS_PER_LANE = 0;
  size_t T; size_t n; int K; const u32* proj; const u8* valid; const u8* on_curve; const u8* r; u32* pre; u8* ok; u8* st;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) EdcEcdsa::eq_affine(t, T, n, K, proj, valid, on_curve, r, pre, ok, st);
  }
};
struct FnEdcSignMul {
  static constexpr const char* NAME = "edc_sign_mul";
  static constexpr int DS_PER_LANE = EdcWork::NWIN;
  static constexpr int MIN_WAVES = 3;
  static constexpr int STAGE_WORDS = EdcEcdsa::GT_WORDS;
  size_t n; const u8* nonces; const u32* gt; u32* proj;
  ELL_HD const u32* stage_src() const { return gt; }
  ELL_HD void operator()(size_t i, const DigitStore& ds, const u32* staged) const {
    if (i < n) EdcEcdsa::sign_mul(i, n, nonces, staged, ds, proj);
  }
  ELL_HD void operator()(size_t i, const DigitStore& ds) const { (*this)(i, ds, gt); }
};
struct FnEdcSignNorm {
  static constexpr const char* NAME = "edc_sign_norm";
  static constexpr int DS_PER_LANE = 0;
  size_t T; size_t n; int K; const u32* proj; u32* pre; u8* kg_xy; u8* kg_inf;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) EdcEcdsa::sign_norm(t, T, n, K, proj, pre, kg_xy, kg_inf);
  }
};

// user-defined Montgomery curves (montcustom.h)
struct FnMontcLadder {
  static constexpr const char* NAME = "montc_ladder";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* k; const u8* x; u32* xz;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) MontcWork::ladder(i, n, k, x, xz);
  }
};
struct FnMontcValidate {
  static constexpr const char* NAME = "montc_validate";
  static constexpr int DS_PER_LANE = 0;
  size_t n; const u8* x; u8* status;
  ELL_HD void operator()(size_t i, const DigitStore&) const {
    if (i < n) MontcWork::validate(i, x, status);
  }
};
struct FnMontcNormalize {
  static constexpr const char* NAME = "montc_normalize";
  static constexpr int DS_PER_LANE = 0;
  size_t T; size_t n; int K; const u32* xz; u32* pre; const u8* vst; u8* out_x; u8* out_flag;
  ELL_HD void operator()(size_t t, const DigitStore&) const {
    if (t < T) MontcWork::normalize(t, T, n, K, xz, pre, vst, out_x, out_flag);
  }
};

// ---- curve metadata ----------------------------------------------------------
struct CurveInfo {
  const char* name;
  int field_bytes;
  int order_bytes;
  int order_bits;
};
inline const CurveInfo* curve_info(int id) {
  static const CurveInfo tab[CURVE_COUNT] = {
      {"secp256k1", 32, 32, 256}, {"p192", 24, 24, 192}, {"p224", 28, 28, 224},
      {"p256", 32, 32, 256},      {"p384", 48, 48, 384}, {"p521", 66, 66, 521},
      {"ed25519", 32, 32, 253},   {"curve25519", 32, 32, 253}};
  // user-defined short curves (Engine::define_short): every width is 32 bytes whatever the prime's size
  static const CurveInfo custom = {"custom", 32, 32, 256};
  if (id >= CURVE_CUSTOM0 && id < CURVE_CUSTOM0 + CURVE_CUSTOM_MAX) return &custom;
  if (id < 0 || id >= CURVE_COUNT) return nullptr;
  return &tab[id];
}

// where the operands of a batch call live: device pointers, or host buffers that the engine stages
enum class Mem { device, host };

inline bool is_custom(int curve) { return curve >= CURVE_CUSTOM0 && curve < CURVE_CUSTOM0 + CURVE_CUSTOM_MAX; }
// The custom-curve kernels read their modulus from ONE parameter block per device (fp_rt.h):
// calls on user-defined curves are serialised per device, from the upload of the block to the
// end of the call's device work.
inline std::mutex& custom_mutex(int device) {
  static std::mutex m[64];
  return m[(unsigned)device % 64u];
}

// ---- the engine ----------------------------------------------------------------
template <class BK>
class Engine {
 public:
  BK bk;
  std::string err;
  // items per field inversion (Montgomery's trick).  With the division-step inversion the
  // per-item part dominates a thread's work, so the scalar (mod n) kernels, which have nothing
  // else to hide their latency behind, prefer half the batch and twice the wavefronts
  // (ecdsa_prep 0.41 -> 0.34 ms, sign_finish 0.45 -> 0.30 ms per 2^20); normalize is best at 16.
  static constexpr int INV_BATCH = ELL_INV_BATCH;
  static constexpr int INV_BATCH_N = ELL_INV_BATCH / 2;
  // Items per inversion in the scalar-field kernels (ecdsa_prep ...): kmax for batches that fill
  // the device anyway; for smaller ones fewer items per thread, so that the n / K threads still
  // give every SIMD a wave (one inversion costs about what two items' other work does; a batch
  // of 131 072 verifies -- one GPU's share of 2^20 over eight -- ran its prep on 256 waves, one
  // per CU, at the lone-wave issue rate: 0.137 ms of a 1.52 ms pass).  ELLGPU_PREP_K overrides.
  // Batch-size dependent tuning, fixed when the context is created: the device's geometry comes
  // from the backend (compute units of THIS device, not a constant), the developer / test
  // overrides from the environment, read once here -- never at launch time:
  //   ELLGPU_SMALL_GRID    largest batch that takes the small-grid (WIDE) kernels (0 = never);
  //                        default: three waves on every SIMD of the device
  //   ELLGPU_SPLIT_VERIFY  0 keeps small-grid verifies on prep -> ecdsa_main (default: prep ||
  //                        table -> ladder)
  //   ELLGPU_PARTED_GRID   largest batch that takes the parted verify (FnEcdsaParts; 0 = never);
  //                        default: half a wave round -- the two half ladders of every item find a
  //                        SIMD of their own (the comb's waves are short)
  //   ELLGPU_PREP_K        items per inversion in the scalar-field kernels (default: by batch size)
  struct Tuning {
    size_t wave_round;        // lanes of one wave on every SIMD of the device
    size_t small_grid;
    bool split_verify;
    size_t parted_grid;       // largest batch that takes the parted verify (three lanes per item)
    size_t coop_grid;         // largest batch whose parts run on the lanes-per-item layer (a wave per part)
    size_t wide_grid;         // ... of p384 / p521 (one item per wave on the wide layer)
    size_t row_from, row_grid;  // batches of row_from < n <= row_grid items run their parts one item per ROW (four items per wave)
    size_t comb_max_bytes;    // ELLGPU_COMB_MAX_BYTES: fixed-base tables above this are treated as unallocatable (0 = no limit)
    int prep_k;
    int norm_k;
    size_t sum_slice;         // ELLGPU_SUM_SLICE: most pairs of terms per launch of a sum (mul_sum); default CHUNK
  };
  Tuning tune_;
  void init_tuning() {
    tune_.wave_round = (size_t)bk.compute_units() * 4 * 64;
    const char* e = getenv("ELLGPU_SMALL_GRID");
    tune_.small_grid = e ? (size_t)strtoull(e, nullptr, 10) : 3 * tune_.wave_round;
    e = getenv("ELLGPU_SPLIT_VERIFY");
    tune_.split_verify = !(e && e[0] == '0');
    e = getenv("ELLGPU_PARTED_GRID");
    tune_.parted_grid = e ? (size_t)strtoull(e, nullptr, 10) : tune_.wave_round / 2;
    // ELLGPU_COOP_GRID  largest batch whose parts take a WAVE each (coop.h; 0 = never); default:
    //                   four waves per SIMD's worth of verify parts (1 365 items on 256 CUs) --
    //                   measured (profiles/r05_small_batch_forms.jsonl): a pass of 1 365 verifies
    //                   0.64 ms on waves against 0.72 on lanes, of 2 048 0.75 against 0.73; above
    //                   that the waves share SIMDs and the one-lane parts (64 items per wave) win
    e = getenv("ELLGPU_COOP_GRID");
    tune_.coop_grid = e ? (size_t)strtoull(e, nullptr, 10) : (size_t)bk.compute_units() * 4 * 4 / 3;
    // One item per row (four items per wave, a wave 1.3x as long as the one-item wave): measured
    // (profiles/r06_latency_rows_ab.txt) it passes the wave-per-part form at ~2.5 items per CU -- 768
    // verifies 382 -> 310 us -- and holds against the one-lane parted form's single 573-us chain up to
    // ~18 per CU: 4 096 verifies 768 -> 608 us, 4 778 a tie.  ELLGPU_ROW_FROM / ELLGPU_ROW_GRID.
    e = getenv("ELLGPU_WIDE_GRID");
    tune_.wide_grid = e ? (size_t)strtoull(e, nullptr, 10) : tune_.coop_grid;
    e = getenv("ELLGPU_ROW_FROM");
    tune_.row_from = e ? (size_t)strtoull(e, nullptr, 10) : (size_t)bk.compute_units() * 5 / 2;
    e = getenv("ELLGPU_ROW_GRID");
    tune_.row_grid = e ? (size_t)strtoull(e, nullptr, 10) : (size_t)bk.compute_units() * 18;
    e = getenv("ELLGPU_COMB_MAX_BYTES");
    tune_.comb_max_bytes = e ? (size_t)strtoull(e, nullptr, 10) : 0;
    e = getenv("ELLGPU_PREP_K");
    tune_.prep_k = e ? atoi(e) : 0;
    e = getenv("ELLGPU_NORM_K");
    tune_.norm_k = e ? atoi(e) : 0;
    // ELLGPU_SUM_SLICE  most pairs of terms that one launch of mul_sum takes (minimum 1); a sum with
    //                   more pairs is walked in slices of that many.  Default: CHUNK.  A developer /
    //                   test override: it lets small sums reach the slice path.
    e = getenv("ELLGPU_SUM_SLICE");
    tune_.sum_slice = e ? (size_t)strtoull(e, nullptr, 10) : CHUNK;
    if (tune_.sum_slice < 1) tune_.sum_slice = 1;
    if (tune_.sum_slice > CHUNK) tune_.sum_slice = CHUNK;
  }
  bool split_small_verify() const { return tune_.split_verify; }
  size_t coop_grid() const { return CoopK256::AVAILABLE ? tune_.coop_grid : 0; }
  // ... of curve CV: p384 / p521 (the wide layer, coop_wide.h) have a threshold of their own
  // (ELLGPU_WIDE_GRID; default: coop_grid)
  template <class CV>
  size_t coop_grid_of() const {
    if constexpr (!CV::ENDO && CoopConsts<CV>::WIDE) return tune_.wide_grid;
    else return coop_grid();
  }
  // The kernel form of a batch of n items on the endomorphism curve (secp256k1): verify, Point#mul
  // and k1*G + k2*P switch on it (ecdsa_chunk, mul_var_chunk, mul_add_g_chunk).  The one place
  // where the small-batch thresholds meet:
  //   FULL        above small_grid: the full-grid tuning, one item per lane
  //   WIDE        above parted_grid: the register-rich small-grid tuning, one item per lane
  //   PARTS_*     the parted form: the halves (and the comb) of an item as parts of their own, then a join --
  //   PARTS_ROW     row_from < n <= row_grid: one item per row of a wave, four items per unit
  //   PARTS_WAVE    else up to coop_grid: a wave per part
  //   PARTS_LANE    else a lane per part
  // Every other curve type is FULL here: the row-layer gates of the NIST curves, sign, mul_fixed,
  // decompress, recover and EdDSA are their own (coop_grid_of<CV>() / coop_grid() alone).
  enum class Form { FULL, WIDE, PARTS_LANE, PARTS_ROW, PARTS_WAVE };
  template <class CV>
  Form form_for(size_t n) const {
    if constexpr (CV::ENDO && Work<CV>::L <= 8) {
      if (n > tune_.small_grid) return Form::FULL;
      if (n > tune_.parted_grid) return Form::WIDE;
      if (CoopK256::AVAILABLE && n > tune_.row_from && n <= tune_.row_grid) return Form::PARTS_ROW;
      return n <= coop_grid() ? Form::PARTS_WAVE : Form::PARTS_LANE;
    }
    return Form::FULL;
  }
  static bool parted(Form f) { return f != Form::FULL && f != Form::WIDE; }
  // threads (PARTS_LANE: whole workgroups per part but the last) or units of the launch that runs
  // `parts` parts of each of n items
  static size_t part_pad(size_t n) { return (n + 127) & ~(size_t)127; }
  static size_t part_units(Form form, size_t n, size_t parts) {
    if (form == Form::PARTS_WAVE) return parts * n;
    if (form == Form::PARTS_ROW) return parts * ((n + 3) / 4);
    return (parts - 1) * part_pad(n) + n;
  }
  // window width of the curve's fixed-base table in use (0 = not built; ellgpu_ctx_comb_bits)
  int comb_bits(int curve) const {
    if (curve < 0 || curve >= CURVE_COUNT || !comb_[curve]) return 0;
    return comb_bits_[curve] ? comb_bits_[curve] : 8;
  }
  // ... and for the ecdsa_prep that runs BESIDE ecdsa_table (small-grid verify): the two kernels
  // share the SIMDs, so what counts is the work, not the latency of a lone chain -- the largest K
  // that still leaves half a wave round of threads (131 072 items: K = 4, 1.332 -> 1.318 ms per
  // pass; 65 536: K = 2; 16 384: K = 1; profiles/r04_split_verify_ab.txt)
  int inv_batch_beside(size_t n, int kmax) const {
    if (tune_.prep_k >= 1 && tune_.prep_k <= 64) return tune_.prep_k;
    int k = kmax;
    while (k > 1 && n / (size_t)k < tune_.wave_round / 2) k >>= 1;
    return k;
  }
  // items per inversion in normalize (ELLGPU_NORM_K overrides)
  // -- on a batch that leaves SIMDs idle the chain of K items per thread counts, not the inversions
  int norm_batch_for(size_t n) const {
    if (tune_.norm_k >= 1 && tune_.norm_k <= 64) return tune_.norm_k;
    int k = INV_BATCH;
    while (k > 1 && n / (size_t)k < tune_.wave_round / 2) k >>= 1;
    return k;
  }
  int inv_batch_for(size_t n, int kmax) const {
    if (tune_.prep_k >= 1 && tune_.prep_k <= 64) return tune_.prep_k;
    int k = kmax;
    while (k > 1 && n / (size_t)k < 2 * tune_.wave_round) k >>= 1;
    return k;
  }
  // The geometry of a shared-inversion kernel on n items: K items per inversion, hence T threads.
  // field_inv: the kernels that invert in the base field (the normalisations ...); scalar_inv: those
  // that invert mod the order (ecdsa_prep, sign_finish, recover_prep).  launch_inv() takes one.
  struct InvBatch {
    int K;
    size_t T;
    InvBatch(size_t n, int k) : K(k), T((n + K - 1) / K) {}
  };
  InvBatch field_inv(size_t n) const { return InvBatch(n, norm_batch_for(n)); }
  InvBatch scalar_inv(size_t n) const { return InvBatch(n, inv_batch_for(n, INV_BATCH_N)); }
  static constexpr size_t CHUNK = 1u << 21;   // max items per launch (bounds the scratch arena)

  explicit Engine(const BK& b) : bk(b) {
    for (int i = 0; i < COMB_SLOTS; i++) { comb_[i] = nullptr; comb_base_[i] = nullptr; comb_bits_[i] = 0; }
    init_tuning();
  }
  ~Engine() {
    for (int i = 0; i < COMB_SLOTS; i++)
      if (comb_[i]) bk.free_(comb_base_[i] ? comb_base_[i] : comb_[i]);
    for (auto& r : bases_)
      if (!r.alias) bk.free_(r.t.base);
    for (auto& a : scratch_)
      for (auto& s : a)
        if (s.p) bk.free_(s.p);
    for (auto& s : staging_)
      if (s.p) bk.free_(s.p);
  }

  // ---- scratch arena: a few grow-only device buffers ----------------------
  struct Buf { void* p = nullptr; size_t cap = 0; };
  enum { S_TBL = 0, S_JAC, S_PRE, S_U12, S_VALID, S_WIRE, S_COUNT };

  void* grow(Buf& b, size_t bytes) {
    if (bytes <= b.cap) return b.p;
    if (b.p) { bk.sync_all(); bk.free_(b.p); b.p = nullptr; b.cap = 0; }
    size_t want = bytes + bytes / 8;
    b.p = bk.alloc(want);
    if (!b.p) { b.p = bk.alloc(bytes); want = bytes; }
    if (!b.p) return nullptr;
    b.cap = want;
    return b.p;
  }
  void* scratch(int which, size_t bytes) { return grow(scratch_[lane_][which], bytes); }
  // How a chunk body claims its scratch: every buffer once (slot, element type, bytes), in the order
  // in which they are to be allocated, then claimed() once behind the last of them -- E_NOMEM if
  // any of the grows failed.  The only caller of scratch().
  template <class T>
  T* claim(int which, size_t bytes) {
    T* p = (T*)scratch(which, bytes);
    claim_failed_ |= !p;
    return p;
  }
  int claimed() {
    if (!claim_failed_) return E_OK;
    claim_failed_ = false;
    return no_scratch();
  }
  int no_scratch() { return fail(E_NOMEM, "scratch allocation failed"); }

  int fail(int code, const char* msg) { err = msg; return code; }

  // ---- fixed-base comb tables, built on the device with our own kernels ----
  // a built table: entry 0, what was allocated, the window width in use, the allocation's bytes
  struct CombTable { void* comb = nullptr; void* base = nullptr; int bits = 0; size_t bytes = 0; };
  // what build_table has to know of a table: plain numbers, nothing of the curve
  struct TablePlan {
    size_t entries;        // without the header slot
    size_t entry_bytes;
    size_t scalar_bytes;   // of a scalar of the build; a point is x || y of as many bytes each
    int bits;              // the window width
    bool header;           // a slot in front of entry 0 holds the width
    bool limit;            // ELLGPU_COMB_MAX_BYTES applies
    bool check_inf;        // refuse a table that holds the point at infinity
  };
  // The one builder of every fixed-base table: the curve's own variable-base kernel on the scalars
  // d << (bits w) and the base.  gen(m, first, dk, dp) launches the kernel that writes the scalars and
  // points of the entries [first, first + m); fill(m, dk, dp, out_xy, out_inf, dst) launches the
  // ladder and the normalisation that writes them to dst, the place of entry `first`.
  //   Slices.  At most ELL_COMB_SLICE = 2^20 entries at a time: the 22-bit signed comb of the 256-bit
  // curves has 25 M entries = 1.6 GB, and a slice needs 1 GB of window-table scratch.
  //   Header slot.  A format that is walked at several widths carries its width in a slot of one
  // entry's size in front of entry 0 (ladder.h comb_bits_of, EdcWork::comb_add).
  //   Byte limit.  ELLGPU_COMB_MAX_BYTES (developer / test override, read when the context is created)
  // refuses a larger table as if its allocation had failed, before anything is allocated.
  //   check_inf (user-defined short ids, whose bases have no known order): out_xy / out_inf are a
  // slice's entries as bytes, which nobody reads, and their infinity flags, fetched slice by slice.
  // One sync at the end surfaces a failed launch (gen's included).  Every temporary is freed on every
  // way out, and the table itself on failure.
  typedef std::function<void(size_t, size_t, u8*, u8*)> TableGen;
  typedef std::function<int(size_t, const u8*, const u8*, u8*, u8*, void*)> TableFill;
  int build_table(const TablePlan& p, const TableGen& gen, const TableFill& fill, CombTable& out) {
    const size_t S = p.scalar_bytes;
    const size_t hdr = p.header ? p.entry_bytes : 0;
    const size_t bytes = hdr + p.entries * p.entry_bytes;
    const size_t slice = p.entries < (size_t)ELL_COMB_SLICE ? p.entries : (size_t)ELL_COMB_SLICE;
    if (p.limit && tune_.comb_max_bytes && bytes > tune_.comb_max_bytes) return fail(E_NOMEM, "comb table allocation failed");
    u8* base = (u8*)bk.alloc(bytes);
    u8* dk = base ? (u8*)bk.alloc(slice * S) : nullptr;
    u8* dp = dk ? (u8*)bk.alloc(slice * 2 * S) : nullptr;
    u8* dchk = dp && p.check_inf ? (u8*)bk.alloc(slice * (2 * S + 1)) : nullptr;
    u8* dinf = dchk ? dchk + slice * 2 * S : nullptr;
    int rc = dp && (dchk || !p.check_inf) ? E_OK : fail(E_NOMEM, "comb table allocation failed");
    if (rc == E_OK) {
      std::vector<u32> width(p.entry_bytes / 4, 0);
      width[0] = (u32)p.bits;
      if (p.header) bk.h2d(base, width.data(), p.entry_bytes);
      std::vector<u8> flags(p.check_inf ? slice : 0);
      bool holds_inf = false;
      for (size_t first = 0; first < p.entries && rc == E_OK; first += slice) {
        const size_t m = p.entries - first < slice ? p.entries - first : slice;
        gen(m, first, dk, dp);
        rc = fill(m, dk, dp, dchk, dinf, base + hdr + first * p.entry_bytes);
        if (rc == E_OK && p.check_inf) {
          bk.d2h(flags.data(), dinf, m);
          if (bk.sync() == E_OK)
            for (size_t i = 0; i < m; i++) holds_inf |= flags[i] != 0;
        }
      }
      const int src = bk.sync();
      if (rc == E_OK && src != E_OK) rc = fail(src, "building the fixed-base table failed on the device");
      if (rc == E_OK && holds_inf) rc = fail(E_ARG, "a multiple of the base inside the table is the point at infinity");
    }
    if (dchk) bk.free_(dchk);
    if (dp) bk.free_(dp);
    if (dk) bk.free_(dk);
    if (rc) {
      if (base) bk.free_(base);
      return rc;
    }
    out.comb = base + hdr;
    out.base = base;
    out.bits = p.bits;
    out.bytes = bytes;
    return E_OK;
  }
  // The test of a caller-chosen base before its table is built (Chk: FnBaseCheck<CV>, FnEdBaseCheck
  // or FnEdcBaseCheck; B: the bytes of a coordinate).  Returns the device copy of x || y for the
  // table's generator to read, which the caller frees; null with rc set where the base is refused.
  // test == false (a curve's own generator) only makes the copy.
  template <class Chk>
  u8* checked_base(const u8* xy, size_t B, bool test, int& rc) {
    u8* dpt = (u8*)bk.alloc(2 * B + 1);            // the point and, behind it, the test's flag
    if (!dpt) { rc = no_scratch(); return nullptr; }
    u8 flag = test ? 1 : 0;
    bk.h2d(dpt, xy, 2 * B);
    if (test) {
      Chk chk{dpt, dpt + 2 * B};
      bk.launch(chk, 1);
      bk.d2h(&flag, dpt + 2 * B, 1);
    }
    rc = bk.sync();
    if (rc) rc = fail(rc, "testing the base failed on the device");
    else if (flag) rc = fail(E_ARG, "the base is not a point of the curve (a coordinate >= p, or off the curve)");
    if (rc) { bk.free_(dpt); dpt = nullptr; }
    return dpt;
  }
  template <class CV>
  int ensure_comb();
  template <class CV>
  int normalize_chunk(size_t n, const u32* jac, u8* out_xy, u8* out_inf, typename Work<CV>::A* raw);
  template <class CV>
  int mul_var_chunk(size_t n, const u8* k, const u8* xy, u8* out_xy, u8* out_inf,
                    typename Work<CV>::A* raw);
  // fixed-base tables of caller-chosen points on Edwards curves (define_ed_base): the test of the
  // base and the build of its table; k1 * B1 (k2 == null) or k1 * B1 + k2 * B2 over built tables, one
  // item per lane at every n.  ed_*: ed25519, tables in EdWork's cached format (own: the curve's own
  // comb, ensure_ed_comb); edc_*: user-defined.
  template <int U = 0>
  int ed_base_table(const u8* xy, bool own, CombTable& out);
  template <int U = 0>
  int ed_base_mul_chunk(size_t n, const u8* k1, const EdWork::P* t1, const u8* k2, const EdWork::P* t2,
                        u8* out_xy, u8* out_inf);
  template <int U = 0>
  int edc_base_table(const u8* xy, int window_bits, CombTable& out);
  template <int U = 0>
  int edc_base_mul_chunk(size_t n, const u8* k1, const EdcWork::A* t1, const u8* k2, const EdcWork::A* t2,
                         u8* out_xy, u8* out_inf);
  // k * B over a comb (the curve's own table for mul_fixed, a caller-chosen base's for mul_base), or
  // with k2: k * B + k2 * B2 over two tables, one item per lane at every n
  template <class CV>
  int mul_fixed_chunk(size_t n, const u8* k, const typename Work<CV>::A* comb, const u8* k2,
                      const typename Work<CV>::A* t2, u8* out_xy, u8* out_inf);
  // a short curve's comb through build_table: gen(m, first, dk, dp, cb) at the width cb in use.  cb:
  // the width to start from; narrow: go on to narrower signed combs on E_NOMEM; check_inf: TablePlan's
  template <class CV, class Gen>
  int build_comb(int cb, bool narrow, bool check_inf, Gen gen, CombTable& out);
  // tests a caller-chosen base on the device and builds its table (define_base)
  template <class CV>
  int base_table(const u8* xy, int window_bits, CombTable& out);
  template <class CV>
  int mul_add2_chunk(size_t n, const u8* k1, const u8* xy1, const u8* k2, const u8* xy2,
                     u8* out_xy, u8* out_inf);
  template <class CV>
  int mul_add_g_chunk(size_t n, const u8* k1, const u8* k2, const u8* xy2, u8* out_xy,
                      u8* out_inf);
  // n sums of m terms each (mul_sum): sum_pairs, the halving steps of sum_fold, one normalisation
  // per sum, sum_mark.  Either the pairs and the results of all n sums fit one chunk
  // (sum_group_max), or n == 1 and the sum is walked in slices.
  template <class CV>
  int sum_chunk(size_t n, size_t m, const u8* k, const u8* xy, u8* out_xy, u8* out_inf);
  template <class CV>
  int ecdsa_chunk(size_t n, const u8* hash, int hash_len, int shift, const u8* r, const u8* s,
                  const u8* pub, u8* ok, u8* st);
  // a verify chunk against the table tq of the signer's key and G's table tg: the scalar-field prep
  // as ecdsa_chunk's, then the two comb walks, one item per lane at every n
  template <class CV>
  int ecdsa_base_chunk(size_t n, const u8* hash, int hash_len, int shift, const u8* r, const u8* s,
                       const typename Work<CV>::A* tg, const typename Work<CV>::A* tq, u8* ok);
  // The two routes of a launch.  They run the same code on the host and are NOT interchangeable:
  //   bk.launch(f, n)   compiles the kernel where the calling chunk body is compiled;
  //   launch_fn(f, n)   compiles it in the translation unit whose group lists launch_fn<Fn> in
  //                     engine_extern.h -- a member of its own, not inline, for that reason alone.
  // The unit fixes the kernel's compile flags (group 6, the scalar-field kernels ecdsa_prep,
  // sign_finish, recover_prep: LLVM's max-ILP scheduling, measured ecdsa_prep 0.334 -> 0.234 ms per
  // 2^20, while the ladder kernels are 0.4-1.3 % slower under it and keep the default) and, on
  // user-defined curves, the parameter block it reads: g_rt (group 16), g_rt_dom (17) or g_rt_ed (18,
  // inst.hip).  The Edwards domain's chunk bodies are compiled in group 18 and are correct only
  // because the short domain's scalar-field kernels they launch (ecdsa_prep, rt_sign_nonce,
  // rt_sign_finish) go through the launch_fn of group 17, where n is.  Moving a launch from one
  // route to the other moves its kernel: check the per-unit kernel lists of a --remarks build.
  // (An Fn that engine_extern.h does not list is compiled where launch_fn is called, as by bk.launch.)
  template <class Fn>
  int launch_fn(const Fn& f, size_t nthreads);
  // The one launch of a shared-inversion kernel: Fn{T, n, K, rest...} on T threads, on the route
  // that the call names.
  enum class Route { here, unit };      // bk.launch / launch_fn
  template <Route R, class Fn, class... A>
  int launch_inv(InvBatch g, size_t n, A... rest) {
    Fn f{g.T, n, g.K, rest...};
    if constexpr (R == Route::unit) return launch_fn(f, g.T);
    else bk.launch(f, g.T);         // (else: the branch not taken must not be instantiated)
    return E_OK;
  }
  // the HmacDRBG nonces of a sign chunk on a user-defined domain, short or Edwards, over the hash
  // drbg_hash (ELLGPU_HASH_*): the short domain's kernels (group 17)
  int draw_nonces(int drbg_hash, size_t n, const u8* hash, int hash_len, int shift, const u8* priv, u8* drawn) {
    if (drbg_hash == 0) return launch_fn(FnRtSignNonce<Sha256>{n, hash, hash_len, shift, priv, CUSTOM_SIGN_MAX_DRAWS, drawn}, n);
    if (drbg_hash == 1) return launch_fn(FnRtSignNonce<Sha384>{n, hash, hash_len, shift, priv, CUSTOM_SIGN_MAX_DRAWS, drawn}, n);
    return launch_fn(FnRtSignNonce<Sha512>{n, hash, hash_len, shift, priv, CUSTOM_SIGN_MAX_DRAWS, drawn}, n);
  }
  template <int U = 0>
  int ensure_ed_comb();
  template <int U = 0>
  int ed_normalize_chunk(size_t n, const u32* ext, u8* out_xy, u8* out_inf, EdWork::P* raw);
  template <int U = 0>
  int ed_mul_var_chunk(size_t n, const u8* k, const u8* xy, u8* out_xy, u8* out_inf, EdWork::P* raw);
  template <int U = 0>
  int ed_mul_fixed_chunk(size_t n, const u8* k, u8* out_xy, u8* out_inf);
  template <int U = 0>
  int ed_mul_add2_chunk(size_t n, const u8* k1, const u8* xy1, const u8* k2, const u8* xy2,
                        u8* out_xy, u8* out_inf);
  // n sums of m terms each on an Edwards curve (ed_mul_sum), EW = EdWork on ed25519, EdcWork on a
  // user-defined id: sum_chunk's shape over that work class -- the pair kernel, the halving steps,
  // one normalisation per sum, the mark.  Either the pairs and the results of all n sums fit one
  // chunk (sum_group_max), or n == 1 and the sum is walked in slices.
  template <class EW>
  int ed_sum_chunk(size_t n, size_t m, const u8* k, const u8* xy, u8* out_xy, u8* out_inf);
  template <int U = 0>
  int x25519_chunk(size_t n, const u8* k, const u8* x, u8* out_x, u8* out_inf, u8* out_bad);
  // user-defined Edwards curves: op 0 = k*P, 1 = k1*P1 + k2*P2, 2 = P1 + P2 (a, b = the inf flags)
  template <int U = 0>
  int edc_chunk(int op, size_t n, const u8* k1, const u8* xy1, const u8* k2, const u8* xy2,
                const u8* a, const u8* b, u8* out_xy, u8* out_inf);
  // the key side of user-defined Edwards curves (edckey.h).  edk_point_chunk: pointFromX / pointFromY
  // (len == 0: a = the coordinates, b = the parities) or decodePoint (a = encodings of len bytes)
  // through front, quotient and root; with `valid` the point goes to the ladder's operand buffer.
  // edk_derive_chunk: KeyPair#derive of raw (len == 0) or SEC1 keys; edk_validate_chunk:
  // KeyPair#validate, order == null without the order test.
  template <int U = 0>
  int edk_point_chunk(size_t n, const u8* a, const u8* b, int from_y, size_t len, u8* out_xy, u8* out_st, u8* valid);
  // edk_point_chunk's three passes over buffers that the caller holds: pts n x 64 bytes, flags 3 n
  // (the status, what the root pass owes each item; the third n are the caller's), nd n x 24 words
  template <int U = 0>
  void edk_point_passes(size_t n, const u8* a, const u8* b, int from_y, size_t len, u8* pts, u8* flags, u32* nd,
                        u8* out_xy, u8* out_st, u8* valid);
  template <int U = 0>
  int edk_derive_chunk(size_t n, const u8* k, const u8* pub, size_t len, u8* out_x, u8* status, u8* err);
  template <int U = 0>
  int edk_validate_chunk(size_t n, const u8* xy, const u8* order, u8* status);
  template <int U = 0>
  int edk_encode_chunk(size_t n, const u8* xy, int compact, u8* out_enc);
  // user-defined Montgomery curves: op 0 = Point#mul + getX (flag: Z == 0), 1 = MontCurve#validate
  // (k, out_x unused), 2 = KeyPair#derive (validate, ladder, getX; flag: the derive status)
  template <int U = 0>
  int montc_chunk(int op, size_t n, const u8* k, const u8* x, u8* out_x, u8* out_flag);
  // wire formats on user-defined short curves (OP_RT_*): pointFromX, decodePoint, the DER parser
  // and the wire verify's status fold -- the kernels of one code object (inst.hip group 16)
  template <int U = 0>
  int rt_wire_chunk(int op, size_t n, const u8* a, const u8* b, size_t len, const u32* lens, u8* o1, u8* o2,
                    u8* o3);
  // KeyPair#derive and #validate on user-defined short curves: rt_ecdh_front, the variable-base
  // ladder of mul_var_chunk (FnMulVar<CvCustom>; none for a validate without the order test), then
  // rt_derive_finish or rt_validate_fold -- the same code object.
  //   derive:   k = the private keys, pub = raw x || y (len == 0) or SEC1 encodings of len bytes,
  //             err may be null
  //   validate: pub = raw x || y, inf may be null
  template <int U = 0>
  int rt_derive_chunk(size_t n, const u8* k, const u8* pub, size_t len, u8* out_x, u8* status, u8* err);
  template <int U = 0>
  int rt_validate_chunk(size_t n, const u8* xy, const u8* inf, bool check_order, u8* status);
  // BasePoint#encode at the curve's own width
  template <int U = 0>
  int rt_encode_chunk(size_t n, const u8* xy, int compact, u8* out_enc);
  // the front pass and the ladder shared by the two above: flags (valid, then the decoder's
  // status) and, with `ladder`, the Jacobian results; the scalars are k, or the order (k == null)
  template <int U = 0>
  int rt_ecdh_ladder(size_t n, const u8* k, const u8* pub, size_t len, bool ladder, u8*& flags, u32*& jac);
  // EC#recoverPubKey on a user-defined ECDSA domain: rt_recover_prep, the run-time square root
  // (rt_wire_chunk), s1 * G + s2 * R over the domain's comb, rt_recover_finish
  template <int U = 0>
  int rt_recover_chunk(size_t n, const u8* hash, int hash_len, const u8* r, const u8* s, const u8* recid,
                       u8* out_xy, u8* out_status);
  // EC#sign on a user-defined ECDSA domain: rt_sign_nonce (nonces == null: drawn over drbg_hash),
  // rt_sign_mul, normalize, rt_sign_finish
  template <int U = 0>
  int rt_sign_chunk(size_t n, const u8* hash, int hash_len, int shift, const u8* priv, const u8* nonces,
                    int drbg_hash, int canonical, u8* out_r, u8* out_s, u8* out_recid, u8* out_ok);
  // ECDSA on a user-defined Edwards domain (edcecdsa.h; inst.hip group 18).  verify: the short
  // domain's ecdsa_prep, edc_ecdsa_ladder, then edc_ecdsa_eq (eqXToP) or edc_ecdsa_eq_affine
  // (no _maxwellTrick).  sign: the short domain's rt_sign_nonce and rt_sign_finish around
  // edc_sign_mul and edc_sign_norm.  ensure_ed_gtable: G's table of the call's domain, once.
  template <int U = 0>
  int ensure_ed_gtable();
  template <int U = 0>
  int edc_verify_chunk(size_t n, const u8* hash, int hash_len, int shift, const u8* r, const u8* s, const u8* pub,
                       u8* ok, u8* st);
  template <int U = 0>
  int edc_sign_chunk(size_t n, const u8* hash, int hash_len, int shift, const u8* priv, const u8* nonces,
                     int drbg_hash, int canonical, u8* out_r, u8* out_s, u8* out_recid, u8* out_ok);
  template <class CV>
  int decompress_chunk(size_t n, const u8* x, const u8* odd, u8* out_xy, u8* out_ok);
  template <class CV>
  int codec_chunk(int op, size_t n, const u8* in, size_t len, int flag, const u8* inf, u8* out, u8* status);
  template <class CV>
  int point_add_chunk(size_t n, const u8* xy1, const u8* inf1, const u8* xy2, const u8* inf2, u8* out_xy, u8* out_inf);
  template <int U = 0>
  int ed_point_add_chunk(size_t n, const u8* xy1, const u8* inf1, const u8* xy2, const u8* inf2, u8* out_xy, u8* out_inf);
  template <class CV>
  int der_chunk(int op, size_t n, const u8* a, const u8* b, size_t stride, u32* lens, u8* o1, u8* o2, u8* o3);
  template <class CV>
  int sign_chunk(size_t n, const u8* hash, int hash_len, int shift, const u8* priv, const u8* nonces,
                 int canonical, u8* out_r, u8* out_s, u8* out_recid, u8* out_ok);
  template <class CV>
  int sign_det_chunk(size_t n, const u8* hash, int hash_len, int shift, const u8* priv, int canonical,
                     u8* out_r, u8* out_s, u8* out_recid, u8* out_ok);
  template <class CV>
  int recover_chunk(size_t n, const u8* hash, int hash_len, const u8* r, const u8* s, const u8* recid,
                    u8* out_xy, u8* out_status);
  // EC#getKeyRecoveryParam: recid_prep, u1 * G + u2 * Q in whatever form mul_add_g_chunk takes at
  // this n, recid_finish
  template <class CV>
  int recid_chunk(size_t n, const u8* hash, int hash_len, const u8* r, const u8* s, const u8* pub_xy,
                  u8* out_recid, u8* out_status);
  template <int U = 0>
  int ed_decompress_chunk(size_t n, const u8* y, const u8* odd, u8* out_xy, u8* out_ok);
  template <int U = 0>
  int ed_codec_chunk(int op, size_t n, const u8* in, int flag, const u8* inf, u8* out, u8* status);
  template <int U = 0>
  int eddsa_chunk(size_t n, size_t o, const u8* msgs, const u64* off, size_t msg_len, const u8* sigs,
                  const u8* pubs, u8* ok, u8* err);
  // a verify chunk against the comb tq of the signer's key, whose encoding is aw, and G's comb tg
  template <int U = 0>
  int eddsa_base_chunk(size_t n, size_t o, const u8* msgs, const u64* off, size_t msg_len, const u8* sigs,
                       const u64 (&aw)[4], const EdWork::P* tg, const EdWork::P* tq, u8* ok, u8* err);
  template <int U = 0>
  int eddsa_sign_chunk(size_t n, size_t o, const u8* secrets, const u8* msgs, const u64* off,
                       size_t msg_len, u8* sig, u8* pub);

  // ---- dispatch over curves (device pointers) --------------------------------
#if defined(ELL_ONLY_CURVE)
// developer build (elliptic_amd/build.py --dev <curve>): one short curve's kernels only, for
// fast kernel iteration; every other short curve reports E_UNSUPPORTED
#define ELL_SHORT_DISPATCH(curve, CALL)                         \
  switch (curve) {                                              \
    case ELL_ONLY_CURVE: { typedef ELL_ONLY_TYPE CV; CALL; } break; \
    default: return fail(E_UNSUPPORTED, is_custom(curve) ? "not available on user-defined curves (scalar multiplication and point addition only)" : "developer build: single curve only"); \
  }
#else
#define ELL_SHORT_DISPATCH(curve, CALL)                         \
  switch (curve) {                                              \
    case CURVE_SECP256K1: { typedef CvSecp256k1 CV; CALL; } break; \
    case CURVE_P192: { typedef CvP192 CV; CALL; } break;           \
    case CURVE_P224: { typedef CvP224 CV; CALL; } break;           \
    case CURVE_P256: { typedef CvP256 CV; CALL; } break;           \
    case CURVE_P384: { typedef CvP384 CV; CALL; } break;           \
    case CURVE_P521: { typedef CvP521 CV; CALL; } break;           \
    default: return is_custom(curve) ? fail(E_UNSUPPORTED, "not available on user-defined curves (scalar multiplication and point addition only)") \
                                     : fail(E_ARG, "unknown curve id");            \
  }
#endif

  // ---- user-defined short Weierstrass curves (run-time prime, arbitrary a) ----------------
  // `new elliptic.curve.short({p, a, b})` (short.js:11-24) with parameters that are no preset:
  // p an odd prime < 2^256 (primality is the caller's business, as it is the reference's), a and
  // b any residues.  Registers the curve under an id >= CURVE_CUSTOM0 of this context; Point#mul,
  // mulAdd / jmulAdd and Point#add then run on the device through the generic-a doubling
  // (ShortOps::dbl, A_KIND 1) and a Montgomery field whose modulus is a kernel-time constant.
  // The parameter block is built by rt_define.h (host arithmetic, no engine) and registered here.
  int register_custom(const RtField& f, int* out_curve) {
    for (size_t i = 0; i < custom_.size(); i++)
      if (memcmp(&custom_[i], &f, sizeof(f)) == 0) { *out_curve = CURVE_CUSTOM0 + (int)i; return E_OK; }
    if ((int)custom_.size() >= CURVE_CUSTOM_MAX)
      return fail(E_UNSUPPORTED, "at most 16 user-defined curves per context");
    custom_.push_back(f);
    RtPmodN pmn;
    rt_p_mod_n(f, pmn.w);
    custom_pmn_.push_back(pmn);
    // an Edwards block carries neither Red#sqrt's constants nor p.byteLength() (its bytes are
    // pinned): the key-side calls (custom_ed_*) upload this copy, which has them, in its place
    RtField aug = f;
    if (f.kind == 1) rt_sqrt_init(aug);
    custom_aug_.push_back(aug);
    *out_curve = CURVE_CUSTOM0 + (int)custom_.size() - 1;
    return E_OK;
  }
  // a built block -> its id, a refusal -> fail()
  int define(const RtStatus& st, const RtField& f, int* out_curve) {
    return st.code ? fail(st.code, st.msg) : register_custom(f, out_curve);
  }
  int define_short(const u8* p_be, const u8* a_be, const u8* b_be, int* out_curve) {
    if (!out_curve) return fail(E_ARG, "null pointer");
    RtField f;
    return define(rt_build_custom(0, p_be, a_be, b_be, f), f, out_curve);
  }
  // An ECDSA domain on a user-defined short curve: EC#verify, k*G and mulAdd with G on the device
  int define_short_domain(const u8* p_be, const u8* a_be, const u8* b_be, const u8* n_be, const u8* gx_be,
                          const u8* gy_be, int* out_curve) {
    if (!out_curve) return fail(E_ARG, "null pointer");
    RtField f;
    return define(rt_build_domain(p_be, a_be, b_be, n_be, gx_be, gy_be, f), f, out_curve);
  }
  // `new elliptic.curve.edwards({p, a, c: 1, d})` (edwards.js:11-31) with parameters that are not
  // ed25519's: a x^2 + y^2 = 1 + d x^2 y^2 over an odd prime p < 2^256; Point#mul, mulAdd and
  // Point#add run on the device in projective coordinates (edcustom.h).
  int define_edwards(const u8* p_be, const u8* a_be, const u8* d_be, int* out_curve) {
    if (!out_curve) return fail(E_ARG, "null pointer");
    RtField f;
    return define(rt_build_custom(1, p_be, a_be, d_be, f), f, out_curve);
  }
  // An ECDSA domain on a user-defined Edwards curve: EC#verify and EC#sign on the device
  // (custom_ed_verify_*, custom_ed_sign_*), and everything a plain define_edwards id can do
  int define_edwards_domain(const u8* p_be, const u8* a_be, const u8* d_be, const u8* n_be, const u8* gx_be,
                            const u8* gy_be, int* out_curve) {
    if (!out_curve) return fail(E_ARG, "null pointer");
    RtField f;
    return define(rt_build_edwards_domain(p_be, a_be, d_be, n_be, gx_be, gy_be, f), f, out_curve);
  }
  // `new elliptic.curve.mont({p, a, b})` (mont.js:11-21) with parameters that are not curve25519's:
  // b y^2 = x^3 + a x^2 + x over an odd prime p < 2^256, x-only; Point#mul + getX,
  // MontCurve#validate and KeyPair#derive run on the device (montcustom.h).  No b: no formula reads it.
  int define_mont(const u8* p_be, const u8* a_be, int* out_curve) {
    if (!out_curve) return fail(E_ARG, "null pointer");
    RtField f;
    return define(rt_build_custom(2, p_be, a_be, nullptr, f), f, out_curve);
  }
  // the id a definition WOULD get (the existing one for parameters already registered, else the
  // next free one), -1 when the table is full; registers nothing.  Invalid parameters report the
  // next free id: the definition itself then fails with its own message, on the first member.
  // edwards: 0 short, 1 Edwards, 2 Montgomery (bd_be unused); dom: n, gx, gy of an ECDSA domain
  // (edwards = 0), else null
  int custom_slot_for(int edwards, const u8* p_be, const u8* a_be, const u8* bd_be,
                      const u8* const* dom = nullptr) {
    RtField f;
    const int rc = (dom ? (edwards ? rt_build_edwards_domain(p_be, a_be, bd_be, dom[0], dom[1], dom[2], f)
                                   : rt_build_domain(p_be, a_be, bd_be, dom[0], dom[1], dom[2], f))
                        : rt_build_custom(edwards, p_be, a_be, bd_be, f)).code;
    if (rc == E_OK)
      for (size_t i = 0; i < custom_.size(); i++)
        if (memcmp(&custom_[i], &f, sizeof(f)) == 0) return CURVE_CUSTOM0 + (int)i;
    if ((int)custom_.size() >= CURVE_CUSTOM_MAX) return rc == E_OK ? -1 : CURVE_CUSTOM0 + (int)custom_.size();
    return CURVE_CUSTOM0 + (int)custom_.size();
  }
  static size_t pipe_step_default() {
    const char* e = getenv("ELLGPU_PIPE_STEP");          // developer override
    int v = e ? atoi(e) : ELL_PIPE_STEP_DEFAULT;
    return (size_t)(v >= 1 && v <= 64 ? v : ELL_PIPE_STEP_DEFAULT);
  }
  bool custom_is_edwards(int curve) const {
    size_t slot = (size_t)(curve - CURVE_CUSTOM0);
    return is_custom(curve) && slot < custom_.size() && custom_[slot].kind == 1;
  }
  bool custom_is_mont(int curve) const {
    size_t slot = (size_t)(curve - CURVE_CUSTOM0);
    return is_custom(curve) && slot < custom_.size() && custom_[slot].kind == 2;
  }
  // an ECDSA domain on a SHORT curve: what the comb, ecdsa_verify, mul_fixed and mul_add2 without p1
  // ask for.  An Edwards domain (kind 1, domain 1) is none: those calls treat it as the plain
  // Edwards curve it also is.
  bool custom_is_domain(int curve) const {
    size_t slot = (size_t)(curve - CURVE_CUSTOM0);
    return is_custom(curve) && slot < custom_.size() && custom_[slot].kind == 0 && custom_[slot].domain == 1;
  }
  // the parameter block of a user-defined curve, null for an id that is none of this context's
  // (the white-box field probes read it: ellgpu_debug_field_op, tests/hostsim)
  const RtField* custom_block(int curve) const {
    size_t slot = (size_t)(curve - CURVE_CUSTOM0);
    return is_custom(curve) && slot < custom_.size() ? &custom_[slot] : nullptr;
  }
  // where the fixed-base table of a curve type lives: the presets' by their id, a domain's in the
  // slot of the curve the current call is on (CustomScope)
  template <class CV>
  int comb_idx() const { return CV::RT_ORDER ? custom_curve_ : CV::ID; }
  template <class CV>
  const typename Work<CV>::A* comb_of() const { return (const typename Work<CV>::A*)comb_[comb_idx<CV>()]; }
  // bk.launch of Fn<CV>{n, a...} on n threads -- for a p521 batch with a second wave to pair
  // (ELL_P521_PAIR_MIN), of the instantiation held to 256 registers, Fn<CV, 2>
  template <template <class, auto...> class Fn, class CV, class... A>
  void launch_paired(size_t n, A... a) {
    if (Work<CV>::L > 12 && n > ELL_P521_PAIR_MIN) {
      Fn<CV, (Work<CV>::L > 12 ? 2 : 0)> f{n, a...};
      bk.launch(f, n);
    } else {
      Fn<CV> f{n, a...};
      bk.launch(f, n);
    }
  }
  // the parts of a parted Point#mul (secp256k1) in the kernel of `form`: the two halves of k * P
  // and, for k * P + kg * G (kg != null), the comb of kg
  template <class CV>
  void launch_mul_parts(Form form, size_t n, const u8* k, const u8* xy, typename Work<CV>::VT* tbl, u32* jac,
                        const u8* kg) {
    const typename Work<CV>::A* comb = kg ? comb_of<CV>() : nullptr;
    const size_t units = part_units(form, n, kg ? 3 : 2);
    if (form == Form::PARTS_WAVE) {           // two or three WAVES per item (coop.h)
      FnMulPartsK256<false> f{n, k, xy, jac, kg, comb};
      bk.launch_coop(f, units);
    } else if (form == Form::PARTS_ROW) {     // one ROW per item and part: four items per wave
      FnMulPartsK256<true> f{n, k, xy, jac, kg, comb};
      bk.launch_coop(f, units);
    } else {                                  // two or three lanes per item
      FnMulParts<CV> f{n, part_pad(n), k, xy, tbl, jac, kg, comb};
      launch_fn(f, units);
    }
  }
  // Brackets one call on a user-defined curve: takes the device's custom-curve lock, uploads the
  // curve's parameter block (synchronously: every earlier user of the block has finished, see the
  // destructor) and, at the end, waits for the call's device work before the lock is released.
  // Nested uses (a composed operation -- ecdsa_verify_wire, custom_verify_wire -- calls the
  // operations it is made of on scratch, with Mem::device, from inside its own scope) are no-ops.
  struct CustomScope {
    Engine* e;
    bool owner = false;
    int rc = E_OK;
    // mont: the call is one of the Montgomery entry points (custom_mont_*); every other call
    // refuses a Montgomery id here, before anything is uploaded.  ed_key: the call is one of the
    // Edwards key-side entry points (custom_ed_*), which run on the curve's augmented block.
    CustomScope(Engine* eng, int curve, bool mont = false, bool ed_key = false) : e(eng) {
      if (!is_custom(curve) || e->custom_active_) return;
      size_t slot = (size_t)(curve - CURVE_CUSTOM0);
      if (slot >= e->custom_.size()) { rc = e->fail(E_ARG, "unknown curve id"); return; }
      if (!mont && e->custom_[slot].kind == 2) {
        rc = e->fail(E_UNSUPPORTED, "not available on user-defined Montgomery curves (x-only: ellgpu_custom_mont_ladder, _validate, _derive)");
        return;
      }
      custom_mutex(e->bk.device_index()).lock();
      owner = true;
      e->custom_active_ = true;
      e->custom_curve_ = curve;
      e->bk.rt_upload(ed_key ? e->custom_aug_[slot] : e->custom_[slot]);
    }
    ~CustomScope() {
      if (!owner) return;
      e->bk.sync();
      e->custom_active_ = false;
      custom_mutex(e->bk.device_index()).unlock();
    }
  };

  int prepare_curve(int curve) {
#if defined(ELL_ONLY_CURVE)
    if (curve < CURVE_ED25519 && curve != ELL_ONLY_CURVE) return fail(E_UNSUPPORTED, "developer build: single curve only");
#endif
    if (curve == CURVE_ED25519) return ensure_ed_comb();
    if (curve == CURVE_CURVE25519) return E_OK;
    int rc = E_OK;
    ELL_SHORT_DISPATCH(curve, rc = ensure_comb<CV>());
    return rc;
  }
  // f(o, m) on the items [o, o + m) of [0, n), at most `step` per launch; stops at the first error
  template <class F>
  static int for_chunks(size_t n, size_t step, F f) {
    for (size_t o = 0; o < n; o += step) {
      const int rc = f(o, n - o < step ? n - o : step);
      if (rc) return rc;
    }
    return E_OK;
  }
  // _truncateToN (ec/index.js:97-102): the right shift that brings a hash of msg_bits bits (0: all
  // hash_len bytes) to the bit length of an order of order_bits bits held in ln 32-bit words
  int truncate_shift(int hash_len, int msg_bits, int order_bits, int ln, int& shift) {
    if (hash_len <= 0 || msg_bits < 0) return fail(E_ARG, "bad hash_len / msg_bits");
    shift = (msg_bits ? msg_bits : hash_len * 8) - order_bits;
    if (shift < 0) shift = 0;
    if (hash_len * 8 - shift > 32 * ln || hash_len - (shift >> 3) > 4 * (ln + 1))
      return fail(E_ARG, "hash_len / msg_bits combination leaves more bits than the order width");
    return E_OK;
  }

  // ---- the operands of a batch call, wherever they live -----------------------
  // An operand: n items of `stride` bytes.  A null pointer is an absent optional operand (the
  // operations have refused the required ones): the body sees nullptr in its place, and a host
  // call gives it no device copy.
  struct In { const void* ptr; size_t stride; bool opt = false; };   // opt: see staged_whole()
  struct Out { void* ptr; size_t stride; };
  static constexpr int STAGED_MAX = 4;        // operands each way (pipelined(), small_call())
  // gives every present operand a staging buffer of its own, inputs and outputs in order
  template <int NI, int NO>
  int stage(size_t n, const In (&in)[NI], const Out (&out)[NO], u8* (&d)[NI], u8* (&r)[NO]) {
    static_assert(NI <= STAGED_MAX && NO <= STAGED_MAX, "too many operands");
    auto slot = [&](int i, const void* host, size_t bytes) {
      return host ? (u8*)grow(staging_[i], bytes ? bytes : 1) : nullptr;
    };
    bool ok = true;
    for (int i = 0; i < NI; i++) ok &= (d[i] = slot(i, in[i].ptr, n * in[i].stride)) || !in[i].ptr;
    for (int i = 0; i < NO; i++) ok &= (r[i] = slot(STAGED_MAX + i, out[i].ptr, n * out[i].stride)) || !out[i].ptr;
    return ok ? E_OK : nomem();
  }
  int nomem() { return fail(E_NOMEM, "staging allocation failed"); }
  // One batch call: body(m, d, r) on at most CHUNK items at a time, where d / r are DEVICE pointers
  // to the inputs / outputs, already offset to the first of the m items -- the only place that
  // does operand pointer arithmetic.  Mem::device: the caller's pointers, chunk by chunk.
  // Mem::host: the operands are staged and the body runs inside each step of pipelined(), on that
  // step's lane, over the device copies.
  template <int NI, int NO, class Body>
  int batch(Mem where, size_t n, const In (&in)[NI], const Out (&out)[NO], Body body) {
    u8* d[NI];
    u8* r[NO];
    auto chunks = [&](size_t first, size_t count) {
      return for_chunks(count, CHUNK, [&](size_t o, size_t m) {
        const u8* di[NI];
        u8* ro[NO];
        for (int i = 0; i < NI; i++) di[i] = d[i] ? d[i] + (first + o) * in[i].stride : nullptr;
        for (int i = 0; i < NO; i++) ro[i] = r[i] ? r[i] + (first + o) * out[i].stride : nullptr;
        return body(m, di, ro);
      });
    };
    if (where == Mem::device) {
      for (int i = 0; i < NI; i++) d[i] = (u8*)in[i].ptr;
      for (int i = 0; i < NO; i++) r[i] = (u8*)out[i].ptr;
      return chunks(0, n);
    }
    if (int rc = stage(n, in, out, d, r)) return rc;
    HostIn hi[NI];
    HostOut ho[NO];
    int ni = 0, no = 0;
    for (int i = 0; i < NI; i++) if (d[i]) hi[ni++] = {d[i], (const u8*)in[i].ptr, in[i].stride};
    for (int i = 0; i < NO; i++) if (r[i]) ho[no++] = {(u8*)out[i].ptr, r[i], out[i].stride};
    return pipelined(n, hi, ni, ho, no, chunks);
  }
  // The EdDSA calls: their operands are whole buffers (`stride` = all their bytes), since the
  // message offsets index the whole message buffer.  So no pipelining: a few items go through
  // small_call(), more are copied in, run as one batch and copied out.  On that path only an
  // optional input may be absent: a null one that is required (possible at n = 0 only, the
  // operations refuse it sooner) fails as an allocation.
  template <int NI, int NO, class Body>
  int staged_whole(size_t n, const In (&in)[NI], const Out (&out)[NO], Body body) {
    u8* d[NI];
    u8* r[NO];
    if (int rc = stage(1, in, out, d, r)) return rc;
    if (n && n <= bk.pipeline_quantum()) {
      SpanIn si[NI];
      SpanOut so[NO];
      for (int i = 0; i < NI; i++) si[i] = {d[i], (const u8*)in[i].ptr, in[i].stride};
      for (int i = 0; i < NO; i++) so[i] = {(u8*)out[i].ptr, r[i], out[i].stride};
      int rc = E_OK;
      if (small_call(si, NI, so, NO, [&]() { return body(d, r); }, &rc)) return rc;
    }
    defer_skip();
    for (int i = 0; i < NI; i++) {
      if (!in[i].ptr && !in[i].opt) return nomem();
      if (in[i].ptr && in[i].stride) bk.h2d(d[i], in[i].ptr, in[i].stride);
    }
    const int rc = body(d, r);
    if (rc) return rc;
    for (int i = 0; i < NO; i++)
      if (r[i]) bk.d2h(out[i].ptr, r[i], out[i].stride);
    return bk.sync();
  }

  // Host-buffer calls are software-pipelined: the batch is cut into chunks that alternate
  // between two compute lanes (stream + scratch arena each), so chunk c+1's wavefronts fill
  // the SIMDs as chunk c's drain (a lone chunk pays ~1 ms of ramp-down at 1 wave round), and
  // chunk c+1's H2D / chunk c-1's D2H run on the copy stream while chunk c computes.  The
  // first chunk is one residency quantum so that compute starts early.  body(o, m) launches
  // items [o, o+m) on the current lane.
  struct HostIn { u8* dev; const u8* host; size_t stride; };
  struct HostOut { u8* host; const u8* dev; size_t stride; };
  // A batch of a few items -- one patched EC#verify, Point#mul or EC#sign -- has nothing to
  // pipeline: its inputs and results travel through ONE pinned host buffer, on the context's own
  // stream, with one synchronisation (no copy streams, no events, no pageable-memory copies that
  // each block the host: 60 -> ~25 us of overhead per call).
  static constexpr size_t SMALL_HOST_BYTES = 256 * 1024;
  // The SPLIT form of such a call (ellgpu_ctx_defer / ellgpu_ctx_collect): an armed context's next
  // small call returns as soon as its copies and kernels are enqueued; the synchronisation and the
  // copy into the caller's result buffers happen in defer_collect().  The host thread is free in
  // between -- the JavaScript layer re-validates what it took on trust (the reference's
  // precomputed tables, elliptic_amd/js/index.js) while the device works.  Anything else that
  // enters the context first completes the pending call (capi_common.h ELL_LOCK).
  struct Deferred {
    bool armed = false, on = false;
    std::thread::id owner;         // the thread that armed: only ITS next call is deferred (a libuv worker's
                                   // batch that slips in between must run to completion as usual)
    struct Out { u8* host; size_t bytes; } outs[4];
    int nout = 0;
    size_t out0 = 0;
    u8* pin = nullptr;
  } defer_;
  void defer_arm() { defer_.armed = true; defer_.owner = std::this_thread::get_id(); }
  bool defer_pending() const { return defer_.on; }
  // is the next small call of THIS thread to be deferred?  (consumes the arming if so)
  bool defer_take() {
    if (!defer_.armed || defer_.owner != std::this_thread::get_id()) return false;
    defer_skip();
    return true;
  }
  // a call of the arming thread that cannot be deferred disarms; another thread's call leaves it armed
  void defer_skip() {
    if (defer_.armed && defer_.owner == std::this_thread::get_id()) defer_.armed = false;
  }
  static size_t pad64(size_t b) { return (b + 63) & ~(size_t)63; }
  int defer_collect() {
    defer_skip();
    if (!defer_.on) return E_OK;
    defer_.on = false;
    bk.select_lane(0);
    const int rs = bk.sync();
    size_t off = defer_.out0;
    for (int i = 0; i < defer_.nout; i++)
      if (defer_.outs[i].host) {
        if (!rs) memcpy(defer_.outs[i].host, defer_.pin + off, defer_.outs[i].bytes);
        off += pad64(defer_.outs[i].bytes);
      }
    if (rs) fail(rs, "device error in a deferred call");
    return rs;
  }
  // the few-item call itself: operands (host -> pinned -> device), body, results (device -> pinned
  // [-> host, now or in defer_collect]).  Returns false when the call does not fit the pinned buffer.
  struct SpanIn { u8* dev; const u8* host; size_t bytes; };
  struct SpanOut { u8* host; const u8* dev; size_t bytes; };
  template <class Body>
  bool small_call(const SpanIn* ins, int nin, const SpanOut* outs, int nout, Body body, int* result) {
    size_t tot = 0;
    for (int i = 0; i < nin; i++) if (ins[i].host) tot += pad64(ins[i].bytes);
    for (int i = 0; i < nout; i++) if (outs[i].host) tot += pad64(outs[i].bytes);
    u8* pin = tot <= SMALL_HOST_BYTES ? (u8*)bk.pinned(SMALL_HOST_BYTES) : nullptr;
    if (!pin) return false;
    const bool defer = defer_take();
    size_t off = 0;
    for (int i = 0; i < nin; i++)
      if (ins[i].host) {
        memcpy(pin + off, ins[i].host, ins[i].bytes);
        if (ins[i].bytes) bk.h2d(ins[i].dev, pin + off, ins[i].bytes);
        off += pad64(ins[i].bytes);
      }
    lane_ = 0;
    const int rc = body();
    const size_t out0 = off;
    for (int i = 0; i < nout; i++)
      if (outs[i].host) {
        if (outs[i].bytes) bk.d2h(pin + off, outs[i].dev, outs[i].bytes);
        off += pad64(outs[i].bytes);
      }
    if (defer && !rc && nout <= 4 && !custom_active_) {
      defer_.on = true;
      defer_.nout = nout;
      for (int i = 0; i < nout; i++) defer_.outs[i] = {outs[i].host, outs[i].bytes};
      defer_.out0 = out0;
      defer_.pin = pin;
      *result = E_OK;
      return true;
    }
    const int rs = bk.sync();
    off = out0;
    for (int i = 0; i < nout; i++)
      if (outs[i].host) {
        if (!rc && !rs) memcpy(outs[i].host, pin + off, outs[i].bytes);
        off += pad64(outs[i].bytes);
      }
    *result = rc ? rc : rs;
    return true;
  }
  template <class Body>
  int pipelined(size_t n, const HostIn* ins, int nin, const HostOut* outs, int nout, Body body) {
    if (n && n <= bk.pipeline_quantum() && nin <= 4 && nout <= 4) {
      SpanIn si[4];
      SpanOut so[4];
      for (int i = 0; i < nin; i++) si[i] = {ins[i].dev, ins[i].host, n * ins[i].stride};
      for (int i = 0; i < nout; i++) so[i] = {outs[i].host, outs[i].dev, n * outs[i].stride};
      int rc = E_OK;
      if (small_call(si, nin, so, nout, [&]() { return body(0, n); }, &rc)) return rc;
    }
    defer_skip();
    size_t q = bk.pipeline_quantum(), step = q;
    size_t o = 0, po = 0, pm = 0;
    int pev = -1, rc = E_OK;
    for (int c = 0; o < n && !rc; c++) {
      size_t m = n - o;
      if (m > step + step / 2) m = step;          // a short tail is absorbed by the last chunk
      for (int i = 0; i < nin; i++)
        if (ins[i].host)
          bk.h2d_copy(ins[i].dev + o * ins[i].stride, ins[i].host + o * ins[i].stride, m * ins[i].stride);
      lane_ = c & 1;
      bk.select_lane(lane_);
      bk.copies_before_compute();
      rc = body(o, m);
      int ev = bk.mark_compute();
      if (pev >= 0) {
        bk.copy_after(pev);
        for (int i = 0; i < nout; i++)
          bk.d2h_copy(outs[i].host + po * outs[i].stride, outs[i].dev + po * outs[i].stride, pm * outs[i].stride);
      }
      pev = ev; po = o; pm = m;
      o += m;
      step = pipe_step_ * q;                      // measured: every chunk boundary costs ~0.4 ms
    }
    if (pev >= 0 && !rc) {
      bk.copy_after(pev);
      for (int i = 0; i < nout; i++)
        bk.d2h_copy(outs[i].host + po * outs[i].stride, outs[i].dev + po * outs[i].stride, pm * outs[i].stride);
    }
    lane_ = 0;
    bk.select_lane(0);
    int rs = bk.sync_lanes();
    return rc ? rc : rs;
  }

  // ---- the operations: one function each, `where` says where the operands live ------------------
  // Every operation is: its checks, its CustomScope, batch().  What the two forms refuse is the
  // same; the ORDER in which the preset operations refuse is each form's own, and both are pinned
  // (tests/test_hostsim_forms.py, tests/test_entry_forms_hostsim.py).  A host call answers first
  // for what staging reads -- a null buffer, a hash_len that is no stride (host_first) -- and
  // only a batch with items asks what its curve and its lengths allow; a device call asks the
  // curve first, whatever n is (asks_curve).
  int host_first(Mem where, bool nul, int hash_len = 1) {
    if (where != Mem::host) return E_OK;
    if (nul) return fail(E_ARG, "null pointer");
    if (hash_len <= 0) return fail(E_ARG, "bad hash_len");
    return E_OK;
  }
  static bool asks_curve(Mem where, size_t n) { return where == Mem::device || n; }

  int mul_fixed(Mem where, int curve, size_t n, const u8* k, u8* out_xy, u8* out_inf) {
    const CurveInfo* ci = curve_info(curve);
    if (!ci) return fail(E_ARG, "unknown curve id");
    const bool nul = n && (!k || !out_xy || !out_inf);
    if (int rc = host_first(where, nul)) return rc;
    if (asks_curve(where, n)) {
      if (curve == CURVE_CURVE25519)
        return fail(E_UNSUPPORTED, "curve25519 has no affine fixed-base form; use x25519_ladder");
      if (nul) return fail(E_ARG, "null pointer");
    }
    // (a host call opens the scope of any user-defined id, and so names an unknown or a Montgomery
    // one as such before its first step finds no table; a device call opens a domain's only and
    // refuses every other one here, empty batch or not)
    const bool dom = custom_is_domain(curve);
    if (where == Mem::device && is_custom(curve) && !dom) return prepare_curve(curve);
    CustomScope sc(this, dom || where == Mem::host ? curve : -1);
    if (sc.rc) return sc.rc;
    const size_t B = ci->field_bytes;
    return batch(where, n, {In{k, B}}, {Out{out_xy, 2 * B}, Out{out_inf, 1}}, [&](size_t m, auto d, auto r) {
      int rc = dom ? ensure_comb<CvCustomDomain>() : prepare_curve(curve);
      if (rc) return rc;
      if (dom) rc = mul_fixed_chunk<CvCustomDomain>(m, d[0], comb_of<CvCustomDomain>(), nullptr, nullptr, r[0], r[1]);
      else if (curve == CURVE_ED25519) rc = ed_mul_fixed_chunk(m, d[0], r[0], r[1]);
      else ELL_SHORT_DISPATCH(curve, rc = mul_fixed_chunk<CV>(m, d[0], comb_of<CV>(), nullptr, nullptr, r[0], r[1]));
      return rc;
    });
  }

  static bool overlap(const u8* a, const u8* b, size_t bytes) {
    return a && b && bytes && (uintptr_t)a < (uintptr_t)b + bytes && (uintptr_t)b < (uintptr_t)a + bytes;
  }
  // ... of two ranges with sizes of their own
  static bool overlap2(const u8* a, size_t na, const u8* b, size_t nb) {
    return a && b && na && nb && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
  }
  int mul_var(Mem where, int curve, size_t n, const u8* k, const u8* xy, u8* out_xy, u8* out_inf) {
    const CurveInfo* ci = curve_info(curve);
    if (!ci) return fail(E_ARG, "unknown curve id");
    const bool nul = n && (!k || !xy || !out_xy || !out_inf);
    if (int rc = host_first(where, nul)) return rc;
    const size_t B = ci->field_bytes;
    if (asks_curve(where, n)) {
      if (curve == CURVE_CURVE25519)
        return fail(E_UNSUPPORTED, "curve25519 is x-only; use x25519_ladder");
      if (nul) return fail(E_ARG, "null pointer");
      // the operands are read again AFTER the results are written (the curve test of
      // Work::domain_mark / mul_join): a result written over its own operand would be tested in its
      // place.  Device pointers only: a host caller's operand and result never share a staging buffer.
      if (where == Mem::device && overlap(xy, out_xy, n * 2 * B)) return fail(E_ARG, "in_xy and out_xy must not overlap");
    }
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{k, B}, In{xy, 2 * B}}, {Out{out_xy, 2 * B}, Out{out_inf, 1}}, [&](size_t m, auto d, auto r) {
      int rc = E_OK;
      if (custom_is_edwards(curve)) rc = edc_chunk(0, m, d[0], d[1], nullptr, nullptr, nullptr, nullptr, r[0], r[1]);
      else if (is_custom(curve)) rc = mul_var_chunk<CvCustom>(m, d[0], d[1], r[0], r[1], nullptr);
      else if (curve == CURVE_ED25519) rc = ed_mul_var_chunk(m, d[0], d[1], r[0], r[1], nullptr);
      else ELL_SHORT_DISPATCH(curve, rc = mul_var_chunk<CV>(m, d[0], d[1], r[0], r[1], nullptr));
      return rc;
    });
  }

  // xy1 == null: k1 * G + k2 * P2 over the curve's fixed-base table
  int mul_add2(Mem where, int curve, size_t n, const u8* k1, const u8* xy1, const u8* k2, const u8* xy2,
               u8* out_xy, u8* out_inf) {
    const CurveInfo* ci = curve_info(curve);
    if (!ci) return fail(E_ARG, "unknown curve id");
    const bool nul = n && (!k1 || !k2 || !xy2 || !out_xy || !out_inf);
    if (int rc = host_first(where, nul)) return rc;
    const size_t B = ci->field_bytes;
    const bool dom = custom_is_domain(curve);
    // (a device call says so before it opens the curve's scope, a host call with items after)
    const bool no_table = is_custom(curve) && !xy1 && !dom;
    const char* const no_table_msg = "user-defined curves without a generator have no fixed-base table: pass the generator as p1";
    if (asks_curve(where, n)) {
      if (curve == CURVE_CURVE25519)
        return fail(E_UNSUPPORTED, "Not supported on Montgomery curve");     // mont.js:155-157
      if (nul) return fail(E_ARG, "null pointer");
      if (where == Mem::device) {
        if (no_table) return fail(E_UNSUPPORTED, no_table_msg);
        if (overlap(xy2, out_xy, n * 2 * B) || overlap(xy1, out_xy, n * 2 * B))   // see mul_var
          return fail(E_ARG, "p1_xy / p2_xy and out_xy must not overlap");
      }
    }
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    if (no_table && n) return fail(E_UNSUPPORTED, no_table_msg);
    return batch(where, n, {In{k1, B}, In{xy1, 2 * B}, In{k2, B}, In{xy2, 2 * B}}, {Out{out_xy, 2 * B}, Out{out_inf, 1}},
                 [&](size_t m, auto d, auto r) {
      int rc = E_OK;
      if (!d[1]) {
        rc = dom ? ensure_comb<CvCustomDomain>() : prepare_curve(curve);
        if (rc) return rc;
      }
      if (custom_is_edwards(curve)) rc = edc_chunk(1, m, d[0], d[1], d[2], d[3], nullptr, nullptr, r[0], r[1]);
      else if (is_custom(curve) && !d[1]) rc = mul_add_g_chunk<CvCustomDomain>(m, d[0], d[2], d[3], r[0], r[1]);
      else if (is_custom(curve)) rc = mul_add2_chunk<CvCustom>(m, d[0], d[1], d[2], d[3], r[0], r[1]);
      else if (curve == CURVE_ED25519) rc = ed_mul_add2_chunk(m, d[0], d[1], d[2], d[3], r[0], r[1]);
      else ELL_SHORT_DISPATCH(curve, rc = d[1] ? mul_add2_chunk<CV>(m, d[0], d[1], d[2], d[3], r[0], r[1])
                                               : mul_add_g_chunk<CV>(m, d[0], d[2], d[3], r[0], r[1]));
      return rc;
    });
  }

  // ---- fixed-base tables of caller-chosen points: BasePoint#precompute on the device ----------
  // define_base builds the comb of a point the caller uses repeatedly (a Pedersen H, a recipient's
  // or a verifier's key, a static ECDH key); mul_base is then mul_fixed over that table and
  // mul_base2 walks two tables into one accumulator.  Short curves only: the six presets and
  // user-defined short ids, plain and domain.
  //   xy == null      the curve's own generator: the handle ALIASES the curve's table (built at
  //                   first use by ensure_comb; release does not free it)
  //   window_bits     signed combs (Work::COMB_SIGNED): 0, 4, 8, 12, 16 or 22, 0 = 16 (or G's own
  //                   width where that is narrower: the CPU unit-test build), narrowed on E_NOMEM
  //                   as ensure_comb narrows; an explicit width that does not fit is E_NOMEM.
  //                   Unsigned combs: 0 or 8.
  // Order of the base.  On a preset every curve point has the prime order n, so the entries
  // ((d << sh) mod n) * P are exact and never O.  On a user-defined id nothing is reduced and the
  // base may have a small order: an entry that is O (stored as (0, 0), which the walks would add
  // as a point) refuses the base.
  // The same (curve, point, width in use) gives the same handle; handles are never reused.
  static constexpr int BASE_MAX = 16;
  struct BaseRec {
    int handle, curve, asked;
    bool alias;
    bool ed = false;           // an Edwards handle (define_ed_base): ed25519 or a user-defined Edwards id
    CombTable t;
    u8 xy[2 * 66];
  };
  BaseRec* base_rec(int handle) {
    for (auto& r : bases_)
      if (r.handle == handle) return &r;
    fail(E_ARG, "unknown base handle");
    return nullptr;
  }
  // is the curve's comb a signed one (E_OK), with the refusals of define_base for the others
  int base_curve_kind(int curve, bool& sgn) {
    if (!curve_info(curve)) return fail(E_ARG, "unknown curve id");
    if (curve == CURVE_ED25519 || curve == CURVE_CURVE25519)
      return fail(E_UNSUPPORTED, "fixed-base tables of caller-chosen points are implemented for short Weierstrass curves");
    sgn = false;
    if (is_custom(curve)) {
      size_t slot = (size_t)(curve - CURVE_CUSTOM0);
      if (slot >= custom_.size()) return fail(E_ARG, "unknown curve id");
      if (custom_[slot].kind != 0)
        return fail(E_UNSUPPORTED, "fixed-base tables of caller-chosen points are implemented for short Weierstrass curves");
      return E_OK;
    }
    ELL_SHORT_DISPATCH(curve, sgn = Work<CV>::COMB_SIGNED);
    return E_OK;
  }
  // ... and of define_ed_base: ed25519 and user-defined Edwards ids, plain and domain
  int ed_base_curve_kind(int curve) {
    if (!curve_info(curve)) return fail(E_ARG, "unknown curve id");
    if (curve == CURVE_ED25519) return E_OK;
    if (curve == CURVE_CURVE25519) return fail(E_UNSUPPORTED, "curve25519 is x-only: it has no fixed-base tables");
    const char* const shorts = "a short Weierstrass curve: its fixed-base tables are ellgpu_base_define's";
    if (!is_custom(curve)) return fail(E_UNSUPPORTED, shorts);
    size_t slot = (size_t)(curve - CURVE_CUSTOM0);
    if (slot >= custom_.size()) return fail(E_ARG, "unknown curve id");
    if (custom_[slot].kind == 0) return fail(E_UNSUPPORTED, shorts);
    if (custom_[slot].kind != 1) return fail(E_UNSUPPORTED, "user-defined Montgomery curves are x-only: they have no fixed-base tables");
    return E_OK;
  }
  // The kernels of a base on a user-defined id are the domain's (CvCustomDomain: the comb walks
  // read the field alone), so a PLAIN id's block goes to their code object as well: the backend
  // uploads it there for a block marked as a domain, and no kernel reads that mark.
  void base_upload(int curve) {
    if (!is_custom(curve) || custom_is_domain(curve)) return;
    RtField f = custom_[(size_t)(curve - CURVE_CUSTOM0)];
    f.domain = 1;
    bk.rt_upload(f);
  }
  // ed: the call is define_ed_base (ellgpu_ed_base_define): ed25519 and user-defined Edwards ids,
  // which this entry point refuses otherwise.  There the identity and points of small order are
  // ordinary table entries of a unified law (no refusal), scalars are 32 bytes as they stand, and
  //   xy == null      ed25519: an alias of the curve's own table; an Edwards domain: a table of the
  //                   domain's G that the handle owns, as if G's coordinates had been passed
  //   window_bits     ed25519: 0 or EdWork::COMB_BITS (EdWork's cached format, comb_mul as it stands);
  //                   user-defined: 0 (= 8), 8 or 16 -- 256 / bits windows x (2^bits - 1) affine
  //                   entries of 64 bytes, the width in the header slot (EdcWork::comb_add)
  int define_base(int curve, const u8* xy, int window_bits, int* out_base, bool* created = nullptr, bool ed = false) {
    if (created) *created = false;
    if (!out_base) return fail(E_ARG, "null pointer");
    bool sgn = false;
    if (int rc = ed ? ed_base_curve_kind(curve) : base_curve_kind(curve, sgn)) return rc;
    const bool dom = ed ? is_custom(curve) && custom_[(size_t)(curve - CURVE_CUSTOM0)].domain == 1 : custom_is_domain(curve);
    const size_t B = (size_t)curve_info(curve)->field_bytes;
    u8 gxy[64];
    if (!xy) {
      if (is_custom(curve) && !dom) return fail(E_ARG, "a user-defined curve without a domain has no generator: pass the base's coordinates");
      if (window_bits) return fail(E_ARG, "the curve's own generator comes with its own table: window_bits must be 0");
      if (ed && dom) {
        const RtField& f = custom_[(size_t)(curve - CURVE_CUSTOM0)];
        store_be<8>(gxy, f.gx, 32);
        store_be<8>(gxy + 32, f.gy, 32);
        xy = gxy;
      }
    } else if (ed) {
      if (curve == CURVE_ED25519 ? !(window_bits == 0 || window_bits == EdWork::COMB_BITS)
                                 : !(window_bits == 0 || window_bits == 8 || window_bits == 16))
        return fail(E_ARG, curve == CURVE_ED25519 ? "window_bits on ed25519: 0 or the width of the curve's own comb"
                                                  : "window_bits on a user-defined Edwards curve: 0, 8 or 16");
    } else if (sgn ? !(window_bits == 0 || window_bits == 4 || window_bits == 8 || window_bits == 12 ||
                       window_bits == 16 || window_bits == 22)
                   : !(window_bits == 0 || window_bits == 8)) {
      return fail(E_ARG, sgn ? "window_bits of a signed comb: 0, 4, 8, 12, 16 or 22" : "window_bits of an unsigned comb: 0 or 8");
    }
    auto same = [&](const BaseRec& r, int bits) {
      if (r.curve != curve || r.alias != !xy) return false;
      return r.alias || (memcmp(r.xy, xy, 2 * B) == 0 && (bits ? r.t.bits == bits : r.asked == 0));
    };
    for (auto& r : bases_)
      if (same(r, window_bits)) { *out_base = r.handle; return E_OK; }
    if ((int)bases_.size() >= BASE_MAX) return fail(E_UNSUPPORTED, "at most 16 live bases per context");
    BaseRec rec;
    rec.curve = curve;
    rec.asked = window_bits;
    rec.alias = !xy;
    rec.ed = ed;
    memset(rec.xy, 0, sizeof rec.xy);
    if (xy) {
      memcpy(rec.xy, xy, 2 * B);
      CustomScope sc(this, curve);
      if (sc.rc) return sc.rc;
      if (!ed) base_upload(curve);
      int rc = E_OK;
      if (ed) rc = curve == CURVE_ED25519 ? ed_base_table(xy, false, rec.t) : edc_base_table(xy, window_bits, rec.t);
      else if (is_custom(curve)) rc = base_table<CvCustomDomain>(xy, window_bits, rec.t);
      else ELL_SHORT_DISPATCH(curve, rc = base_table<CV>(xy, window_bits, rec.t));
      if (rc) return rc;
      // (a default width that narrowed may have arrived at a table that exists)
      for (auto& r : bases_)
        if (same(r, rec.t.bits)) {
          bk.free_(rec.t.base);
          *out_base = r.handle;
          return E_OK;
        }
    }
    rec.handle = next_base_++;
    bases_.push_back(rec);
    *out_base = rec.handle;
    if (created) *created = true;
    return E_OK;
  }
  // unissued: the handle never reached the caller (a group's define that another member refused
  // takes it back, capi_common.h) -- the newest handle is then free again, so that the members'
  // counters stay in step
  int release_base(int handle, bool unissued = false) {
    for (size_t i = 0; i < bases_.size(); i++)
      if (bases_[i].handle == handle) {
        if (unissued && handle == next_base_ - 1) next_base_--;
        if (!bases_[i].alias) {
          bk.sync_all();                          // a call on a caller's stream may still be walking the table
          bk.free_(bases_[i].t.base);
        }
        bases_.erase(bases_.begin() + (long)i);
        return E_OK;
      }
    return fail(E_ARG, "unknown base handle");
  }
  // an alias whose curve has not built its table yet reports 0 bits and 0 bytes
  int base_info(int handle, int* out_curve, int* out_bits, u64* out_bytes) {
    BaseRec* r = base_rec(handle);
    if (!r) return E_ARG;
    int bits = r->t.bits;
    size_t bytes = r->t.bytes;
    if (r->alias && r->ed) {
      bits = comb_[CURVE_ED25519] ? EdWork::COMB_BITS : 0;
      bytes = bits ? EdWork::COMB_ENTRIES * sizeof(EdWork::P) : 0;
    } else if (r->alias) {
      bits = comb_[r->curve] ? (comb_bits_[r->curve] ? comb_bits_[r->curve] : 8) : 0;
      bytes = 0;
      if (bits) {
        if (is_custom(r->curve)) bytes = comb_bytes<CvCustomDomain>(bits);
        else ELL_SHORT_DISPATCH(r->curve, bytes = comb_bytes<CV>(bits));
      }
    }
    if (out_curve) *out_curve = r->curve;
    if (out_bits) *out_bits = bits;
    if (out_bytes) *out_bytes = (u64)bytes;
    return E_OK;
  }
  // entries (and bytes, with the header slot) of curve type CV's comb at window width cb
  template <class CV>
  static size_t comb_entries(int cb) {
    typedef Work<CV> W;
    return W::COMB_SIGNED ? (size_t)comb_windows(8 * W::BYTES, cb) << (cb - 1) : W::COMB_ENTRIES;
  }
  template <class CV>
  static size_t comb_bytes(int cb) { return (comb_entries<CV>(cb) + 1) * sizeof(typename Work<CV>::A); }
  // the table a base stands for, for the call in progress (an alias: the curve's own, built here
  // on first use)
  int base_table_ptr(const BaseRec& r, const void*& comb) {
    if (!r.alias) { comb = r.t.comb; return E_OK; }
    if (r.ed) {                                    // ed25519's own table
      const int rc = ensure_ed_comb();
      comb = comb_[CURVE_ED25519];
      return rc;
    }
    const int rc = custom_is_domain(r.curve) ? ensure_comb<CvCustomDomain>() : prepare_curve(r.curve);
    comb = comb_[r.curve];
    return rc;
  }
  // One chunk of k1 * B1 (r2 and k2 null) or k1 * B1 + k2 * B2 over the tables of one curve, on the
  // curve's family: ed25519, a user-defined Edwards id, a user-defined short id, a preset
  int walk_tables(const BaseRec& r1, const BaseRec* r2, size_t m, const u8* k1, const u8* k2, u8* out_xy, u8* out_inf) {
    const void* t1 = nullptr;
    const void* t2 = nullptr;
    int rc = base_table_ptr(r1, t1);
    if (rc == E_OK && r2) rc = base_table_ptr(*r2, t2);
    if (rc) return rc;
    const int curve = r1.curve;
    if (r1.ed) return curve == CURVE_ED25519
                          ? ed_base_mul_chunk(m, k1, (const EdWork::P*)t1, k2, (const EdWork::P*)t2, out_xy, out_inf)
                          : edc_base_mul_chunk(m, k1, (const EdcWork::A*)t1, k2, (const EdcWork::A*)t2, out_xy, out_inf);
    if (is_custom(curve)) {
      typedef const Work<CvCustomDomain>::A* T;
      return mul_fixed_chunk<CvCustomDomain>(m, k1, (T)t1, k2, (T)t2, out_xy, out_inf);
    }
    ELL_SHORT_DISPATCH(curve, rc = mul_fixed_chunk<CV>(m, k1, (const typename Work<CV>::A*)t1, k2,
                                                        (const typename Work<CV>::A*)t2, out_xy, out_inf));
    return rc;
  }
  // P.precompute(); P.mul(k): k as it stands (field_bytes bytes, neither reduced nor truncated, as
  // in mul_fixed), out_inf = 1 and a zeroed result at O.  No status 2: the base was tested when defined.
  int mul_base(Mem where, int base, size_t n, const u8* k, u8* out_xy, u8* out_inf) {
    const BaseRec* r = base_rec(base);
    if (!r) return E_ARG;
    if (n && (!k || !out_xy || !out_inf)) return fail(E_ARG, "null pointer");
    const int curve = r->curve;
    const size_t B = (size_t)curve_info(curve)->field_bytes;
    if (where == Mem::device && (overlap2(k, n * B, out_xy, n * 2 * B) || overlap2(k, n * B, out_inf, n)))
      return fail(E_ARG, "k and the results must not overlap");
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    if (!r->ed) base_upload(curve);
    return batch(where, n, {In{k, B}}, {Out{out_xy, 2 * B}, Out{out_inf, 1}}, [&](size_t m, auto d, auto o) {
      return walk_tables(*r, nullptr, m, d[0], nullptr, o[0], o[1]);
    });
  }
  // k1 * B1 + k2 * B2 (_wnafMulAdd on two precomputed operands); base1 == base2 is allowed
  int mul_base2(Mem where, int base1, int base2, size_t n, const u8* k1, const u8* k2, u8* out_xy, u8* out_inf) {
    const BaseRec* r1 = base_rec(base1);
    const BaseRec* r2 = r1 ? base_rec(base2) : nullptr;
    if (!r1 || !r2) return E_ARG;
    if (r1->curve != r2->curve || r1->ed != r2->ed) return fail(E_ARG, "the two bases are on different curves");
    if (n && (!k1 || !k2 || !out_xy || !out_inf)) return fail(E_ARG, "null pointer");
    const int curve = r1->curve;
    const size_t B = (size_t)curve_info(curve)->field_bytes;
    if (where == Mem::device)
      for (const u8* k : {k1, k2})
        if (overlap2(k, n * B, out_xy, n * 2 * B) || overlap2(k, n * B, out_inf, n))
          return fail(E_ARG, "k1 / k2 and the results must not overlap");
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    if (!r1->ed) base_upload(curve);
    return batch(where, n, {In{k1, B}, In{k2, B}}, {Out{out_xy, 2 * B}, Out{out_inf, 1}}, [&](size_t m, auto d, auto o) {
      return walk_tables(*r1, r2, m, d[0], d[1], o[0], o[1]);
    });
  }

  // ok: the verdicts, strictly 0 / 1.  st (may be null): the domain status per item -- 2 where the
  // key is not on the curve (verdict 0 there), else 0 (Work::store_verdict)
  int ecdsa_verify(Mem where, int curve, size_t n, const u8* hash, int hash_len, int msg_bits,
                   const u8* r, const u8* s, const u8* pub, u8* ok, u8* st) {
    const CurveInfo* ci = curve_info(curve);
    if (!ci) return fail(E_ARG, "unknown curve id");
    const bool nul = n && (!hash || !r || !s || !pub || !ok);
    if (int rc = host_first(where, nul, hash_len)) return rc;
    const bool dom = custom_is_domain(curve);
    CustomScope sc(this, dom || where == Mem::host ? curve : -1);      // as mul_fixed
    if (sc.rc) return sc.rc;
    int shift = 0;                 // a domain's own n, in 8 words
    if (asks_curve(where, n)) {
      if (curve >= CURVE_ED25519 && !dom)
        return fail(E_UNSUPPORTED, is_custom(curve) ? "ECDSA verify on a user-defined curve needs its domain (ellgpu_curve_define_short_domain)"
                                                    : "ECDSA verify is implemented for the short Weierstrass presets");
      if (nul) return fail(E_ARG, "null pointer");
      int rc = dom ? truncate_shift(hash_len, msg_bits, (int)custom_[(size_t)(curve - CURVE_CUSTOM0)].nbits, 8, shift)
                   : truncate_shift(hash_len, msg_bits, ci->order_bits, (ci->order_bits + 31) / 32, shift);
      if (rc) return rc;
    }
    const size_t B = ci->field_bytes, NB = ci->order_bytes;
    return batch(where, n, {In{hash, (size_t)hash_len}, In{r, NB}, In{s, NB}, In{pub, 2 * B}}, {Out{ok, 1}, Out{st, 1}},
                 [&](size_t m, auto d, auto o) {
      int rc = dom ? ensure_comb<CvCustomDomain>() : prepare_curve(curve);
      if (rc) return rc;
      if (dom) rc = ecdsa_chunk<CvCustomDomain>(m, d[0], hash_len, shift, d[1], d[2], d[3], o[0], o[1]);
      else ELL_SHORT_DISPATCH(curve, rc = ecdsa_chunk<CV>(m, d[0], hash_len, shift, d[1], d[2], d[3], o[0], o[1]));
      return rc;
    });
  }

  // EC#verify against the fixed-base table of the signer's key: ok[i] is what ecdsa_verify writes
  // for the same item with the point of `base` as its key, strictly 0 / 1.  Both scalar
  // multiplications are comb walks (u1 over G's table -- the curve's own, at the width it has --
  // and u2 over the key's, at the width it was defined with).  No status: the key was tested
  // against the curve when the handle was defined.  Handles of define_base on the six presets and
  // on user-defined short DOMAIN ids, the generator alias included (the key with d = 1).
  int ecdsa_verify_base(Mem where, int base, size_t n, const u8* hash, int hash_len, int msg_bits,
                        const u8* r, const u8* s, u8* ok) {
    const BaseRec* rec = base_rec(base);
    if (!rec) return E_ARG;
    if (rec->ed)
      return fail(E_UNSUPPORTED, "ECDSA verify against a key handle is implemented for short Weierstrass curves (an Edwards handle: ellgpu_custom_ed_verify takes the key per item)");
    const int curve = rec->curve;
    const bool dom = custom_is_domain(curve);
    if (is_custom(curve) && !dom)
      return fail(E_UNSUPPORTED, "ECDSA verify on a user-defined curve needs its domain (ellgpu_curve_define_short_domain)");
    if (!n) return E_OK;
    const bool nul = !hash || !r || !s || !ok;
    if (int rc = host_first(where, nul, hash_len)) return rc;
    if (nul) return fail(E_ARG, "null pointer");
    const CurveInfo* ci = curve_info(curve);
    const size_t NB = ci->order_bytes;
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    int shift = 0;
    if (int rc = dom ? truncate_shift(hash_len, msg_bits, (int)custom_[(size_t)(curve - CURVE_CUSTOM0)].nbits, 8, shift)
                     : truncate_shift(hash_len, msg_bits, ci->order_bits, (ci->order_bits + 31) / 32, shift))
      return rc;
    if (where == Mem::device)
      if (overlap2(hash, n * (size_t)hash_len, ok, n) || overlap2(r, n * NB, ok, n) || overlap2(s, n * NB, ok, n))
        return fail(E_ARG, "hash / r / s and the verdicts must not overlap");
    return batch(where, n, {In{hash, (size_t)hash_len}, In{r, NB}, In{s, NB}}, {Out{ok, 1}}, [&](size_t m, auto d, auto o) {
      int rc = dom ? ensure_comb<CvCustomDomain>() : prepare_curve(curve);
      const void* tq = nullptr;
      if (rc == E_OK) rc = base_table_ptr(*rec, tq);
      if (rc) return rc;
      const void* tg = comb_[curve];
      if (dom) {
        typedef const Work<CvCustomDomain>::A* T;
        return ecdsa_base_chunk<CvCustomDomain>(m, d[0], hash_len, shift, d[1], d[2], (T)tg, (T)tq, o[0]);
      }
      ELL_SHORT_DISPATCH(curve, rc = ecdsa_base_chunk<CV>(m, d[0], hash_len, shift, d[1], d[2], (const typename Work<CV>::A*)tg,
                                                           (const typename Work<CV>::A*)tq, o[0]));
      return rc;
    });
  }

  // out_bad (may be null): out_bad[i] = 1 where x[i] is no abscissa of the curve (KeyPair#derive's validate)
  int x25519(Mem where, size_t n, const u8* k, const u8* x, u8* out_x, u8* out_inf, u8* out_bad = nullptr) {
    if (n && (!k || !x || !out_x || !out_inf)) return fail(E_ARG, "null pointer");
    return batch(where, n, {In{k, 32}, In{x, 32}}, {Out{out_x, 32}, Out{out_inf, 1}, Out{out_bad, 1}},
                 [&](size_t m, auto d, auto r) { return x25519_chunk(m, d[0], d[1], r[0], r[1], r[2]); });
  }

  // ECDSA sign on the presets.  nonces != null: caller-supplied nonces, one pass of EC#sign's loop
  // per item; nonces == null (det): the reference's own nonce source (HmacDRBG, deterministic)
  int ecdsa_sign(Mem where, int curve, size_t n, const u8* hash, int hash_len, int msg_bits, const u8* priv,
                 const u8* nonces, bool det, int canonical, u8* out_r, u8* out_s, u8* out_recid, u8* out_ok) {
    const CurveInfo* ci = curve_info(curve);
    if (!ci) return fail(E_ARG, "unknown curve id");
    const bool nul = n && (!hash || !priv || (!det && !nonces) || !out_r || !out_s || !out_recid || !out_ok);
    if (int rc = host_first(where, nul, hash_len)) return rc;
    int shift = 0;
    if (asks_curve(where, n)) {
      if (curve >= CURVE_ED25519)
        return fail(E_UNSUPPORTED, "ECDSA sign is implemented for the short Weierstrass presets");
      if (nul) return fail(E_ARG, "null pointer");
      if (int rc = truncate_shift(hash_len, msg_bits, ci->order_bits, (ci->order_bits + 31) / 32, shift)) return rc;
    }
    const size_t NB = ci->order_bytes;
    return batch(where, n, {In{hash, (size_t)hash_len}, In{priv, NB}, In{det ? nullptr : nonces, NB}},
                 {Out{out_r, NB}, Out{out_s, NB}, Out{out_recid, 1}, Out{out_ok, 1}}, [&](size_t m, auto d, auto r) {
      int rc = prepare_curve(curve);
      if (rc) return rc;
      if (det) ELL_SHORT_DISPATCH(curve, rc = sign_det_chunk<CV>(m, d[0], hash_len, shift, d[1], canonical, r[0], r[1], r[2], r[3]))
      else ELL_SHORT_DISPATCH(curve, rc = sign_chunk<CV>(m, d[0], hash_len, shift, d[1], d[2], canonical, r[0], r[1], r[2], r[3]));
      return rc;
    });
  }

  // EC#recoverPubKey (ec/index.js:231-259) over a batch: status 0 point / 1 infinity /
  // 2 the reference throws / 3 outside the engine's domain (r = 0 or r >= n)
  int ecdsa_recover(Mem where, int curve, size_t n, const u8* hash, int hash_len, const u8* r, const u8* s,
                    const u8* recid, u8* out_xy, u8* out_status) {
    const CurveInfo* ci = curve_info(curve);
    if (!ci) return fail(E_ARG, "unknown curve id");
    const bool nul = n && (!hash || !r || !s || !recid || !out_xy || !out_status);
    if (int rc = host_first(where, nul, hash_len)) return rc;
    if (asks_curve(where, n)) {
      if (curve >= CURVE_ED25519)
        return fail(E_UNSUPPORTED, "public-key recovery is an ECDSA (short Weierstrass) operation");
      if (nul) return fail(E_ARG, "null pointer");
      if (hash_len <= 0 || hash_len > 8 * ((ci->order_bits + 31) / 32))
        return fail(E_ARG, "hash_len must be 1 .. twice the order width");
    }
    const size_t B = ci->field_bytes, NB = ci->order_bytes;
    return batch(where, n, {In{hash, (size_t)hash_len}, In{r, NB}, In{s, NB}, In{recid, 1}},
                 {Out{out_xy, 2 * B}, Out{out_status, 1}}, [&](size_t m, auto d, auto o) {
      int rc = prepare_curve(curve);
      if (rc) return rc;
      ELL_SHORT_DISPATCH(curve, rc = recover_chunk<CV>(m, d[0], hash_len, d[1], d[2], d[3], o[0], o[1]));
      return rc;
    });
  }

  // EC#getKeyRecoveryParam (ec/index.js:261-278) over a batch, in one pass instead of the
  // reference's up to four recoveries (Work::recid_prep): status 0 with the id in out_recid /
  // 1 the reference throws ('Unable to find valid recovery factor') / 2 the key is not on the
  // curve / 3 outside the engine's domain (r = 0, r >= n or s = 0 mod n).  The six presets only:
  // the rule rests on cofactor 1 and a prime n, which nothing promises of a user-defined id.
  int ecdsa_recid(Mem where, int curve, size_t n, const u8* hash, int hash_len, const u8* r, const u8* s,
                  const u8* pub_xy, u8* out_recid, u8* out_status) {
    const CurveInfo* ci = curve_info(curve);
    if (!ci || (is_custom(curve) && !custom_block(curve))) return fail(E_ARG, "unknown curve id");
    if (curve >= CURVE_ED25519)
      return fail(E_UNSUPPORTED, is_custom(curve) ? "the one-pass recovery id is implemented for the short Weierstrass presets (a user-defined curve may have a cofactor: run EC#getKeyRecoveryParam's loop over ellgpu_custom_recover)"
                                                  : "the recovery id is an ECDSA (short Weierstrass) notion");
    if (!out_status || (n && (!hash || !r || !s || !pub_xy || !out_recid))) return fail(E_ARG, "null pointer");
    if (hash_len <= 0 || hash_len > 8 * ((ci->order_bits + 31) / 32))
      return fail(E_ARG, "hash_len must be 1 .. twice the order width");
    const size_t B = ci->field_bytes, NB = ci->order_bytes;
    if (where == Mem::device) {
      // r and the key are read again after the statuses are written (recid_finish, the curve test)
      const u8* const ins[4] = {hash, r, s, pub_xy};
      const size_t lens[4] = {n * (size_t)hash_len, n * NB, n * NB, n * 2 * B};
      for (int k = 0; k < 4; k++)
        if (overlap2(ins[k], lens[k], out_recid, n) || overlap2(ins[k], lens[k], out_status, n))
          return fail(E_ARG, "hash / r / s / pub_xy and the results must not overlap");
      if (overlap2(out_recid, n, out_status, n)) return fail(E_ARG, "out_recid and out_status must not overlap");
    }
    return batch(where, n, {In{hash, (size_t)hash_len}, In{r, NB}, In{s, NB}, In{pub_xy, 2 * B}},
                 {Out{out_recid, 1}, Out{out_status, 1}}, [&](size_t m, auto d, auto o) {
      int rc = prepare_curve(curve);
      if (rc) return rc;
      ELL_SHORT_DISPATCH(curve, rc = recid_chunk<CV>(m, d[0], hash_len, d[1], d[2], d[3], o[0], o[1]));
      return rc;
    });
  }

  // n sums of m terms k * P each (include/ellgpu_addn.h): _wnafMulAdd / _endoWnafMulAdd on any number
  // of points.  The short curves only: the presets and user-defined short ids, plain and domain.
  // An item of the batch is a whole sum (strides m B and m 2 B); a chunk is a group of sums whose
  // pairs of terms and results fit one launch (sum_group_max), or one slice after the other of a sum
  // that is longer than that (sum_chunk).  One item per lane at every n: form_for is not consulted.
  // Sums per chunk: the pairs (ceil(m / 2) per sum) fit the slice size, and the pairs and the results
  // together CHUNK entries of Jacobian scratch.  0: one sum has more pairs than that -- slices.
  size_t sum_group_max(size_t m) const {
    const size_t P = m / 2 + (m & 1);
    const size_t a = tune_.sum_slice / P, b = CHUNK / (P + 1);
    return a < b ? a : b;
  }
  int mul_sum(Mem where, int curve, size_t n, size_t m, const u8* k, const u8* xy, u8* out_xy, u8* out_inf) {
    const CurveInfo* ci = curve_info(curve);
    if (!ci || (is_custom(curve) && !custom_block(curve))) return fail(E_ARG, "unknown curve id");
    if (curve == CURVE_ED25519 || custom_is_edwards(curve))
      return fail(E_UNSUPPORTED, "sums of k * P terms are implemented for the short Weierstrass curves; Edwards curves are a later change (ellgpu_mul_add2 takes two terms there)");
    if (curve == CURVE_CURVE25519 || custom_is_mont(curve))
      return fail(E_UNSUPPORTED, "Not supported on Montgomery curve");     // mont.js:155-157
    if (m == 0) return fail(E_ARG, "m must be at least 1");
    const size_t B = ci->field_bytes;
    if (n && (m > SIZE_MAX / n || n * m > SIZE_MAX / (2 * B))) return fail(E_ARG, "n * m terms do not fit size_t");
    if (n && (!k || !xy || !out_xy || !out_inf)) return fail(E_ARG, "null pointer");
    if (n == 0) return E_OK;
    if (where == Mem::device) {
      // the flags of the terms are folded into out_inf after the results are written
      const u8* const ins[2] = {k, xy};
      const size_t lens[2] = {n * m * B, n * m * 2 * B};
      for (int i = 0; i < 2; i++)
        if (overlap2(ins[i], lens[i], out_xy, n * 2 * B) || overlap2(ins[i], lens[i], out_inf, n))
          return fail(E_ARG, "k / xy and the results must not overlap");
      if (overlap2(out_xy, n * 2 * B, out_inf, n)) return fail(E_ARG, "out_xy and out_inf must not overlap");
    }
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    const size_t G = sum_group_max(m);
    return batch(where, n, {In{k, m * B}, In{xy, m * 2 * B}}, {Out{out_xy, 2 * B}, Out{out_inf, 1}},
                 [&](size_t c, auto d, auto r) {
      return for_chunks(c, G ? G : 1, [&](size_t o, size_t g) {
        int rc = E_OK;
        const u8* kk = d[0] + o * m * B;
        const u8* pp = d[1] + o * m * 2 * B;
        if (is_custom(curve)) rc = sum_chunk<CvCustom>(g, m, kk, pp, r[0] + o * 2 * B, r[1] + o);
        else ELL_SHORT_DISPATCH(curve, rc = sum_chunk<CV>(g, m, kk, pp, r[0] + o * 2 * B, r[1] + o));
        return rc;
      });
    });
  }

  // The same on the Edwards curves (elliptic_amd/include/ellgpu_edsum.h): ed25519 and user-defined
  // Edwards ids, plain and domain -- a domain id is the plain curve it also is.  B = 32 everywhere.
  // The identity comes out as the family's normalisation writes it ((0, 1); out_inf 1 on ed25519, 0
  // on a user-defined id), the unified law takes torsion points and the identity as ordinary terms.
  // Chunks and slices as mul_sum's; one item per lane at every n: coop_grid() is not consulted.
  int ed_mul_sum(Mem where, int curve, size_t n, size_t m, const u8* k, const u8* xy, u8* out_xy, u8* out_inf) {
    const CurveInfo* ci = curve_info(curve);
    if (!ci || (is_custom(curve) && !custom_block(curve))) return fail(E_ARG, "unknown curve id");
    if (curve == CURVE_CURVE25519 || custom_is_mont(curve))
      return fail(E_UNSUPPORTED, "Not supported on Montgomery curve");     // mont.js:155-157
    if (curve != CURVE_ED25519 && !custom_is_edwards(curve))
      return fail(E_UNSUPPORTED, "sums of k * P terms on the short Weierstrass curves are ellgpu_mul_sum's; this entry point takes ed25519 and user-defined Edwards ids");
    if (m == 0) return fail(E_ARG, "m must be at least 1");
    const size_t B = 32;
    if (n && (m > SIZE_MAX / n || n * m > SIZE_MAX / (2 * B))) return fail(E_ARG, "n * m terms do not fit size_t");
    if (n && (!k || !xy || !out_xy || !out_inf)) return fail(E_ARG, "null pointer");
    if (n == 0) return E_OK;
    if (where == Mem::device) {
      // the flags of the terms are folded into out_inf after the results are written
      const u8* const ins[2] = {k, xy};
      const size_t lens[2] = {n * m * B, n * m * 2 * B};
      for (int i = 0; i < 2; i++)
        if (overlap2(ins[i], lens[i], out_xy, n * 2 * B) || overlap2(ins[i], lens[i], out_inf, n))
          return fail(E_ARG, "k / xy and the results must not overlap");
      if (overlap2(out_xy, n * 2 * B, out_inf, n)) return fail(E_ARG, "out_xy and out_inf must not overlap");
    }
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    const size_t G = sum_group_max(m);
    return batch(where, n, {In{k, m * B}, In{xy, m * 2 * B}}, {Out{out_xy, 2 * B}, Out{out_inf, 1}},
                 [&](size_t c, auto d, auto r) {
      return for_chunks(c, G ? G : 1, [&](size_t o, size_t g) {
        const u8* kk = d[0] + o * m * B;
        const u8* pp = d[1] + o * m * 2 * B;
        return is_custom(curve) ? ed_sum_chunk<EdcWork>(g, m, kk, pp, r[0] + o * 2 * B, r[1] + o)
                                : ed_sum_chunk<EdWork>(g, m, kk, pp, r[0] + o * 2 * B, r[1] + o);
      });
    });
  }

  // EdDSA (ed25519).  msgs: concatenated message bytes; off (n + 1 offsets, in the memory the
  // other operands are in) or, if null, a uniform stride msg_len.  Whole-buffer operands: a host
  // call goes through staged_whole(), and tests the offsets it can read.
  int check_eddsa_messages(size_t n, const u8* msgs, const u64* off, size_t msg_len, size_t& total) {
    if (off)                       // len = off[i+1] - off[i] per item: offsets must not decrease
      for (size_t i = 0; i < n; i++)
        if (off[i] > off[i + 1]) return fail(E_ARG, "message offsets must be non-decreasing");
    total = off ? (size_t)off[n] : n * msg_len;
    if (total && !msgs) return fail(E_ARG, "null message pointer");
    return E_OK;
  }
  int eddsa_verify(Mem where, size_t n, const u8* msgs, const u64* off, size_t msg_len, const u8* sigs,
                   const u8* pubs, u8* ok, u8* err) {
    auto run = [&](const u8* dm, const u64* doff, const u8* ds, const u8* dp, u8* dok, u8* derr) {
      if (n && (!ds || !dp || !dok || (!dm && (doff || msg_len)))) return fail(E_ARG, "null pointer");
      return for_chunks(n, CHUNK, [&](size_t o, size_t m) {
        if (int rc = prepare_curve(CURVE_ED25519)) return rc;
        return eddsa_chunk(m, o, dm, doff, msg_len, ds, dp, dok, derr);
      });
    };
    if (where == Mem::device) return run(msgs, off, sigs, pubs, ok, err);
    if (n && (!sigs || !pubs || !ok)) return fail(E_ARG, "null pointer");
    size_t total;
    if (int rc = check_eddsa_messages(n, msgs, off, msg_len, total)) return rc;
    return staged_whole(n, {In{msgs ? msgs : (const u8*)"", total}, In{off, off ? (n + 1) * sizeof(u64) : 0, true},
                            In{sigs, n * 64}, In{pubs, n * 32}},
                        {Out{ok, n}, Out{err, n}}, [&](auto d, auto r) {
      return run(d[0], (const u64*)d[1], d[2], d[3], r[0], r[1]);
    });
  }
  // EDDSA#verify(msg, sig, A) with A the point of a define_ed_base handle on ed25519: ok and err are
  // what eddsa_verify writes for the same items with encodePoint(A) repeated as the key.  h walks
  // the key's comb and S the curve's own (the generator alias: both walks read that one).  The
  // handle is looked up before n is: the refusals hold for an empty batch too.
  int eddsa_verify_base(Mem where, int base, size_t n, const u8* msgs, const u64* off, size_t msg_len,
                        const u8* sigs, u8* ok, u8* err) {
    const BaseRec* rec = base_rec(base);
    if (!rec) return E_ARG;
    if (!rec->ed)
      return fail(E_UNSUPPORTED, "EdDSA verify against a key handle takes a handle of ellgpu_ed_base_define on ed25519 (a short Weierstrass handle: ellgpu_ecdsa_verify_base)");
    if (rec->curve != CURVE_ED25519)
      return fail(E_UNSUPPORTED, "the engine has no EdDSA on a user-defined Edwards curve: EdDSA verify against a key handle is ed25519's");
    if (!rec->alias && rec->t.bits != EdWork::COMB_BITS)
      return fail(E_UNSUPPORTED, "the key's table does not have the width of ed25519's own comb");
    if (!n) return E_OK;
    if (!sigs || !ok) return fail(E_ARG, "null pointer");
    // encodePoint(A), once per call: the generator alias keeps no coordinates of its own
    u8 axy[64], enc[32];
    if (rec->alias) {
      u32 gx[8], gy[8];
      for (int i = 0; i < 8; i++) { gx[i] = consts::ED25519_C::gx_plain[i]; gy[i] = consts::ED25519_C::gy_plain[i]; }
      store_be<8>(axy, gx, 32);
      store_be<8>(axy + 32, gy, 32);
    } else {
      memcpy(axy, rec->xy, 64);
    }
    EdWork::encode_affine(enc, axy);
    u64 aw[4];
    EdWork::bytes_to_words(aw, enc);
    auto run = [&](const u8* dm, const u64* doff, const u8* ds, u8* dok, u8* derr) {
      if (!dm && (doff || msg_len)) return fail(E_ARG, "null pointer");
      return for_chunks(n, CHUNK, [&](size_t o, size_t m) {
        if (int rc = prepare_curve(CURVE_ED25519)) return rc;
        const void* tq = nullptr;
        if (int rc = base_table_ptr(*rec, tq)) return rc;
        return eddsa_base_chunk(m, o, dm, doff, msg_len, ds, aw, (const EdWork::P*)comb_[CURVE_ED25519],
                                (const EdWork::P*)tq, dok, derr);
      });
    };
    if (where == Mem::device) {
      // (with offsets in device memory the host does not know where the messages end: their extent
      // is then taken as the offsets' own array and the first message byte)
      const size_t mlen = off ? 1 : n * msg_len;
      const u8* ins[3] = {sigs, msgs, (const u8*)off};
      const size_t lens[3] = {n * 64, mlen, off ? (n + 1) * sizeof(u64) : 0};
      for (int k = 0; k < 3; k++)
        if (overlap2(ins[k], lens[k], ok, n) || overlap2(ins[k], lens[k], err, n))
          return fail(E_ARG, "sigs / msgs / msg_off and the results must not overlap");
      if (overlap2(ok, n, err, n)) return fail(E_ARG, "out_ok and out_err must not overlap");
      return run(msgs, off, sigs, ok, err);
    }
    size_t total;
    if (int rc = check_eddsa_messages(n, msgs, off, msg_len, total)) return rc;
    return staged_whole(n, {In{msgs ? msgs : (const u8*)"", total}, In{off, off ? (n + 1) * sizeof(u64) : 0, true},
                            In{sigs, n * 64}},
                        {Out{ok, n}, Out{err, n}}, [&](auto d, auto r) {
      return run(d[0], (const u64*)d[1], d[2], r[0], r[1]);
    });
  }
  // EDDSA#sign with KeyPair.fromSecret, from 32-byte secrets; pub (n x 32, the encoded public
  // keys) may be null
  int eddsa_sign(Mem where, size_t n, const u8* secrets, const u8* msgs, const u64* off, size_t msg_len,
                 u8* sig, u8* pub) {
    auto run = [&](const u8* dsec, const u8* dm, const u64* doff, u8* dsig, u8* dpub) {
      if (n && (!dsec || !dsig || (!dm && (doff || msg_len)))) return fail(E_ARG, "null pointer");
      return for_chunks(n, CHUNK / 2, [&](size_t o, size_t m) {     // two fixed-base multiplications per item
        if (int rc = prepare_curve(CURVE_ED25519)) return rc;
        return eddsa_sign_chunk(m, o, dsec, dm, doff, msg_len, dsig, dpub);
      });
    };
    if (where == Mem::device) return run(secrets, msgs, off, sig, pub);
    if (n && (!secrets || !sig)) return fail(E_ARG, "null pointer");
    size_t total;
    if (int rc = check_eddsa_messages(n, msgs, off, msg_len, total)) return rc;
    return staged_whole(n, {In{msgs ? msgs : (const u8*)"", total}, In{off, off ? (n + 1) * sizeof(u64) : 0, true},
                            In{secrets, n * 32}},
                        {Out{sig, n * 64}, Out{pub, n * 32}}, [&](auto d, auto r) {
      return run(d[2], d[0], (const u64*)d[1], r[0], r[1]);
    });
  }

  // point decompression: short curves from x (pointFromX), ed25519 from y (pointFromY)
  int decompress(Mem where, int curve, size_t n, const u8* v, const u8* odd, u8* out_xy, u8* out_ok) {
    const CurveInfo* ci = curve_info(curve);
    if (!ci) return fail(E_ARG, "unknown curve id");
    const bool nul = n && (!v || !odd || !out_xy || !out_ok);
    if (int rc = host_first(where, nul)) return rc;
    if (asks_curve(where, n)) {
      if (curve == CURVE_CURVE25519) return fail(E_UNSUPPORTED, "curve25519 points are x-only");
      if (nul) return fail(E_ARG, "null pointer");
    }
    const size_t B = ci->field_bytes;
    return batch(where, n, {In{v, B}, In{odd, 1}}, {Out{out_xy, 2 * B}, Out{out_ok, 1}}, [&](size_t m, auto d, auto r) {
      int rc = E_OK;
      if (curve == CURVE_ED25519) rc = ed_decompress_chunk(m, d[0], d[1], r[0], r[1]);
      else ELL_SHORT_DISPATCH(curve, rc = decompress_chunk<CV>(m, d[0], d[1], r[0], r[1]));
      return rc;
    });
  }

  // ---- SEC1 / EdDSA point codecs and key validation --------------------------------
  enum { OP_DECODE = 0, OP_ENCODE = 1, OP_VALIDATE = 2 };
  // decodePoint (base.js:270-293; eddsa/index.js:99-109): n encodings of enc_len bytes each
  int decode_points(Mem where, int curve, size_t n, const u8* enc, size_t enc_len, u8* out_xy, u8* out_status) {
    const CurveInfo* ci = curve_info(curve);
    if (!ci) return fail(E_ARG, "unknown curve id");
    const bool nul = n && (!enc || !out_xy || !out_status);
    if (int rc = host_first(where, nul)) return rc;
    if (asks_curve(where, n)) {
      if (curve == CURVE_CURVE25519) return fail(E_UNSUPPORTED, "curve25519 points are x-only");
      if (nul) return fail(E_ARG, "null pointer");
      if (curve == CURVE_ED25519 && enc_len != 32) return fail(E_ARG, "ed25519 encodings are 32 bytes");
      if (enc_len == 0) return fail(E_ARG, "enc_len must be positive");
    }
    const size_t B = ci->field_bytes;
    return batch(where, n, {In{enc, enc_len}}, {Out{out_xy, 2 * B}, Out{out_status, 1}}, [&](size_t m, auto d, auto r) {
      int rc = E_OK;
      if (curve == CURVE_ED25519) rc = ed_codec_chunk(OP_DECODE, m, d[0], 0, nullptr, r[0], r[1]);
      else ELL_SHORT_DISPATCH(curve, rc = codec_chunk<CV>(OP_DECODE, m, d[0], enc_len, 0, nullptr, r[0], r[1]));
      return rc;
    });
  }
  static size_t encoded_len(int curve, size_t B, int compact) {
    return curve == CURVE_ED25519 ? 32 : (compact ? 1 + B : 1 + 2 * B);
  }
  // BasePoint#encode (base.js:295-311) / EDDSA#encodePoint (eddsa/index.js:94-98)
  int encode_points(Mem where, int curve, size_t n, const u8* xy, int compact, u8* out_enc) {
    const CurveInfo* ci = curve_info(curve);
    if (!ci) return fail(E_ARG, "unknown curve id");
    const bool nul = n && (!xy || !out_enc);
    if (int rc = host_first(where, nul)) return rc;
    if (asks_curve(where, n)) {
      if (curve == CURVE_CURVE25519) return fail(E_UNSUPPORTED, "curve25519 points are x-only");
      if (nul) return fail(E_ARG, "null pointer");
    }
    const size_t B = ci->field_bytes;
    return batch(where, n, {In{xy, 2 * B}}, {Out{out_enc, encoded_len(curve, B, compact)}}, [&](size_t m, auto d, auto r) {
      int rc = E_OK;
      if (curve == CURVE_ED25519) rc = ed_codec_chunk(OP_ENCODE, m, d[0], 0, nullptr, r[0], nullptr);
      else ELL_SHORT_DISPATCH(curve, rc = codec_chunk<CV>(OP_ENCODE, m, d[0], 0, compact, nullptr, r[0], nullptr));
      return rc;
    });
  }
  // KeyPair#validate (ec/key.js:41-52): 0 ok, 1 'Invalid public key' (inf[i] set), 2 'Public key
  // is not a point', 3 'Public key * N != O' (only tested when check_order)
  int validate(Mem where, int curve, size_t n, const u8* xy, const u8* inf, int check_order, u8* out_status) {
    const CurveInfo* ci = curve_info(curve);
    if (!ci) return fail(E_ARG, "unknown curve id");
    const bool nul = n && (!xy || !out_status);
    if (int rc = host_first(where, nul)) return rc;
    if (asks_curve(where, n)) {
      if (curve == CURVE_CURVE25519) return fail(E_UNSUPPORTED, "curve25519 points are x-only");
      if (nul) return fail(E_ARG, "null pointer");
    }
    const size_t B = ci->field_bytes;
    return batch(where, n, {In{xy, 2 * B}, In{inf, 1}}, {Out{out_status, 1}}, [&](size_t m, auto d, auto r) {
      int rc = E_OK;
      if (curve == CURVE_ED25519) rc = ed_codec_chunk(OP_VALIDATE, m, d[0], check_order, d[1], nullptr, r[0]);
      else ELL_SHORT_DISPATCH(curve, rc = codec_chunk<CV>(OP_VALIDATE, m, d[0], 0, check_order, d[1], nullptr, r[0]));
      return rc;
    });
  }

  // ---- Point#add on affine points (short.js:365-412, edwards.js:350-360) ----------------
  int point_add(Mem where, int curve, size_t n, const u8* xy1, const u8* inf1, const u8* xy2, const u8* inf2,
                u8* out_xy, u8* out_inf) {
    const CurveInfo* ci = curve_info(curve);
    if (!ci) return fail(E_ARG, "unknown curve id");
    const bool nul = n && (!xy1 || !xy2 || !out_xy || !out_inf);
    if (int rc = host_first(where, nul)) return rc;
    if (asks_curve(where, n)) {
      if (curve == CURVE_CURVE25519) return fail(E_UNSUPPORTED, "Not supported on Montgomery curve");   // mont.js:103-105
      if (nul) return fail(E_ARG, "null pointer");
    }
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    const size_t B = ci->field_bytes;
    return batch(where, n, {In{xy1, 2 * B}, In{inf1, 1}, In{xy2, 2 * B}, In{inf2, 1}}, {Out{out_xy, 2 * B}, Out{out_inf, 1}},
                 [&](size_t m, auto d, auto r) {
      int rc = E_OK;
      if (custom_is_edwards(curve)) rc = edc_chunk(2, m, nullptr, d[0], nullptr, d[2], d[1], d[3], r[0], r[1]);
      else if (is_custom(curve)) rc = point_add_chunk<CvCustom>(m, d[0], d[1], d[2], d[3], r[0], r[1]);
      else if (curve == CURVE_ED25519) rc = ed_point_add_chunk(m, d[0], d[1], d[2], d[3], r[0], r[1]);
      else ELL_SHORT_DISPATCH(curve, rc = point_add_chunk<CV>(m, d[0], d[1], d[2], d[3], r[0], r[1]));
      return rc;
    });
  }

  // ---- signature DER codec and EC#verify on wire formats ------------------------------
  enum { OP_FROM_DER = 0, OP_TO_DER = 1, OP_WIRE_STATUS = 2 };
  int check_short(int curve, const CurveInfo*& ci) {
    ci = curve_info(curve);
    if (!ci) return fail(E_ARG, "unknown curve id");
    if (curve >= CURVE_ED25519) return fail(E_UNSUPPORTED, "ECDSA signatures belong to the short Weierstrass presets");
    return E_OK;
  }
  // Signature#_importDER (ec/signature.js:83-147): der = n records of `stride` bytes, der_len[i] used
  int sig_from_der(Mem where, int curve, size_t n, const u8* der, size_t stride, const u32* der_len,
                   u8* out_r, u8* out_s, u8* out_status) {
    const CurveInfo* ci;
    int rc = check_short(curve, ci);
    if (rc) return rc;
    if (n && (!der || !der_len || !out_r || !out_s || !out_status)) return fail(E_ARG, "null pointer");
    if (asks_curve(where, n) && stride == 0) return fail(E_ARG, "stride must be positive");
    const size_t NB = ci->order_bytes;
    return batch(where, n, {In{der, stride}, In{der_len, 4}}, {Out{out_r, NB}, Out{out_s, NB}, Out{out_status, 1}},
                 [&](size_t m, auto d, auto r) {
      ELL_SHORT_DISPATCH(curve, rc = der_chunk<CV>(OP_FROM_DER, m, d[0], nullptr, stride, (u32*)d[1], r[0], r[1], r[2]));
      return rc;
    });
  }
  // Signature#toDER (ec/signature.js:149-176): out = n records of `stride` >= 2 NB + 9 bytes
  int sig_to_der(Mem where, int curve, size_t n, const u8* r, const u8* s, u8* out_der, size_t stride, u32* out_len) {
    const CurveInfo* ci;
    int rc = check_short(curve, ci);
    if (rc) return rc;
    if (n && (!r || !s || !out_der || !out_len)) return fail(E_ARG, "null pointer");
    const size_t NB = ci->order_bytes;
    if (asks_curve(where, n) && stride < 2 * NB + 9) return fail(E_ARG, "stride must be at least 2 * order_bytes + 9");
    return batch(where, n, {In{r, NB}, In{s, NB}}, {Out{out_der, stride}, Out{out_len, 4}}, [&](size_t m, auto d, auto o) {
      ELL_SHORT_DISPATCH(curve, rc = der_chunk<CV>(OP_TO_DER, m, d[0], d[1], stride, (u32*)o[1], o[0], nullptr, nullptr));
      return rc;
    });
  }
  // the scratch of a wire verify of m items: r, s (NB bytes each), the decoded key (2 B), and the
  // statuses of the key, the signature and the verify
  struct WireTmp { u8 *r, *s, *xy, *kst, *sst, *vst; };
  int wire_tmp(size_t m, size_t B, size_t NB, WireTmp& t) {
    t.r = claim<u8>(S_WIRE, m * (2 * NB + 2 * B + 3));
    if (int rc = claimed()) return rc;
    t.s = t.r + m * NB;
    t.xy = t.s + m * NB;
    t.kst = t.xy + m * 2 * B;
    t.sst = t.kst + m;
    t.vst = t.sst + m;
    return E_OK;
  }
  // EC#verify(msg, derSignature, encodedKey) (ec/index.js:188-229 with keyFromPublic ->
  // decodePoint and new Signature(der)): decode, parse and verify on the device -- the three
  // operations above, on scratch
  int ecdsa_verify_wire(Mem where, int curve, size_t n, const u8* hash, int hash_len, int msg_bits,
                        const u8* der, size_t der_stride, const u32* der_len, const u8* pub_enc,
                        size_t pub_len, u8* ok, u8* err) {
    const CurveInfo* ci;
    int rc = check_short(curve, ci);
    if (rc) return rc;
    if (n && (!hash || !der || !der_len || !pub_enc || !ok)) return fail(E_ARG, "null pointer");
    if ((rc = host_first(where, false, hash_len))) return rc;
    if (asks_curve(where, n) && (hash_len <= 0 || der_stride == 0 || pub_len == 0))
      return fail(E_ARG, "bad hash_len / stride / pub_len");
    const size_t B = ci->field_bytes, NB = ci->order_bytes;
    return batch(where, n, {In{hash, (size_t)hash_len}, In{der, der_stride}, In{der_len, 4}, In{pub_enc, pub_len}},
                 {Out{ok, 1}, Out{err, 1}}, [&](size_t m, auto d, auto o) {
      WireTmp t;
      if ((rc = wire_tmp(m, B, NB, t))) return rc;
      rc = decode_points(Mem::device, curve, m, d[3], pub_len, t.xy, t.kst);
      if (rc) return rc;
      rc = sig_from_der(Mem::device, curve, m, d[1], der_stride, (const u32*)d[2], t.r, t.s, t.sst);
      if (rc) return rc;
      rc = ecdsa_verify(Mem::device, curve, m, d[0], hash_len, msg_bits, t.r, t.s, t.xy, o[0], t.vst);
      if (rc) return rc;
      ELL_SHORT_DISPATCH(curve, rc = der_chunk<CV>(OP_WIRE_STATUS, m, t.kst, t.sst, 0, nullptr, o[0], o[1], t.vst));
      return rc;
    });
  }

  // ---- wire formats on user-defined short curves -------------------------------------------
  // ShortCurve#pointFromX, BaseCurve#decodePoint and EC#verify(msg, der, key) where the curve
  // is the caller's own (ellgpu_custom_*).  Entry points of their own: the preset-named ones
  // refuse user-defined ids before a kernel is chosen, and keep doing so.  Coordinates in and
  // out are 32 bytes; a SEC1 coordinate is p.byteLength() bytes, the block's pbytes.
  // The checks of the custom_* operations are the same in both forms, in the same order.
  enum { OP_RT_DECOMPRESS = 0, OP_RT_DECODE = 1, OP_RT_FROM_DER = 2, OP_RT_WIRE_STATUS = 3 };
  // The id check of every custom_* operation: a user-defined id of this context whose curve is of
  // `kind` (0 short, 1 Edwards, 2 Montgomery) and, with no_domain, has an ECDSA domain.  A preset
  // or unknown id is an argument error, the rest unsupported.  The messages: what to say to a preset
  // id, to another kind (a Montgomery id has one of its own where `mont` is set) and to a plain id.
  struct CustomIdMsgs { const char *preset, *kind, *mont, *no_domain; };
  int check_custom(int curve, u32 kind, const CustomIdMsgs& m) {
    if (!is_custom(curve)) return fail(E_ARG, curve_info(curve) ? m.preset : "unknown curve id");
    const RtField* f = custom_block(curve);
    if (!f) return fail(E_ARG, "unknown curve id");
    if (f->kind != kind) return fail(E_UNSUPPORTED, f->kind == 2 && m.mont ? m.mont : m.kind);
    if (m.no_domain && !f->domain) return fail(E_UNSUPPORTED, m.no_domain);
    return E_OK;
  }
  // a short curve; with no_domain: ... and a domain on it, for the operations that need n and G
  int check_custom_short(int curve, const char* no_domain = nullptr) {
    return check_custom(curve, 0, {"not a user-defined curve id (the presets have ellgpu_decompress, ellgpu_decode_points and ellgpu_ecdsa_verify_wire)",
                                   "not available on user-defined Edwards curves",
                                   "not available on user-defined Montgomery curves (x-only: ellgpu_custom_mont_ladder, _validate, _derive)",
                                   no_domain});
  }
  int custom_decompress(Mem where, int curve, size_t n, const u8* x, const u8* odd, u8* out_xy, u8* out_status) {
    int rc = check_custom_short(curve);
    if (rc) return rc;
    if (n && (!x || !odd || !out_xy || !out_status)) return fail(E_ARG, "null pointer");
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{x, 32}, In{odd, 1}}, {Out{out_xy, 64}, Out{out_status, 1}}, [&](size_t m, auto d, auto r) {
      return rt_wire_chunk(OP_RT_DECOMPRESS, m, d[0], d[1], 0, nullptr, r[0], r[1], nullptr);
    });
  }
  // enc_len other than 1 + pbytes and 1 + 2 pbytes is no error of the call: every item is then
  // 'Unknown point format', as in the reference
  int custom_decode_points(Mem where, int curve, size_t n, const u8* enc, size_t enc_len, u8* out_xy, u8* out_status) {
    int rc = check_custom_short(curve);
    if (rc) return rc;
    if (n && (!enc || !out_xy || !out_status)) return fail(E_ARG, "null pointer");
    if (enc_len == 0) return fail(E_ARG, "enc_len must be positive");
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{enc, enc_len}}, {Out{out_xy, 64}, Out{out_status, 1}}, [&](size_t m, auto d, auto r) {
      return rt_wire_chunk(OP_RT_DECODE, m, d[0], nullptr, enc_len, nullptr, r[0], r[1], nullptr);
    });
  }
  // EC#verify(msg, derSignature, encodedKey) on a domain: decode, parse and verify on the device,
  // composed like ecdsa_verify_wire
  int custom_verify_wire(Mem where, int curve, size_t n, const u8* hash, int hash_len, int msg_bits, const u8* der,
                         size_t der_stride, const u32* der_len, const u8* pub_enc, size_t pub_len, u8* ok, u8* err) {
    int rc = check_custom_short(curve, "ECDSA verify on a user-defined curve needs its domain (ellgpu_curve_define_short_domain)");
    if (rc) return rc;
    if (n && (!hash || !der || !der_len || !pub_enc || !ok)) return fail(E_ARG, "null pointer");
    if (hash_len <= 0 || der_stride == 0 || pub_len == 0) return fail(E_ARG, "bad hash_len / stride / pub_len");
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{hash, (size_t)hash_len}, In{der, der_stride}, In{der_len, 4}, In{pub_enc, pub_len}},
                 {Out{ok, 1}, Out{err, 1}}, [&](size_t m, auto d, auto o) {
      WireTmp t;
      if ((rc = wire_tmp(m, 32, 32, t))) return rc;
      rc = rt_wire_chunk(OP_RT_DECODE, m, d[3], nullptr, pub_len, nullptr, t.xy, t.kst, nullptr);
      if (rc) return rc;
      rc = rt_wire_chunk(OP_RT_FROM_DER, m, d[1], nullptr, der_stride, (const u32*)d[2], t.r, t.s, t.sst);
      if (rc) return rc;
      rc = ecdsa_verify(Mem::device, curve, m, d[0], hash_len, msg_bits, t.r, t.s, t.xy, o[0], t.vst);
      if (rc) return rc;
      return rt_wire_chunk(OP_RT_WIRE_STATUS, m, t.kst, t.sst, 0, nullptr, o[0], o[1], t.vst);
    });
  }

  // EC#recoverPubKey (ec/index.js:231-259) on a domain: status 0 point / 1 infinity / 2 the
  // reference throws / 3 r = 0 or r >= n, as ecdsa_recover.  e = new BN(hash) is not
  // truncated, only reduced mod n; s is not range-checked (the reference reduces it).
  int custom_recover(Mem where, int curve, size_t n, const u8* hash, int hash_len, const u8* r, const u8* s,
                     const u8* recid, u8* out_xy, u8* out_status) {
    int rc = check_custom_short(curve, "public-key recovery on a user-defined curve needs its domain (ellgpu_curve_define_short_domain)");
    if (rc) return rc;
    if (n && (!hash || !r || !s || !recid || !out_xy || !out_status)) return fail(E_ARG, "null pointer");
    if (hash_len < 1 || hash_len > 64) return fail(E_ARG, "hash_len must be 1 .. 64");
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{hash, (size_t)hash_len}, In{r, 32}, In{s, 32}, In{recid, 1}},
                 {Out{out_xy, 64}, Out{out_status, 1}}, [&](size_t m, auto d, auto o) {
      if ((rc = ensure_comb<CvCustomDomain>())) return rc;
      return rt_recover_chunk(m, d[0], hash_len, d[1], d[2], d[3], o[0], o[1]);
    });
  }

  // EC#sign (ec/index.js:110-186) on a domain: one pass of its loop for supplied nonces
  // (nonces != null), or with the reference's own HmacDRBG over drbg_hash (nonces == null).
  // The checks behind the domain check (rc: its result) are those of a short and of an Edwards domain.
  int check_custom_sign(int rc, int curve, size_t n, const u8* hash, int hash_len, int msg_bits, const u8* priv,
                        const u8* nonces, bool det, int drbg_hash, u8* out_r, u8* out_s, u8* out_recid,
                        u8* out_ok, int& shift) {
    if (rc) return rc;
    if (n && (!hash || !priv || (!det && !nonces) || !out_r || !out_s || !out_recid || !out_ok))
      return fail(E_ARG, "null pointer");
    if (hash_len < 1 || hash_len > 64) return fail(E_ARG, "hash_len must be 1 .. 64");
    if (det && (drbg_hash < 0 || drbg_hash > 2)) return fail(E_ARG, "drbg_hash must be ELLGPU_HASH_SHA256, _SHA384 or _SHA512");
    const int nbits = (int)custom_[(size_t)(curve - CURVE_CUSTOM0)].nbits;
    rc = truncate_shift(hash_len, msg_bits, nbits, 8, shift);
    if (rc) return rc;
    // hmac-drbg's constructor: entropy of n.byteLength() bytes against hmacStrength = 192 bits
    if (det && (nbits + 7) / 8 < 24)
      return fail(E_UNSUPPORTED, "EC#sign throws on this domain: 'Not enough entropy. Minimum is: 192 bits' (n.byteLength() < 24)");
    return E_OK;
  }
  int custom_sign(Mem where, int curve, size_t n, const u8* hash, int hash_len, int msg_bits, const u8* priv,
                  const u8* nonces, bool det, int drbg_hash, int canonical, u8* out_r, u8* out_s,
                  u8* out_recid, u8* out_ok) {
    int shift;
    int rc = check_custom_sign(check_custom_short(curve, "ECDSA sign on a user-defined curve needs its domain (ellgpu_curve_define_short_domain)"),
                               curve, n, hash, hash_len, msg_bits, priv, nonces, det, drbg_hash, out_r, out_s, out_recid, out_ok, shift);
    if (rc) return rc;
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{hash, (size_t)hash_len}, In{priv, 32}, In{det ? nullptr : nonces, 32}},
                 {Out{out_r, 32}, Out{out_s, 32}, Out{out_recid, 1}, Out{out_ok, 1}}, [&](size_t m, auto d, auto o) {
      if ((rc = ensure_comb<CvCustomDomain>())) return rc;
      return rt_sign_chunk(m, d[0], hash_len, shift, d[1], d[2], drbg_hash, canonical, o[0], o[1], o[2], o[3]);
    });
  }

  // ---- the key side on user-defined short curves: ECDH, validation, SEC1 encoding ---------------
  // KeyPair#derive (ec/key.js:101-107), KeyPair#validate (key.js:40-51) and BasePoint#encode
  // (base.js:295-311).  derive and encode need neither n nor G: a plain define_short id will do;
  // validate's order test needs the domain's n.
  int custom_pbytes() const { return (int)custom_[(size_t)(custom_curve_ - CURVE_CUSTOM0)].pbytes; }
  // wire: pub is n SEC1 encodings of pub_len bytes (ellgpu_custom_derive_wire) -- a length that is
  // neither 1 + pbytes nor 1 + 2 pbytes is no error of the call: every item is then 'Unknown point
  // format' -- else n x 64 raw coordinates (ellgpu_custom_derive).  rc: the curve check's result;
  // the rest is the same on a short and on an Edwards curve.
  int check_custom_derive(int rc, size_t n, const u8* priv, const u8* pub, bool wire, size_t pub_len, u8* out_x,
                          u8* out_status) {
    if (rc) return rc;
    if (n && (!priv || !pub || !out_x || !out_status)) return fail(E_ARG, "null pointer");
    if (wire && pub_len == 0) return fail(E_ARG, "pub_len must be positive");
    return E_OK;
  }
  int custom_derive(Mem where, int curve, size_t n, const u8* priv, const u8* pub, bool wire, size_t pub_len, u8* out_x,
                    u8* out_status, u8* out_err) {
    int rc = check_custom_derive(check_custom_short(curve), n, priv, pub, wire, pub_len, out_x, out_status);
    if (rc) return rc;
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{priv, 32}, In{pub, wire ? pub_len : 64}}, {Out{out_x, 32}, Out{out_status, 1}, Out{out_err, 1}},
                 [&](size_t m, auto d, auto o) {
      return rt_derive_chunk(m, d[0], d[1], wire ? pub_len : 0, o[0], o[1], o[2]);
    });
  }
  // statuses as validate's; check_order on a plain id: it has no n
  int custom_validate(Mem where, int curve, size_t n, const u8* xy, const u8* inf, int check_order, u8* out_status) {
    int rc = check_custom_short(curve, check_order ? "the order test on a user-defined curve needs its domain (ellgpu_curve_define_short_domain)" : nullptr);
    if (rc) return rc;
    if (n && (!xy || !out_status)) return fail(E_ARG, "null pointer");
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{xy, 64}, In{inf, 1}}, {Out{out_status, 1}}, [&](size_t m, auto d, auto o) {
      return rt_validate_chunk(m, d[0], d[1], check_order != 0, o[0]);
    });
  }
  // rows of 1 + pbytes (compact) or 1 + 2 pbytes bytes
  int custom_encode_points(Mem where, int curve, size_t n, const u8* xy, int compact, u8* out_enc) {
    int rc = check_custom_short(curve);
    if (rc) return rc;
    if (n && (!xy || !out_enc)) return fail(E_ARG, "null pointer");
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    const size_t EL = 1 + (compact ? 1 : 2) * (size_t)custom_pbytes();
    return batch(where, n, {In{xy, 64}}, {Out{out_enc, EL}}, [&](size_t m, auto d, auto o) {
      return rt_encode_chunk(m, d[0], compact, o[0]);
    });
  }

  // ---- user-defined Montgomery curves (ellgpu_custom_mont_*) --------------------------------
  // op as montc_chunk's.  A preset or unknown id is an argument error, a short or Edwards
  // user-defined id is unsupported.
  enum { OP_MONTC_LADDER = 0, OP_MONTC_VALIDATE = 1, OP_MONTC_DERIVE = 2 };
  int custom_mont(Mem where, int curve, int op, size_t n, const u8* k, const u8* x, u8* out_x, u8* out_flag) {
    int rc = check_custom(curve, 2, {"not a user-defined curve id (curve25519 has ellgpu_x25519_ladder and ellgpu_x25519_derive)",
                                     "not a user-defined Montgomery curve (ellgpu_curve_define_mont)", nullptr, nullptr});
    if (rc) return rc;
    const bool v = op == OP_MONTC_VALIDATE;        // (k and out_x unused: absent operands)
    if (n && (!x || !out_flag || (!v && (!k || !out_x)))) return fail(E_ARG, "null pointer");
    CustomScope sc(this, curve, true);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{v ? nullptr : k, 32}, In{x, 32}}, {Out{v ? nullptr : out_x, 32}, Out{out_flag, 1}},
                 [&](size_t m, auto d, auto r) { return montc_chunk(op, m, d[0], d[1], r[0], r[1]); });
  }

  // ---- the key side of user-defined Edwards curves (ellgpu_custom_ed_*) --------------------------
  // pointFromX / pointFromY, decodePoint, KeyPair#validate, KeyPair#derive and BasePoint#encode on a
  // define_edwards id (edckey.h).  A preset or unknown id is an argument error, a short or
  // Montgomery user-defined id is unsupported.  Every call runs under CustomScope's ed_key form: on
  // the curve's augmented block, which the other calls never see.
  // p.byteLength() of the Edwards curve of the call in progress: from the augmented copy (the registered block's is zero)
  int custom_ed_pbytes() const { return (int)custom_aug_[(size_t)(custom_curve_ - CURVE_CUSTOM0)].pbytes; }
  int check_custom_ed(int curve) {
    return check_custom(curve, 1, {"not a user-defined curve id (ed25519 has ellgpu_decompress, ellgpu_decode_points, ellgpu_validate and ellgpu_ecdh_derive)",
                                   "not a user-defined Edwards curve (ellgpu_curve_define_edwards)", nullptr, nullptr});
  }
  int custom_ed_decompress(Mem where, int curve, size_t n, const u8* v, const u8* odd, int from_y, u8* out_xy, u8* out_status) {
    int rc = check_custom_ed(curve);
    if (rc) return rc;
    if (n && (!v || !odd || !out_xy || !out_status)) return fail(E_ARG, "null pointer");
    CustomScope sc(this, curve, false, true);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{v, 32}, In{odd, 1}}, {Out{out_xy, 64}, Out{out_status, 1}}, [&](size_t m, auto d, auto r) {
      return edk_point_chunk(m, d[0], d[1], from_y ? 1 : 0, 0, r[0], r[1], nullptr);
    });
  }
  // enc_len other than 1 + PL and 1 + 2 PL is no error of the call: every item is then 'Unknown point format'
  int custom_ed_decode_points(Mem where, int curve, size_t n, const u8* enc, size_t enc_len, u8* out_xy, u8* out_status) {
    int rc = check_custom_ed(curve);
    if (rc) return rc;
    if (n && (!enc || !out_xy || !out_status)) return fail(E_ARG, "null pointer");
    if (enc_len == 0) return fail(E_ARG, "enc_len must be positive");
    CustomScope sc(this, curve, false, true);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{enc, enc_len}}, {Out{out_xy, 64}, Out{out_status, 1}}, [&](size_t m, auto d, auto r) {
      return edk_point_chunk(m, d[0], nullptr, 0, enc_len, r[0], r[1], nullptr);
    });
  }
  // order_host: 32 bytes in HOST memory wherever the operands are (a parameter of the call, not a batch operand), or null
  int custom_ed_validate(Mem where, int curve, size_t n, const u8* xy, const u8* order_host, u8* out_status) {
    int rc = check_custom_ed(curve);
    if (rc) return rc;
    if (n && (!xy || !out_status)) return fail(E_ARG, "null pointer");
    CustomScope sc(this, curve, false, true);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{xy, 64}}, {Out{out_status, 1}}, [&](size_t m, auto d, auto r) {
      return edk_validate_chunk(m, d[0], order_host, r[0]);
    });
  }
  // wire: pub is n SEC1 encodings of pub_len bytes (ellgpu_custom_ed_derive_wire), else n x 64 raw coordinates
  int custom_ed_derive(Mem where, int curve, size_t n, const u8* priv, const u8* pub, bool wire, size_t pub_len, u8* out_x,
                       u8* out_status, u8* out_err) {
    int rc = check_custom_derive(check_custom_ed(curve), n, priv, pub, wire, pub_len, out_x, out_status);
    if (rc) return rc;
    CustomScope sc(this, curve, false, true);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{priv, 32}, In{pub, wire ? pub_len : 64}}, {Out{out_x, 32}, Out{out_status, 1}, Out{out_err, 1}},
                 [&](size_t m, auto d, auto o) {
      return edk_derive_chunk(m, d[0], d[1], wire ? pub_len : 0, o[0], o[1], o[2]);
    });
  }
  // rows of 1 + PL (compact) or 1 + 2 PL bytes: the short curve's row writer (Work::rt_encode_point)
  int custom_ed_encode_points(Mem where, int curve, size_t n, const u8* xy, int compact, u8* out_enc) {
    int rc = check_custom_ed(curve);
    if (rc) return rc;
    if (n && (!xy || !out_enc)) return fail(E_ARG, "null pointer");
    CustomScope sc(this, curve, false, true);
    if (sc.rc) return sc.rc;
    const size_t EL = 1 + (compact ? 1 : 2) * (size_t)custom_ed_pbytes();
    return batch(where, n, {In{xy, 64}}, {Out{out_enc, EL}}, [&](size_t m, auto d, auto o) {
      return edk_encode_chunk(m, d[0], compact, o[0]);
    });
  }

  // ---- ECDSA on user-defined Edwards domains (ellgpu_custom_ed_verify, _sign, _sign_det) --------
  // EC#verify and EC#sign over a define_edwards_domain id (edcecdsa.h).  A preset or unknown id is
  // an argument error; a short id, a Montgomery id and an Edwards id without a domain are unsupported.
  int check_custom_ed_domain(int curve) {
    const char* need = "ECDSA on a user-defined Edwards curve needs its domain (ellgpu_curve_define_edwards_domain)";
    return check_custom(curve, 1, {"not a user-defined curve id (the presets have ellgpu_ecdsa_verify and ellgpu_ecdsa_sign)",
                                   need, nullptr, need});
  }
  int custom_ed_verify(Mem where, int curve, size_t n, const u8* hash, int hash_len, int msg_bits, const u8* r,
                       const u8* s, const u8* pub, u8* ok, u8* st) {
    int shift;
    int rc = check_custom_ed_domain(curve);
    if (rc) return rc;
    if (n && (!hash || !r || !s || !pub || !ok)) return fail(E_ARG, "null pointer");
    if (hash_len < 1 || hash_len > 64) return fail(E_ARG, "hash_len must be 1 .. 64");
    rc = truncate_shift(hash_len, msg_bits, (int)custom_[(size_t)(curve - CURVE_CUSTOM0)].nbits, 8, shift);
    if (rc) return rc;
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{hash, (size_t)hash_len}, In{r, 32}, In{s, 32}, In{pub, 64}}, {Out{ok, 1}, Out{st, 1}},
                 [&](size_t m, auto d, auto o) {
      if ((rc = ensure_ed_gtable())) return rc;
      return edc_verify_chunk(m, d[0], hash_len, shift, d[1], d[2], d[3], o[0], o[1]);
    });
  }
  // the argument list and semantics of custom_sign on a short domain
  int custom_ed_sign(Mem where, int curve, size_t n, const u8* hash, int hash_len, int msg_bits, const u8* priv,
                     const u8* nonces, bool det, int drbg_hash, int canonical, u8* out_r, u8* out_s,
                     u8* out_recid, u8* out_ok) {
    int shift;
    int rc = check_custom_sign(check_custom_ed_domain(curve), curve, n, hash, hash_len, msg_bits, priv, nonces, det,
                               drbg_hash, out_r, out_s, out_recid, out_ok, shift);
    if (rc) return rc;
    CustomScope sc(this, curve);
    if (sc.rc) return sc.rc;
    return batch(where, n, {In{hash, (size_t)hash_len}, In{priv, 32}, In{det ? nullptr : nonces, 32}},
                 {Out{out_r, 32}, Out{out_s, 32}, Out{out_recid, 1}, Out{out_ok, 1}}, [&](size_t m, auto d, auto o) {
      if ((rc = ensure_ed_gtable())) return rc;
      return edc_sign_chunk(m, d[0], hash_len, shift, d[1], d[2], drbg_hash, canonical, o[0], o[1], o[2], o[3]);
    });
  }

  // scratch arena of the current call (0 / 1: the compute lanes of pipelined(); a device-pointer
  // call takes the lane of its stream, HipBackend::use_stream_dev)
  void set_lane(int l) { lane_ = l & 1; }
  int reserve(int curve, size_t n) {
    // run a dummy-sized allocation pass by touching the arena the way a verify /
    // mul_add2 batch of n items would
    const CurveInfo* ci = curve_info(curve);
    if (!ci) return fail(E_ARG, "unknown curve id");
    int rc = prepare_curve(curve);
    if (rc) return rc;
    size_t m = n < CHUNK ? n : CHUNK;
    size_t L = (size_t)(ci->field_bytes + 3) / 4 + 1;       // +1: the 29-bit secp256k1 field stores 9 limbs
    size_t ent = (curve == CURVE_ED25519) ? 16 * 4 * L * 4 : 32 * 3 * L * 4;
    // both lanes: a caller that alternates two streams works in both arenas
    for (int l = 0; l < 2 && rc == E_OK; l++) {
      lane_ = l;
      claim<void>(S_TBL, m * ent);
      claim<void>(S_JAC, m * 4 * L * 4);
      claim<void>(S_PRE, m * L * 4);
      claim<void>(S_U12, m * 2 * L * 4);
      claim<void>(S_VALID, m);
      rc = claimed();
    }
    lane_ = 0;
    return rc;
  }

 private:
  // (indexed by preset id, and by user-defined id for the combs of ECDSA domains: comb_idx)
  static constexpr int COMB_SLOTS = CURVE_CUSTOM0 + CURVE_CUSTOM_MAX;
  void* comb_[COMB_SLOTS];                   // entry 0 of the fixed-base table (the slot in front of it: its geometry)
  void* comb_base_[COMB_SLOTS];              // what was allocated
  int comb_bits_[COMB_SLOTS];                // window width in use (signed combs may be narrower than the default)
  std::vector<BaseRec> bases_;               // the live caller-chosen bases (define_base), at most BASE_MAX
  int next_base_ = 0;                        // handles are never reused
  Buf scratch_[2][S_COUNT];   // one scratch arena per compute lane (see pipelined())
  int lane_ = 0;
  bool claim_failed_ = false;   // a claim() since the last claimed() got no memory
  Buf staging_[2 * STAGED_MAX];   // the host-buffer calls' device copies: inputs, then outputs (stage())
  std::vector<RtField> custom_;  // user-defined curves of this context (id = CURVE_CUSTOM0 + index)
  std::vector<RtPmodN> custom_pmn_;  // p mod n of each (zero for a curve without a domain): rt_recover_prep's argument
  std::vector<RtField> custom_aug_;  // an Edwards curve's block with Red#sqrt's constants and pbytes (else a plain copy)
  bool custom_active_ = false;
  int custom_curve_ = 0;         // the user-defined curve of the call in progress (CustomScope)
  size_t pipe_step_ = pipe_step_default();   // chunks after the first, in quanta
};

// ---- out-of-class definitions of the per-(curve, operation) members: NOT inline, so that
// `extern template` (engine_extern.h) really keeps their kernels out of other TUs ----
template <class BK>
template <class CV>
int Engine<BK>::ensure_comb() {
  typedef Work<CV> W;
  if (comb_[comb_idx<CV>()]) return E_OK;
  CombTable t;
  const int rc = build_comb<CV>(W::COMB_BITS, true, false, [&](size_t m, size_t first, u8* dk, u8* dp, int cb) {
    FnCombGen<CV> g{m, first, dk, dp, cb};
    bk.launch(g, m);
  }, t);
  if (rc) return rc;
  comb_[comb_idx<CV>()] = t.comb;
  comb_base_[comb_idx<CV>()] = t.base;
  comb_bits_[comb_idx<CV>()] = t.bits;
  return E_OK;
}

template <class BK>
template <class CV, class Gen>
int Engine<BK>::build_comb(int cb, bool narrow, bool check_inf, Gen gen, CombTable& out) {
  typedef Work<CV> W;
  // (a domain's entries come from the user-defined curves' own ladder: the same field and points,
  // no second instantiation of it)
  typedef typename std::conditional<CV::RT_ORDER, CvCustom, CV>::type CVL;
  // When the device cannot hold a SIGNED comb (the 256-bit curves: 12 windows x 2^21 entries =
  // 1.6 GB at the default 22 bits), or the window-table scratch of its build, the SAME kernels run
  // on a narrower one, whose header slot tells them so: 16 bits (17 windows, 36 MB), 12, 8, 4.
  for (;;) {
    const TablePlan plan{comb_entries<CV>(cb), sizeof(typename W::A), (size_t)W::BYTES, cb, true, true, check_inf};
    const int rc = build_table(plan, [&](size_t m, size_t first, u8* dk, u8* dp) { gen(m, first, dk, dp, cb); },
                               [&](size_t m, const u8* dk, const u8* dp, u8* out_xy, u8* out_inf, void* dst) {
      return mul_var_chunk<CVL>(m, dk, dp, out_xy, out_inf, (typename W::A*)dst);
    }, out);
    if (rc != E_NOMEM) return rc;
    if (!narrow || !W::COMB_SIGNED || cb <= 4) return fail(E_NOMEM, "comb table allocation failed");
    err.clear();
    cb = cb > 16 ? 16 : (cb > 12 ? 12 : (cb > 8 ? 8 : 4));
  }
}

template <class BK>
template <class CV>
int Engine<BK>::base_table(const u8* xy, int window_bits, CombTable& out) {
  typedef Work<CV> W;
  int rc = E_OK;
  u8* dpt = checked_base<FnBaseCheck<CV>>(xy, W::BYTES, true, rc);
  if (!dpt) return rc;
  // 0: 16 bits (36 MB, 17 additions per item) -- not G's 22 (1.6 GB): a caller may hold 16 bases
  const int dflt = W::COMB_SIGNED ? (W::COMB_BITS < 16 ? W::COMB_BITS : 16) : W::COMB_BITS;
  rc = build_comb<CV>(window_bits ? window_bits : dflt, window_bits == 0, CV::RT_ORDER,
                      [&](size_t m, size_t first, u8* dk, u8* dp, int cb) {
    FnBaseCombGen<CV> g{m, first, dpt, dk, dp, cb};
    bk.launch(g, m);
  }, out);
  bk.free_(dpt);
  return rc;
}


template <class BK>
template <class CV>
int Engine<BK>::normalize_chunk(size_t n, const u32* jac, u8* out_xy, u8* out_inf, typename Work<CV>::A* raw) {
  typedef Work<CV> W;
  u32* pre = claim<u32>(S_PRE, n * W::NS * 4);
  if (int rc = claimed()) return rc;
  return launch_inv<Route::here, FnNormalize<CV>>(field_inv(n), n, jac, pre, out_xy, out_inf, raw);
}


template <class BK>
template <class CV>
int Engine<BK>::mul_var_chunk(size_t n, const u8* k, const u8* xy, u8* out_xy, u8* out_inf,
                  typename Work<CV>::A* raw) {
  typedef Work<CV> W;
  const Form form = form_for<CV>(n);
  // the window-table scratch is sized by the tuning that is launched (the small-grid tuning's
  // 5-bit windows take twice the slots per item of the full-grid tuning's); the parted form has a
  // table and a result per half
  const size_t slots = form != Form::FULL ? (size_t)W::template stride<true>() : (size_t)W::template stride<false>();
  const size_t halves = parted(form) ? 2 : 1;
  auto* tbl = claim<typename W::VT>(S_TBL, halves * n * slots * sizeof(typename W::VT));
  u32* jac = claim<u32>(S_JAC, halves * n * 3 * W::NS * 4);
  if (int rc = claimed()) return rc;
  bool launched = false;
  if constexpr (CV::ENDO && W::L <= 8) {
    if (parted(form)) {                     // most SIMDs would idle: the halves of every item apart, then the join
      launch_mul_parts<CV>(form, n, k, xy, tbl, jac, nullptr);
      FnMulJoin<CV> fj{n, jac, false, xy, out_xy, out_inf, raw};   // ... to affine, and the domain test
      return launch_fn(fj, n);
    } else if (form == Form::WIDE) {        // at most three waves per SIMD: the register-rich tuning
      FnMulVar<CV, 3, true> f{n, k, xy, tbl, jac};
      launch_fn(f, n);
      launched = true;
    }
  }
  if constexpr (!CV::ENDO && CoopNist<CV>::AVAILABLE) {
    // a handful of items: the ladder of every item on a wave of its own (the row layer); the
    // normalisation and the domain test below are the one-lane kernels'
    if (n <= coop_grid_of<CV>() && out_inf) {
      FnMulPartsN<CV> fc{n, k, xy, jac, nullptr, nullptr};
      bk.launch_coop(fc, n);
      launched = true;
    }
  }
  if (!launched) launch_paired<FnMulVar, CV>(n, k, xy, tbl, jac);
  int rc = normalize_chunk<CV>(n, jac, out_xy, out_inf, raw);
  if (rc == E_OK && out_inf) {                  // (the comb build has no out_inf: its points are G)
    FnDomainMark<CV> g{n, xy, nullptr, out_xy, out_inf};
    bk.launch(g, n);
  }
  return rc;
}


template <class BK>
template <class CV>
int Engine<BK>::mul_fixed_chunk(size_t n, const u8* k, const typename Work<CV>::A* comb, const u8* k2,
                                const typename Work<CV>::A* t2, u8* out_xy, u8* out_inf) {
  typedef Work<CV> W;
  // a handful of items: the comb and the item's own inversion on a wave, one launch (the scalar is
  // Point#mul's: BYTES bytes as they stand -- coop_sign_point<CW, false>, no _truncateToN)
  constexpr bool row_k256 = CV::ENDO && W::L <= 8 && CoopK256::AVAILABLE;
  constexpr bool row_nist = !CV::ENDO && CoopNist<CV>::AVAILABLE;
  if constexpr ((row_k256 || row_nist) && W::NBYTES == W::BYTES) {
    if (!k2 && n <= coop_grid_of<CV>() && out_inf) {
      typedef typename std::conditional<row_k256, CoopK256, CoopNist<CV>>::type CW;
      FnMulFixedC<CV, CW> fc{n, k, comb, out_xy, out_inf};
      bk.launch_coop(fc, n);
      return E_OK;
    }
  }
  u32* jac = claim<u32>(S_JAC, n * 3 * W::NS * 4);
  if (int rc = claimed()) return rc;
  // (two tables: one item per lane at every n, and one normalisation for the sum)
  if (k2) launch_paired<FnMulBase2, CV>(n, k, comb, k2, t2, jac);
  else launch_paired<FnMulFixed, CV>(n, k, comb, jac);
  return normalize_chunk<CV>(n, jac, out_xy, out_inf, nullptr);
}



template <class BK>
template <class CV>
int Engine<BK>::mul_add2_chunk(size_t n, const u8* k1, const u8* xy1, const u8* k2, const u8* xy2,
                   u8* out_xy, u8* out_inf) {
  typedef Work<CV> W;
  u32* jac = claim<u32>(S_JAC, n * 3 * W::NS * 4);
  auto* tbl = claim<typename W::J>(S_TBL, n * 2 * W::TBLJ * sizeof(typename W::J));
  if (int rc = claimed()) return rc;
  FnMulAdd2<CV> f{n, k1, xy1, k2, xy2, tbl, jac};
  bk.launch(f, n);
  int rc = normalize_chunk<CV>(n, jac, out_xy, out_inf, nullptr);
  if (rc == E_OK && out_inf) {
    FnDomainMark<CV> g{n, xy1, xy2, out_xy, out_inf};
    bk.launch(g, n);
  }
  return rc;
}

// Scratch: never more Jacobian entries or window tables than mul_add2_chunk claims for CHUNK items.
// S_JAC holds three runs of planes -- the pairs' (at most `cap` entries), the slices' partial sums
// (nsl entries, none when every sum is whole) and the compact results (n) -- and S_VALID the flags
// of the same entries, a byte each; S_TBL the pairs' window tables.
template <class BK>
template <class CV>
int Engine<BK>::sum_chunk(size_t n, size_t m, const u8* k, const u8* xy, u8* out_xy, u8* out_inf) {
  typedef Work<CV> W;
  const size_t P = m / 2 + (m & 1);
  const bool whole = n <= sum_group_max(m);
  size_t s = P, nsl = 0;                  // pairs per launch and row; slices of the one sum
  if (!whole) {
    if (n != 1) return fail(E_ARG, "a sum that is walked in slices is a chunk of its own");
    s = tune_.sum_slice;
    nsl = (P - 1) / s + 1;
    if (s + nsl + 1 > CHUNK) {            // the slices' partial sums and the result share the pairs' scratch
      s = CHUNK / 2;
      nsl = (P - 1) / s + 1;
    }
    if (nsl + 1 > CHUNK / 2) return fail(E_ARG, "m: too many terms for one sum");
  }
  const size_t cap = whole ? n * P : s;
  const size_t E = 3 * (size_t)W::NS;       // words of a Jacobian entry
  u32* jac = claim<u32>(S_JAC, (cap + nsl + n) * E * 4);
  auto* tbl = claim<typename W::J>(S_TBL, cap * 2 * W::TBLJ * sizeof(typename W::J));
  u8* flag = claim<u8>(S_VALID, cap + nsl + n);
  if (int rc = claimed()) return rc;
  u32* pjac = jac + cap * E;
  u8* pflag = flag + cap;
  u32* cjac = pjac + nsl * E;
  u8* cflag = pflag + nsl;
  // the halving steps of `rows` rows of `len` partial sums; the last one (the copy step of a row
  // that starts with one partial) writes entry d0 + row of the dn-entry planes dst / dflag
  auto fold = [&](size_t rows, size_t len, u32* src, u8* sflag, u32* dst, u8* dflag, size_t dn, size_t d0) {
    const size_t stride = len;
    for (;; len = (len + 1) / 2) {
      FnSumFold<CV> f{rows, stride, len, src, sflag, dst, dflag, dn, d0};
      bk.launch(f, rows * ((len + 1) / 2));
      if (len <= 2) break;
    }
  };
  if (whole) {
    FnSumPairs<CV> f{n, P, m, 0, k, xy, tbl, jac, flag};
    bk.launch(f, n * P);
    fold(n, P, jac, flag, cjac, cflag, n, 0);
  } else {
    for (size_t sl = 0; sl < nsl; sl++) {
      const size_t q0 = sl * s, len = P - q0 < s ? P - q0 : s;
      FnSumPairs<CV> f{1, len, m, q0, k, xy, tbl, jac, flag};
      bk.launch(f, len);
      fold(1, len, jac, flag, pjac, pflag, nsl, sl);
    }
    fold(1, nsl, pjac, pflag, cjac, cflag, 1, 0);
  }
  int rc = normalize_chunk<CV>(n, cjac, out_xy, out_inf, nullptr);
  if (rc) return rc;
  FnSumMark<CV> g{n, cflag, out_xy, out_inf};
  bk.launch(g, n);
  return E_OK;
}

template <class BK>
template <class CV>
int Engine<BK>::mul_add_g_chunk(size_t n, const u8* k1, const u8* k2, const u8* xy2, u8* out_xy,
                    u8* out_inf) {
  typedef Work<CV> W;
  if constexpr (CV::ENDO && W::L <= 8) {
    const Form form = form_for<CV>(n);
    // (k1*G + k2*P has no WIDE kernel: a wide batch that is not parted runs the ordinary mul_add_g below)
    if (parted(form)) {                     // most SIMDs would idle: k2's halves and k1's comb apart, then the join
      u32* pj = claim<u32>(S_JAC, 3 * n * 3 * W::NS * 4);
      auto* pt = claim<typename W::VT>(S_TBL, 2 * n * (size_t)W::template stride<true>() * sizeof(typename W::VT));
      if (int rc = claimed()) return rc;
      launch_mul_parts<CV>(form, n, k2, xy2, pt, pj, k1);
      FnMulJoin<CV> fj{n, pj, true, xy2, out_xy, out_inf, nullptr};
      return launch_fn(fj, n);
    }
  }
  if constexpr (!CV::ENDO && CoopNist<CV>::AVAILABLE) {
    if (n <= coop_grid_of<CV>()) {                 // the ladder of k2 and the comb of k1 on a wave each, joined on one lane
      u32* pj = claim<u32>(S_JAC, 2 * n * 3 * W::NS * 4);
      if (int rc = claimed()) return rc;
      FnMulPartsN<CV> fc{n, k2, xy2, pj, k1, comb_of<CV>()};
      bk.launch_coop(fc, 2 * n);
      FnMulJoin<CV> fj{n, pj, false, xy2, out_xy, out_inf, nullptr};
      return launch_fn(fj, n);
    }
  }
  u32* jac = claim<u32>(S_JAC, n * 3 * W::NS * 4);
  auto* tbl = claim<typename W::VT>(S_TBL, n * (size_t)W::template stride<false>() * sizeof(typename W::VT));
  if (int rc = claimed()) return rc;
  launch_paired<FnMulAddG, CV>(n, k1, k2, xy2, comb_of<CV>(), tbl, jac);
  int rc = normalize_chunk<CV>(n, jac, out_xy, out_inf, nullptr);
  if (rc == E_OK && out_inf) {
    FnDomainMark<CV> g{n, nullptr, xy2, out_xy, out_inf};
    bk.launch(g, n);
  }
  return rc;
}


template <class BK>
template <int U>
int Engine<BK>::rt_wire_chunk(int op, size_t n, const u8* a, const u8* b, size_t len, const u32* lens, u8* o1,
                              u8* o2, u8* o3) {
  if (op == OP_RT_DECOMPRESS) {
    FnRtDecompress f{n, a, b, o1, o2};
    bk.launch(f, n);
  } else if (op == OP_RT_DECODE) {
    FnRtDecodePoint f{n, a, len, (int)custom_[(size_t)(custom_curve_ - CURVE_CUSTOM0)].pbytes, o1, o2};
    bk.launch(f, n);
  } else if (op == OP_RT_FROM_DER) {
    FnSigFromDer<CvCustom> f{n, a, len, lens, o1, o2, o3};
    bk.launch(f, n);
  } else {
    FnWireStatus<CvCustom> f{n, a, b, o3, o1, o2};
    bk.launch(f, n);
  }
  return E_OK;
}

template <class BK>
template <int U>
int Engine<BK>::rt_encode_chunk(size_t n, const u8* xy, int compact, u8* out_enc) {
  FnRtEncodePoint f{n, xy, compact, custom_pbytes(), out_enc};
  bk.launch(f, n);
  return E_OK;
}

template <class BK>
template <int U>
int Engine<BK>::rt_ecdh_ladder(size_t n, const u8* k, const u8* pub, size_t len, bool ladder, u8*& flags, u32*& jac) {
  typedef Work<CvCustom> W;
  // the points, the order as scalars and the flags live across the ladder kernel, which uses
  // S_TBL / S_JAC only (as in rt_recover_chunk)
  flags = claim<u8>(S_VALID, 2 * n);
  u8* pts = nullptr;
  u8* scal = nullptr;
  typename W::VT* tbl = nullptr;
  jac = nullptr;
  if (ladder) {
    pts = claim<u8>(S_U12, n * (size_t)(k ? 64 : 96));
    tbl = claim<typename W::VT>(S_TBL, n * (size_t)W::template stride<false>() * sizeof(typename W::VT));
    jac = claim<u32>(S_JAC, n * 3 * W::NS * 4);
  }
  if (int rc = claimed()) return rc;
  if (ladder && !k) scal = pts + n * 64;
  FnRtEcdhFront f0{n, pub, len, custom_pbytes(), pts, flags + n, flags, scal};
  bk.launch(f0, n);
  if (ladder) launch_paired<FnMulVar, CvCustom>(n, k ? k : (const u8*)scal, (const u8*)pts, tbl, jac);   // form_for<CvCustom>: FULL
  return E_OK;
}

template <class BK>
template <int U>
int Engine<BK>::rt_derive_chunk(size_t n, const u8* k, const u8* pub, size_t len, u8* out_x, u8* status, u8* err) {
  typedef Work<CvCustom> W;
  u8* flags;
  u32* jac;
  int rc = rt_ecdh_ladder(n, k, pub, len, true, flags, jac);
  if (rc) return rc;
  u32* pre = claim<u32>(S_PRE, n * W::NS * 4);
  if ((rc = claimed())) return rc;
  return launch_inv<Route::here, FnRtDeriveFinish>(field_inv(n), n, jac, flags + n, flags, pre, out_x, status, err);
}

template <class BK>
template <int U>
int Engine<BK>::rt_validate_chunk(size_t n, const u8* xy, const u8* inf, bool check_order, u8* status) {
  u8* flags;
  u32* jac;
  int rc = rt_ecdh_ladder(n, nullptr, xy, 0, check_order, flags, jac);
  if (rc) return rc;
  FnRtValidateFold f2{n, inf, flags, jac, status};
  bk.launch(f2, n);
  return E_OK;
}

template <class BK>
template <int U>
int Engine<BK>::rt_recover_chunk(size_t n, const u8* hash, int hash_len, const u8* r, const u8* s,
                                 const u8* recid, u8* out_xy, u8* out_status) {
  typedef Work<CvCustomDomain> W;
  // the scalars, the x-coordinates and the points R live across the ladder kernels, which use
  // S_TBL / S_JAC / S_PRE only (as in recover_chunk)
  u8* buf = claim<u8>(S_U12, n * (2 * 32 + 3 * 32));
  u8* flags = claim<u8>(S_VALID, 3 * n);
  u32* pre = claim<u32>(S_PRE, n * W::LN * 4);
  if (int rc = claimed()) return rc;
  u8* s1 = buf;
  u8* s2 = s1 + n * 32;
  u8* xs = s2 + n * 32;
  u8* rxy = xs + n * 32;
  u8* odd = flags;
  u8* dec_st = flags + n;
  u8* inf = flags + 2 * n;
  launch_inv<Route::here, FnRtRecoverPrep>(scalar_inv(n), n, custom_pmn_[(size_t)(custom_curve_ - CURVE_CUSTOM0)], hash,
                                           hash_len, r, s, recid, pre, xs, odd, s1, s2, out_status);
  int rc = rt_wire_chunk(OP_RT_DECOMPRESS, n, xs, odd, 0, nullptr, rxy, dec_st, nullptr);
  if (rc) return rc;
  rc = mul_add_g_chunk<CvCustomDomain>(n, s1, s2, rxy, out_xy, inf);           // s1 * G + s2 * R
  if (rc) return rc;
  FnRtRecoverFinish f2{n, dec_st, inf, out_xy, out_status};
  bk.launch(f2, n);
  return E_OK;
}

template <class BK>
template <int U>
int Engine<BK>::rt_sign_chunk(size_t n, const u8* hash, int hash_len, int shift, const u8* priv,
                              const u8* nonces, int drbg_hash, int canonical, u8* out_r, u8* out_s,
                              u8* out_recid, u8* out_ok) {
  typedef Work<CvCustomDomain> W;
  u32* jac = claim<u32>(S_JAC, n * 3 * W::NS * 4);
  u8* kg = claim<u8>(S_U12, n * (2 * W::BYTES + 1));             // k*G affine + infinity flags
  u8* drawn = nonces ? nullptr : claim<u8>(S_TBL, n * W::NBYTES);   // the passes below use S_JAC / S_U12 / S_PRE
  if (int rc = claimed()) return rc;
  u8* kg_inf = kg + n * 2 * W::BYTES;
  if (!nonces) {
    draw_nonces(drbg_hash, n, hash, hash_len, shift, priv, drawn);   // (group 17 is this body's own unit too)
    nonces = drawn;
  }
  FnRtSignMul f1{n, nonces, comb_of<CvCustomDomain>(), jac};
  bk.launch(f1, n);
  int rc = normalize_chunk<CvCustomDomain>(n, jac, kg, kg_inf, nullptr);
  if (rc) return rc;
  u32* pre = claim<u32>(S_PRE, n * (W::LN > W::NS ? W::LN : W::NS) * 4);
  if ((rc = claimed())) return rc;
  return launch_inv<Route::here, FnRtSignFinish>(scalar_inv(n), n, hash, hash_len, shift, priv, nonces, kg, kg_inf,
                                                 canonical, pre, out_r, out_s, out_recid, out_ok);
}

template <class BK>
template <int U>
int Engine<BK>::edc_chunk(int op, size_t n, const u8* k1, const u8* xy1, const u8* k2, const u8* xy2,
                          const u8* a, const u8* b, u8* out_xy, u8* out_inf) {
  u32* proj = claim<u32>(S_JAC, n * 3 * 8 * 4);
  u32* pre = claim<u32>(S_PRE, n * 8 * 4);
  auto* tbl = claim<EdcWork::P>(S_TBL, n * 16 * sizeof(EdcWork::P));
  if (int rc = claimed()) return rc;
  if (op == 0) {
    FnEdcMulVar f{n, k1, xy1, tbl, proj};
    bk.launch(f, n);
  } else if (op == 1) {
    FnEdcMulAdd2 f{n, k1, xy1, k2, xy2, tbl, proj};
    bk.launch(f, n);
  } else {
    FnEdcPointAdd f{n, xy1, a, xy2, b, proj};
    bk.launch(f, n);
  }
  launch_inv<Route::here, FnEdcNormalize>(field_inv(n), n, proj, pre, out_xy, out_inf);
  if (op != 2 && out_inf) {                       // Point#add is one formula: the reference's own
    FnEdcDomainMark h{n, xy1, op == 1 ? xy2 : nullptr, out_xy, out_inf};
    bk.launch(h, n);
  }
  return E_OK;
}

template <class BK>
template <int U>
int Engine<BK>::montc_chunk(int op, size_t n, const u8* k, const u8* x, u8* out_x, u8* out_flag) {
  if (op == OP_MONTC_VALIDATE) {
    FnMontcValidate fv{n, x, out_flag};
    bk.launch(fv, n);
    return E_OK;
  }
  u32* xz = claim<u32>(S_JAC, n * 2 * 8 * 4);
  u32* pre = claim<u32>(S_PRE, n * 8 * 4);
  u8* vst = op == OP_MONTC_DERIVE ? claim<u8>(S_VALID, n) : nullptr;
  if (int rc = claimed()) return rc;
  if (vst) {
    FnMontcValidate fv{n, x, vst};
    bk.launch(fv, n);
  }
  FnMontcLadder f{n, k, x, xz};
  bk.launch(f, n);
  return launch_inv<Route::here, FnMontcNormalize>(field_inv(n), n, xz, pre, vst, out_x, out_flag);
}

template <class BK>
template <int U>
int Engine<BK>::edk_point_chunk(size_t n, const u8* a, const u8* b, int from_y, size_t len, u8* out_xy, u8* out_st,
                                u8* valid) {
  // the point under construction, the decoder's status and what the root pass owes each item live
  // across the three passes; out_xy == null: the finished point stays in S_U12 for the ladder
  u8* pts = claim<u8>(S_U12, n * 64);
  u8* flags = claim<u8>(S_VALID, 3 * n);
  u32* nd = claim<u32>(S_PRE, n * 24 * 4);                       // numerator, denominator, prefix products
  if (int rc = claimed()) return rc;
  edk_point_passes(n, a, b, from_y, len, pts, flags, nd, out_xy, out_st, valid);
  return E_OK;
}

template <class BK>
template <int U>
void Engine<BK>::edk_point_passes(size_t n, const u8* a, const u8* b, int from_y, size_t len, u8* pts, u8* flags,
                                  u32* nd, u8* out_xy, u8* out_st, u8* valid) {
  u8* st = flags;
  u8* need = flags + n;
  u32* pre = nd + n * 16;
  if (len) {
    FnEdcKeyFrontEnc f{n, a, len, custom_ed_pbytes(), pts, st, need, nd};
    bk.launch(f, n);
  } else {
    FnEdcKeyFrontCoord f{n, a, b, from_y, pts, st, need, nd};
    bk.launch(f, n);
  }
  launch_inv<Route::here, FnEdcKeyQuotient>(field_inv(n), n, nd, pre);
  FnEdcKeyRoot r{n, nd, pts, st, need, out_xy ? out_xy : pts, out_st, valid};
  bk.launch(r, n);
}

template <class BK>
template <int U>
int Engine<BK>::edk_derive_chunk(size_t n, const u8* k, const u8* pub, size_t len, u8* out_x, u8* status, u8* err) {
  u8* pts = claim<u8>(S_U12, n * 64);
  u8* flags = claim<u8>(S_VALID, 3 * n);
  u32* pre = claim<u32>(S_PRE, n * 24 * 4);
  u32* proj = claim<u32>(S_JAC, n * 3 * 8 * 4);
  auto* tbl = claim<EdcWork::P>(S_TBL, n * 8 * sizeof(EdcWork::P));
  if (int rc = claimed()) return rc;
  u8* dec_st = flags;
  u8* valid = flags + 2 * n;
  if (len) {                                    // decodePoint into pts, in the buffers held here
    edk_point_passes(n, pub, nullptr, 0, len, pts, flags, pre, nullptr, dec_st, valid);
  } else {
    FnEdcKeyFrontXy f0{n, pub, pts, valid, nullptr, nullptr, EdcKey::Scalar{}};
    bk.launch(f0, n);
  }
  FnEdcMulVar lad{n, k, pts, tbl, proj};
  bk.launch(lad, n);
  return launch_inv<Route::here, FnEdcKeyDeriveFinish>(field_inv(n), n, proj, len ? dec_st : nullptr, valid, pre, out_x,
                                                       status, err);
}

template <class BK>
template <int U>
int Engine<BK>::edk_encode_chunk(size_t n, const u8* xy, int compact, u8* out_enc) {
  FnRtEncodePoint f{n, xy, compact, custom_ed_pbytes(), out_enc};        // the short curve's row writer
  bk.launch(f, n);
  return E_OK;
}

template <class BK>
template <int U>
int Engine<BK>::edk_validate_chunk(size_t n, const u8* xy, const u8* order, u8* status) {
  u8* flags = claim<u8>(S_VALID, 3 * n);
  u8* pts = nullptr;
  u8* scal = nullptr;
  u32* proj = nullptr;
  EdcWork::P* tbl = nullptr;
  EdcKey::Scalar ord{};
  if (order) {
    pts = claim<u8>(S_U12, n * 96);                              // the points, then `order` once per item
    proj = claim<u32>(S_JAC, n * 3 * 8 * 4);
    tbl = claim<EdcWork::P>(S_TBL, n * 8 * sizeof(EdcWork::P));
  }
  if (int rc = claimed()) return rc;
  if (order) {
    scal = pts + n * 64;
    memcpy(ord.b, order, 32);
  }
  FnEdcKeyFrontXy f0{n, xy, pts, flags + 2 * n, flags, scal, ord};
  bk.launch(f0, n);
  if (order) {
    FnEdcMulVar lad{n, scal, pts, tbl, proj};                     // the ladder of Point#mul, one scalar for all
    bk.launch(lad, n);
  }
  FnEdcKeyValidateFold f2{n, flags, flags + 2 * n, proj, status};
  bk.launch(f2, n);
  return E_OK;
}

// G .. 8G of the Edwards domain of the call in progress, in the slot a short domain's comb would
// take (comb_idx): built on the device on first use.  Its 512 bytes are NOT counted against
// ELLGPU_COMB_MAX_BYTES: that limit makes a comb fall back to a narrower one, and this table has no
// narrower form -- under the limit the calls would only fail.  comb_bits_ stays 0: the slot holds no comb.
template <class BK>
template <int U>
int Engine<BK>::ensure_ed_gtable() {
  const int idx = custom_curve_;
  if (comb_[idx]) return E_OK;
  u32* gt = (u32*)bk.alloc(EdcEcdsa::GT_WORDS * sizeof(u32));
  if (!gt) return fail(E_NOMEM, "generator table allocation failed");
  FnEdcEcdsaGTable f{gt};
  bk.launch(f, 1);
  const int src = bk.sync();
  if (src != E_OK) {
    bk.free_(gt);
    return fail(src, "building the generator table failed on the device");
  }
  comb_[idx] = gt;
  comb_base_[idx] = gt;
  return E_OK;
}

template <class BK>
template <int U>
int Engine<BK>::edc_verify_chunk(size_t n, const u8* hash, int hash_len, int shift, const u8* r, const u8* s,
                                 const u8* pub, u8* ok, u8* st) {
  auto* tbl = claim<EdcWork::P>(S_TBL, n * 8 * sizeof(EdcWork::P));
  u32* pre = claim<u32>(S_PRE, n * 8 * 4);
  u32* u12 = claim<u32>(S_U12, n * 2 * 8 * 4);
  u8* flags = claim<u8>(S_VALID, 2 * n);
  u32* proj = claim<u32>(S_JAC, n * 3 * 8 * 4);
  if (int rc = claimed()) return rc;
  u8* valid = flags;
  u8* onc = flags + n;
  const u32* gt = (const u32*)comb_[custom_curve_];
  // the short domain's prep, in its unit (group 17): it reads n from that unit's block
  launch_inv<Route::unit, FnEcdsaPrep<CvCustomDomain>>(scalar_inv(n), n, hash, hash_len, shift, r, s, pre, u12, valid);
  FnEdcEcdsaLadder f2{n, u12, pub, gt, tbl, proj, onc};
  bk.launch(f2, n);
  if (custom_[(size_t)(custom_curve_ - CURVE_CUSTOM0)].ncand != RT_NO_MAXWELL) {
    FnEdcEcdsaEq f3{n, proj, valid, onc, r, ok, st};
    bk.launch(f3, n);
    return E_OK;
  }
  return launch_inv<Route::here, FnEdcEcdsaEqAffine>(field_inv(n), n, proj, valid, onc, r, pre, ok, st);
}

template <class BK>
template <int U>
int Engine<BK>::edc_sign_chunk(size_t n, const u8* hash, int hash_len, int shift, const u8* priv, const u8* nonces,
                               int drbg_hash, int canonical, u8* out_r, u8* out_s, u8* out_recid, u8* out_ok) {
  u32* proj = claim<u32>(S_JAC, n * 3 * 8 * 4);
  u8* kg = claim<u8>(S_U12, n * (64 + 1));                       // k*G affine + infinity flags
  u32* pre = claim<u32>(S_PRE, n * 8 * 4);
  u8* drawn = nonces ? nullptr : claim<u8>(S_TBL, n * 32);
  if (int rc = claimed()) return rc;
  u8* kg_inf = kg + n * 64;
  const u32* gt = (const u32*)comb_[custom_curve_];
  // the nonces and the finish are the short domain's, in its unit (group 17): they read n from that unit's block
  if (!nonces) {
    draw_nonces(drbg_hash, n, hash, hash_len, shift, priv, drawn);
    nonces = drawn;
  }
  FnEdcSignMul f1{n, nonces, gt, proj};
  bk.launch(f1, n);
  launch_inv<Route::here, FnEdcSignNorm>(field_inv(n), n, proj, pre, kg, kg_inf);
  return launch_inv<Route::unit, FnRtSignFinish>(scalar_inv(n), n, hash, hash_len, shift, priv, nonces, kg, kg_inf,
                                                 canonical, pre, out_r, out_s, out_recid, out_ok);
}

template <class BK>
template <class Fn>
int Engine<BK>::launch_fn(const Fn& f, size_t nthreads) {
  bk.launch(f, nthreads);
  return E_OK;
}

template <class BK>
template <class CV>
int Engine<BK>::ecdsa_chunk(size_t n, const u8* hash, int hash_len, int shift, const u8* r, const u8* s,
                const u8* pub, u8* ok, u8* st) {
  typedef Work<CV> W;
  const Form form = form_for<CV>(n);
  const bool wide = form != Form::FULL;
  const size_t slots = wide ? (size_t)W::template stride<true>() : (size_t)W::template stride<false>();
  auto* tbl = claim<typename W::VT>(S_TBL, n * slots * sizeof(typename W::VT));
  u32* pre = claim<u32>(S_PRE, n * (W::LN > W::NS ? W::LN : W::NS) * 4);
  u32* u12 = claim<u32>(S_U12, n * 2 * W::LN * 4);
  u8* valid = claim<u8>(S_VALID, n);
  if (int rc = claimed()) return rc;
  if constexpr (CV::ENDO && W::L <= 8 && ELL_SPLIT_SMALL_VERIFY) {
    // (the two-kernel form on a FULL grid was measured too, round 4: 8.22 -> 8.37 ms per 2^20 --
    // the table kernel alone takes 0.65 ms where building the table inside ecdsa_main costs
    // 0.5 ms, and there is no latency to hide at four waves per SIMD; small grids only)
    // (the verify takes the table and parted forms only under split_small_verify(): without it a
    // wide batch, parted or not, is ecdsa_prep -> the WIDE ecdsa_main below)
    if (wide && split_small_verify()) {
      // latency-bound batch: the window table does not depend on s^-1, so it is built BESIDE
      // ecdsa_prep -- one launch whose first workgroups run the prep and whose others build the
      // tables (FnEcdsaPrepTable); the ladder follows in stream order.  (Round 4 first ran the two
      // as separate kernels on two streams with an event fork / join: 0.6-1.9 % slower than this
      // fused launch, profiles/r04_split_verify_ab.txt.)
      if (form == Form::PARTS_WAVE) {
        // a handful of items: the prep on a wave per item, the table on another (row layer), one launch
        FnEcdsaPrepTableC fptc{n, hash, hash_len, shift, r, s, pre, u12, valid, pub, tbl};
        bk.launch_coop(fptc, 2 * n);
      } else if (form == Form::PARTS_ROW) {
        const size_t pu = (n + 63) / 64;
        FnEcdsaPrepTableR fptr{n, pu, hash, hash_len, shift, r, s, pre, u12, valid, pub, tbl};
        bk.launch_coop(fptr, pu + (n + 3) / 4);
      } else {
        // a geometry of its own, not scalar_inv()'s: the prep shares the launch with the table, so K
        // comes from inv_batch_beside() and the prep's threads are padded to whole workgroups
        const int Ks = inv_batch_beside(n, INV_BATCH_N);
        const size_t Ts = (n + Ks - 1) / Ks;
        const size_t tpad = (Ts + 127) & ~(size_t)127;          // whole workgroups of either kind
        FnEcdsaPrepTable<CV> fpt{{Ts, n, Ks, hash, hash_len, shift, r, s, pre, u12, valid}, tpad, {n, pub, tbl}};
        launch_fn(fpt, tpad + n);
      }
      if (form == Form::WIDE) {
        FnEcdsaLadder<CV, true> fl{n, u12, valid, r, pub, comb_of<CV>(), tbl, ok, st};
        return launch_fn(fl, n);
      }
      // most SIMDs would idle beside this batch: the half ladders and the comb of every item as
      // three parts, then the join
      u32* jac = claim<u32>(S_JAC, n * 3 * 3 * W::NS * 4);
      if (int rc = claimed()) return rc;
      const size_t units = part_units(form, n, 3);
      if (form == Form::PARTS_WAVE) {         // every part on a wave of its own, lanes-per-item arithmetic
        FnEcdsaPartsK256<false> fc{n, u12, comb_of<CV>(), tbl, jac};
        bk.launch_coop(fc, units);
      } else if (form == Form::PARTS_ROW) {   // one item per row, four per wave
        FnEcdsaPartsK256<true> fr{n, u12, comb_of<CV>(), tbl, jac};
        bk.launch_coop(fr, units);
      } else {                                // three lanes per item
        FnEcdsaParts<CV> fp{n, part_pad(n), u12, comb_of<CV>(), tbl, jac};
        launch_fn(fp, units);
      }
      FnEcdsaJoin<CV> fj{n, valid, r, pub, tbl, jac, ok, st};
      return launch_fn(fj, n);
    }
  }
  if constexpr (!CV::ENDO && CoopNist<CV>::AVAILABLE) {
    if (n <= coop_grid_of<CV>()) {
      // a handful of items on a curve without an endomorphism: the scalar-field prep as it is
      // (one inversion per item), then the ladder and the comb of every item on a WAVE each (the
      // row layer, coop_mont.h), and the one-lane join
      typedef CoopNist<CV> CW;
      u32* jac = claim<u32>(S_JAC, n * 2 * 3 * W::NS * 4);
      auto* gt = claim<typename CW::A>(S_TBL, n * CW::TABLE_BYTES);
      if (int rc = claimed()) return rc;
      // the prep on a wave per item, the window table of the key on another, one launch ...
      FnEcdsaPrepTableN<CV> fpt{n, hash, hash_len, shift, r, s, pre, u12, valid, pub, gt};
      bk.launch_coop(fpt, 2 * n);
      // ... then the ladder over that table and the comb
      FnEcdsaPartsN<CV> fc{n, u12, pub, comb_of<CV>(), jac, gt};
      bk.launch_coop(fc, 2 * n);
      FnEcdsaJoin2<CV> fj{n, valid, r, pub, jac, ok, st};
      return launch_fn(fj, n);
    }
  }
  launch_inv<Route::unit, FnEcdsaPrep<CV>>(scalar_inv(n), n, hash, hash_len, shift, r, s, pre, u12, valid);
  if constexpr (CV::ENDO && W::L <= 8) {
    if (wide) {                             // at most three waves per SIMD: the register-rich tuning
      FnEcdsaMain<CV, 3, true> f2{n, u12, valid, r, pub, comb_of<CV>(), tbl, ok, st};
      return launch_fn(f2, n);              // (its own translation unit: engine_extern.h group 7)
    }
  }
  launch_paired<FnEcdsaMain, CV>(n, u12, valid, r, pub, comb_of<CV>(), tbl, ok, st);
  return E_OK;
}

template <class BK>
template <class CV>
int Engine<BK>::ecdsa_base_chunk(size_t n, const u8* hash, int hash_len, int shift, const u8* r, const u8* s,
                                 const typename Work<CV>::A* tg, const typename Work<CV>::A* tq, u8* ok) {
  typedef Work<CV> W;
  u32* pre = claim<u32>(S_PRE, n * (W::LN > W::NS ? W::LN : W::NS) * 4);
  u32* u12 = claim<u32>(S_U12, n * 2 * W::LN * 4);
  u8* valid = claim<u8>(S_VALID, n);
  if (int rc = claimed()) return rc;
  launch_inv<Route::unit, FnEcdsaPrep<CV>>(scalar_inv(n), n, hash, hash_len, shift, r, s, pre, u12, valid);
  launch_paired<FnEcdsaBase, CV>(n, u12, valid, r, tg, tq, ok);
  return E_OK;
}

// ---- Edwards / Montgomery -------------------------------------------------

template <class BK>
template <int U>
int Engine<BK>::ensure_ed_comb() {
  if (comb_[CURVE_ED25519]) return E_OK;
  u32 gx[8], gy[8];
  for (int i = 0; i < 8; i++) { gx[i] = consts::ED25519_C::gx_plain[i]; gy[i] = consts::ED25519_C::gy_plain[i]; }
  u8 g[64];
  store_be<8>(g, gx, 32);
  store_be<8>(g + 32, gy, 32);
  CombTable t;
  const int rc = ed_base_table(g, true, t);
  if (rc) return rc;
  comb_[CURVE_ED25519] = t.comb;
  return E_OK;
}


template <class BK>
template <int U>
int Engine<BK>::ed_normalize_chunk(size_t n, const u32* ext, u8* out_xy, u8* out_inf, EdWork::P* raw) {
  u32* pre = claim<u32>(S_PRE, n * 8 * 4);
  if (int rc = claimed()) return rc;
  return launch_inv<Route::here, FnEdNormalize>(field_inv(n), n, ext, pre, out_xy, out_inf, raw);
}

template <class BK>
template <int U>
int Engine<BK>::ed_mul_var_chunk(size_t n, const u8* k, const u8* xy, u8* out_xy, u8* out_inf, EdWork::P* raw) {
  auto* tbl = claim<EdWork::P>(S_TBL, n * 8 * sizeof(EdWork::P));
  u32* ext = claim<u32>(S_JAC, n * 4 * 8 * 4);
  if (int rc = claimed()) return rc;
  if (n <= coop_grid()) {
    FnEdMulC fc{n, nullptr, nullptr, k, xy, nullptr, ext};
    bk.launch_coop(fc, n);
  } else {
    FnEdMulVar f{n, k, xy, tbl, ext};
    bk.launch(f, n);
  }
  int rc = ed_normalize_chunk(n, ext, out_xy, out_inf, raw);
  if (rc == E_OK && out_inf) {
    FnEdDomainMark g{n, xy, nullptr, out_xy, out_inf};
    bk.launch(g, n);
  }
  return rc;
}

template <class BK>
template <int U>
int Engine<BK>::ed_mul_fixed_chunk(size_t n, const u8* k, u8* out_xy, u8* out_inf) {
  if (n <= coop_grid() && out_xy) {                    // a handful of items: one item per wave, one launch
    FnEdMulFixedC fc{n, k, (const EdWork::P*)comb_[CURVE_ED25519], out_xy, out_inf};
    bk.launch_coop(fc, n);
    return E_OK;
  }
  u32* ext = claim<u32>(S_JAC, n * 4 * 8 * 4);
  if (int rc = claimed()) return rc;
  FnEdMulFixed f{n, k, (const EdWork::P*)comb_[CURVE_ED25519], ext};
  bk.launch(f, n);
  return ed_normalize_chunk(n, ext, out_xy, out_inf, nullptr);
}

template <class BK>
template <int U>
int Engine<BK>::ed_mul_add2_chunk(size_t n, const u8* k1, const u8* xy1, const u8* k2, const u8* xy2,
                      u8* out_xy, u8* out_inf) {
  u32* ext = claim<u32>(S_JAC, n * 4 * 8 * 4);
  auto* tbl = claim<EdWork::P>(S_TBL, n * 16 * sizeof(EdWork::P));
  if (int rc = claimed()) return rc;
  if (n <= coop_grid()) {
    FnEdMulC fc{n, k1, xy1, k2, xy2, (const EdWork::P*)comb_[CURVE_ED25519], ext};
    bk.launch_coop(fc, n);
  } else if (xy1) {
    FnEdMulAdd2 f{n, k1, xy1, k2, xy2, tbl, ext};
    bk.launch(f, n);
  } else {
    FnEdMulAddG f{n, k1, k2, xy2, (const EdWork::P*)comb_[CURVE_ED25519], tbl, ext};
    bk.launch(f, n);
  }
  int rc = ed_normalize_chunk(n, ext, out_xy, out_inf, nullptr);
  if (rc == E_OK && out_inf) {
    FnEdDomainMark g{n, xy1, xy2, out_xy, out_inf};
    bk.launch(g, n);
  }
  return rc;
}

// sum_chunk<CV> over an Edwards work class.  Scratch: never more entries or window tables than that
// family's mul_add2 chunk claims for CHUNK items (ed_mul_add2_chunk: four planes of 8 words per
// item; edc_chunk: three).  S_JAC holds three runs of planes -- the pairs' (at most `cap` entries),
// the slices' partial sums (nsl entries, none when every sum is whole) and the compact results (n)
// -- and S_VALID the flags of the same entries, a byte each; S_TBL the pairs' window tables.
template <class BK>
template <class EW>
int Engine<BK>::ed_sum_chunk(size_t n, size_t m, const u8* k, const u8* xy, u8* out_xy, u8* out_inf) {
  constexpr bool ED = std::is_same<EW, EdWork>::value;
  const size_t P = m / 2 + (m & 1);
  const bool whole = n <= sum_group_max(m);
  size_t s = P, nsl = 0;                  // pairs per launch and row; slices of the one sum
  if (!whole) {
    if (n != 1) return fail(E_ARG, "a sum that is walked in slices is a chunk of its own");
    s = tune_.sum_slice;
    nsl = (P - 1) / s + 1;
    if (s + nsl + 1 > CHUNK) {            // the slices' partial sums and the result share the pairs' scratch
      s = CHUNK / 2;
      nsl = (P - 1) / s + 1;
    }
    if (nsl + 1 > CHUNK / 2) return fail(E_ARG, "m: too many terms for one sum");
  }
  const size_t cap = whole ? n * P : s;
  const size_t E = (size_t)EW::SUM_PLANES * 8;     // words of an entry
  u32* ext = claim<u32>(S_JAC, (cap + nsl + n) * E * 4);
  auto* tbl = claim<typename EW::P>(S_TBL, cap * 16 * sizeof(typename EW::P));
  u8* flag = claim<u8>(S_VALID, cap + nsl + n);
  u32* pre = ED ? nullptr : claim<u32>(S_PRE, n * 8 * 4);      // (ed_normalize_chunk claims its own)
  if (int rc = claimed()) return rc;
  u32* pext = ext + cap * E;
  u8* pflag = flag + cap;
  u32* cext = pext + nsl * E;
  u8* cflag = pflag + nsl;
  // the halving steps of `rows` rows of `len` partial sums; the last one (the copy step of a row
  // that starts with one partial) writes entry d0 + row of the dn-entry planes dst / dflag
  auto fold = [&](size_t rows, size_t len, u32* src, u8* sflag, u32* dst, u8* dflag, size_t dn, size_t d0) {
    const size_t stride = len;
    for (;; len = (len + 1) / 2) {
      FnEdSumFold<EW> f{rows, stride, len, src, sflag, dst, dflag, dn, d0};
      bk.launch(f, rows * ((len + 1) / 2));
      if (len <= 2) break;
    }
  };
  if (whole) {
    FnEdSumPairs<EW> f{n, P, m, 0, k, xy, tbl, ext, flag};
    bk.launch(f, n * P);
    fold(n, P, ext, flag, cext, cflag, n, 0);
  } else {
    for (size_t sl = 0; sl < nsl; sl++) {
      const size_t q0 = sl * s, len = P - q0 < s ? P - q0 : s;
      FnEdSumPairs<EW> f{1, len, m, q0, k, xy, tbl, ext, flag};
      bk.launch(f, len);
      fold(1, len, ext, flag, pext, pflag, nsl, sl);
    }
    fold(1, nsl, pext, pflag, cext, cflag, 1, 0);
  }
  if constexpr (ED) {
    if (int rc = ed_normalize_chunk(n, cext, out_xy, out_inf, nullptr)) return rc;
  } else {
    launch_inv<Route::here, FnEdcNormalize>(field_inv(n), n, cext, pre, out_xy, out_inf);
  }
  FnEdSumMark<EW> g{n, cflag, out_xy, out_inf};
  bk.launch(g, n);
  return E_OK;
}

// ---- fixed-base tables of caller-chosen points on Edwards curves ---------------------------------
// The test of the base (x, y < p, on the curve) runs on the device (checked_base), then build_table
// runs the curve's own variable-base kernel on the scalars and points that FnEdBaseCombGen writes.

template <class BK>
template <int U>
int Engine<BK>::ed_base_table(const u8* xy, bool own, CombTable& out) {
  int rc = E_OK;
  u8* dpt = checked_base<FnEdBaseCheck>(xy, 32, !own, rc);
  if (!dpt) return rc;
  // (the curve's own comb has never been subject to ELLGPU_COMB_MAX_BYTES, and is not now)
  const TablePlan plan{EdWork::COMB_ENTRIES, sizeof(EdWork::P), 32, EdWork::COMB_BITS, false, !own, false};
  rc = build_table(plan, [&](size_t m, size_t first, u8* dk, u8* dp) {
    FnEdBaseCombGen<false> g{m, first, dpt, dk, dp, EdWork::COMB_BITS};
    bk.launch(g, m);
  }, [&](size_t m, const u8* dk, const u8* dp, u8*, u8*, void* dst) {
    return ed_mul_var_chunk(m, dk, dp, nullptr, nullptr, (EdWork::P*)dst);
  }, out);
  bk.free_(dpt);
  return rc;
}


template <class BK>
template <int U>
int Engine<BK>::ed_base_mul_chunk(size_t n, const u8* k1, const EdWork::P* t1, const u8* k2, const EdWork::P* t2,
                                  u8* out_xy, u8* out_inf) {
  u32* ext = claim<u32>(S_JAC, n * 4 * 8 * 4);
  if (int rc = claimed()) return rc;
  if (k2) {
    FnEdMulBase2 f{n, k1, t1, k2, t2, ext};
    bk.launch(f, n);
  } else {
    FnEdMulFixed f{n, k1, t1, ext};
    bk.launch(f, n);
  }
  return ed_normalize_chunk(n, ext, out_xy, out_inf, nullptr);
}

template <class BK>
template <int U>
int Engine<BK>::edc_base_table(const u8* xy, int window_bits, CombTable& out) {
  const int bits = window_bits ? window_bits : 8;
  int rc = E_OK;
  u8* dpt = checked_base<FnEdcBaseCheck>(xy, 32, true, rc);
  if (!dpt) return rc;
  const TablePlan plan{(size_t)(256 / bits) * (((size_t)1 << bits) - 1), sizeof(EdcWork::A), 32, bits, true, true, false};
  rc = build_table(plan, [&](size_t m, size_t first, u8* dk, u8* dp) {
    FnEdBaseCombGen<true> g{m, first, dpt, dk, dp, bits};
    bk.launch(g, m);
  }, [&](size_t m, const u8* dk, const u8* dp, u8*, u8*, void* dst) {
    u32* proj = claim<u32>(S_JAC, m * 3 * 8 * 4);
    u32* pre = claim<u32>(S_PRE, m * 8 * 4);
    auto* tbl = claim<EdcWork::P>(S_TBL, m * 8 * sizeof(EdcWork::P));
    if (int nm = claimed()) return nm;
    FnEdcMulVar f{m, dk, dp, tbl, proj};
    bk.launch(f, m);
    return launch_inv<Route::here, FnEdcBaseNormalize>(field_inv(m), m, proj, pre, (EdcWork::A*)dst);
  }, out);
  bk.free_(dpt);
  return rc;
}


template <class BK>
template <int U>
int Engine<BK>::edc_base_mul_chunk(size_t n, const u8* k1, const EdcWork::A* t1, const u8* k2, const EdcWork::A* t2,
                                   u8* out_xy, u8* out_inf) {
  u32* proj = claim<u32>(S_JAC, n * 3 * 8 * 4);
  u32* pre = claim<u32>(S_PRE, n * 8 * 4);
  if (int rc = claimed()) return rc;
  if (k2) {
    FnEdcMulBase2 f{n, k1, t1, k2, t2, proj};
    bk.launch(f, n);
  } else {
    FnEdcMulBase f{n, k1, t1, proj};
    bk.launch(f, n);
  }
  return launch_inv<Route::here, FnEdcNormalize>(field_inv(n), n, proj, pre, out_xy, out_inf);
}

template <class BK>
template <int U>
int Engine<BK>::x25519_chunk(size_t n, const u8* k, const u8* x, u8* out_x, u8* out_inf, u8* out_bad) {
  u32* xz = claim<u32>(S_JAC, n * 2 * 8 * 4);
  u32* pre = claim<u32>(S_PRE, n * 8 * 4);
  if (int rc = claimed()) return rc;
  if (n <= coop_grid()) {
    FnX25519C fc{n, k, x, xz, out_bad};
    bk.launch_coop(fc, out_bad ? 2 * n : n);
  } else {
    FnX25519 f{n, k, x, xz};
    bk.launch(f, n);
    if (out_bad) {
      FnX25519Validate fv{n, x, out_bad};
      bk.launch(fv, n);
    }
  }
  return launch_inv<Route::here, FnX25519Normalize>(field_inv(n), n, xz, pre, out_x, out_inf);
}


template <class BK>
template <class CV>
int Engine<BK>::decompress_chunk(size_t n, const u8* x, const u8* odd, u8* out_xy, u8* out_ok) {
  if constexpr (!CV::F::HAS_SQRT) {
    return fail(E_UNSUPPORTED, "point decompression is not available in this field");
  } else {
    if constexpr (CV::ID == CURVE_SECP256K1 && CoopK256::AVAILABLE) {
      if (n <= coop_grid()) {                          // a handful of items: the square root on a wave each
        FnDecompressC fc{n, x, odd, out_xy, out_ok};
        bk.launch_coop(fc, n);
        return E_OK;
      }
    }
    FnDecompress<CV> f{n, x, odd, out_xy, out_ok};
    bk.launch(f, n);
    return E_OK;
  }
}
template <class BK>
template <class CV>
int Engine<BK>::codec_chunk(int op, size_t n, const u8* in, size_t len, int flag, const u8* inf, u8* out,
                            u8* status) {
  typedef Work<CV> W;
  if (op == OP_DECODE) {
    FnDecodePoint<CV> f{n, in, len, out, status};
    bk.launch(f, n);
    return E_OK;
  }
  if (op == OP_ENCODE) {
    FnEncodePoint<CV> f{n, in, flag, out};
    bk.launch(f, n);
    return E_OK;
  }
  // validate: curve equation, then (flag) n * P == O through the variable-base ladder
  u8* tmp = nullptr;
  if (flag) {
    tmp = claim<u8>(S_U12, n * (3 * (size_t)W::BYTES + 1));
    if (int rc = claimed()) return rc;
  }
  FnValidatePoint<CV> f{n, in, inf, status, tmp};
  bk.launch(f, n);
  if (!flag) return E_OK;
  u8* mxy = tmp + n * W::BYTES;
  u8* minf = mxy + n * 2 * W::BYTES;
  int rc = mul_var_chunk<CV>(n, tmp, in, mxy, minf, nullptr);
  if (rc) return rc;
  FnOrderStatus g{n, minf, status};
  bk.launch(g, n);
  return E_OK;
}
template <class BK>
template <class CV>
int Engine<BK>::point_add_chunk(size_t n, const u8* xy1, const u8* inf1, const u8* xy2, const u8* inf2,
                                u8* out_xy, u8* out_inf) {
  typedef Work<CV> W;
  u32* jac = claim<u32>(S_JAC, n * 3 * W::NS * 4);
  if (int rc = claimed()) return rc;
  FnPointAdd<CV> f{n, xy1, inf1, xy2, inf2, jac};
  bk.launch(f, n);
  return normalize_chunk<CV>(n, jac, out_xy, out_inf, nullptr);
}
template <class BK>
template <class CV>
int Engine<BK>::der_chunk(int op, size_t n, const u8* a, const u8* b, size_t stride, u32* lens, u8* o1, u8* o2,
                          u8* o3) {
  if (op == OP_FROM_DER) {
    FnSigFromDer<CV> f{n, a, stride, lens, o1, o2, o3};
    bk.launch(f, n);
  } else if (op == OP_TO_DER) {
    FnSigToDer<CV> f{n, a, b, o1, stride, lens};
    bk.launch(f, n);
  } else {
    FnWireStatus<CV> f{n, a, b, o3, o1, o2};
    bk.launch(f, n);
  }
  return E_OK;
}
template <class BK>
template <class CV>
int Engine<BK>::sign_det_chunk(size_t n, const u8* hash, int hash_len, int shift, const u8* priv,
                               int canonical, u8* out_r, u8* out_s, u8* out_recid, u8* out_ok) {
  typedef Work<CV> W;
  u8* nonces = claim<u8>(S_TBL, n * W::NBYTES);           // the sign pipeline uses S_JAC / S_U12 / S_PRE
  if (int rc = claimed()) return rc;
  FnDetNonce<CV> f{n, hash, hash_len, shift, priv, nonces};
  bk.launch(f, n);
  return sign_chunk<CV>(n, hash, hash_len, shift, priv, nonces, canonical, out_r, out_s, out_recid, out_ok);
}

template <class BK>
template <class CV>
int Engine<BK>::recover_chunk(size_t n, const u8* hash, int hash_len, const u8* r, const u8* s,
                              const u8* recid, u8* out_xy, u8* out_status) {
  if constexpr (!CV::F::HAS_SQRT) {
    return fail(E_UNSUPPORTED, "public-key recovery needs point decompression, which this field does not have");
  } else {
    typedef Work<CV> W;
    const size_t B = W::BYTES, NB = W::NBYTES;
    // scalars, the x-coordinates and the decompressed points R live across the ladder kernels,
    // which use S_TBL / S_JAC / S_PRE only
    u8* buf = claim<u8>(S_U12, n * (2 * NB + 3 * B));
    u8* flags = claim<u8>(S_VALID, 3 * n);
    u32* pre = claim<u32>(S_PRE, n * W::LN * 4);
    int rc = claimed();
    if (rc) return rc;
    u8* s1 = buf;
    u8* s2 = s1 + n * NB;
    u8* xs = s2 + n * NB;
    u8* rxy = xs + n * B;
    u8* odd = flags;
    u8* dec_ok = flags + n;
    u8* inf = flags + 2 * n;
    bool front = false;
    if constexpr (CV::ID == CURVE_SECP256K1 && CoopK256::AVAILABLE) {
      if (n <= coop_grid()) {                          // a handful of items: R's square root beside r^-1, one launch
        FnRecoverPartsC fc{n, hash, hash_len, r, s, recid, pre, xs, odd, s1, s2, out_status, rxy, dec_ok};
        bk.launch_coop(fc, 2 * n);
        front = true;
      }
    }
    if (!front) {
      launch_inv<Route::unit, FnRecoverPrep<CV>>(scalar_inv(n), n, hash, hash_len, r, s, recid, pre, xs, odd, s1, s2,
                                                 out_status);
      rc = decompress_chunk<CV>(n, xs, odd, rxy, dec_ok);
      if (rc) return rc;
    }
    rc = mul_add_g_chunk<CV>(n, s1, s2, rxy, out_xy, inf);         // s1 * G + s2 * R
    if (rc) return rc;
    FnRecoverFinish<CV> f2{n, dec_ok, inf, out_xy, out_status};
    bk.launch(f2, n);
    return E_OK;
  }
}

template <class BK>
template <class CV>
int Engine<BK>::recid_chunk(size_t n, const u8* hash, int hash_len, const u8* r, const u8* s, const u8* pub_xy,
                            u8* out_recid, u8* out_status) {
  typedef Work<CV> W;
  const size_t B = W::BYTES, NB = W::NBYTES;
  // both scalars, R' and its flags live across the ladder kernels, which use S_TBL / S_JAC / S_PRE only
  u8* buf = claim<u8>(S_U12, n * (2 * NB + 2 * B));
  u8* inf = claim<u8>(S_VALID, n);
  u32* pre = claim<u32>(S_PRE, n * W::LN * 4);
  if (int rc = claimed()) return rc;
  u8* u1 = buf;
  u8* u2 = u1 + n * NB;
  u8* xy = u2 + n * NB;
  int rc = launch_inv<Route::unit, FnRecidPrep<CV>>(scalar_inv(n), n, hash, hash_len, r, s, pre, u1, u2, out_status);
  if (rc) return rc;
  rc = mul_add_g_chunk<CV>(n, u1, u2, pub_xy, xy, inf);             // R' = u1 * G + u2 * Q
  if (rc) return rc;
  FnRecidFinish<CV> f2{n, r, xy, inf, out_recid, out_status};
  bk.launch(f2, n);
  return E_OK;
}

template <class BK>
template <int U>
int Engine<BK>::ed_decompress_chunk(size_t n, const u8* y, const u8* odd, u8* out_xy, u8* out_ok) {
  FnEdDecompress f{n, y, odd, out_xy, out_ok};
  bk.launch(f, n);
  return E_OK;
}

template <class BK>
template <int U>
int Engine<BK>::ed_point_add_chunk(size_t n, const u8* xy1, const u8* inf1, const u8* xy2, const u8* inf2,
                                   u8* out_xy, u8* out_inf) {
  u32* ext = claim<u32>(S_JAC, n * 4 * 8 * 4);
  if (int rc = claimed()) return rc;
  FnEdPointAdd f{n, xy1, inf1, xy2, inf2, ext};
  bk.launch(f, n);
  return ed_normalize_chunk(n, ext, out_xy, out_inf, nullptr);
}

template <class BK>
template <int U>
int Engine<BK>::ed_codec_chunk(int op, size_t n, const u8* in, int flag, const u8* inf, u8* out, u8* status) {
  if (op == OP_DECODE) {
    FnEdDecodePoint f{n, in, out, status};
    bk.launch(f, n);
    return E_OK;
  }
  if (op == OP_ENCODE) {
    FnEdEncodePoint f{n, in, out};
    bk.launch(f, n);
    return E_OK;
  }
  u8* tmp = nullptr;
  if (flag) {
    tmp = claim<u8>(S_U12, n * (3 * 32 + 1));
    if (int rc = claimed()) return rc;
  }
  FnEdValidatePoint f{n, in, inf, status, tmp};
  bk.launch(f, n);
  if (!flag) return E_OK;
  u8* mxy = tmp + n * 32;
  u8* minf = mxy + n * 64;
  int rc = ed_mul_var_chunk(n, tmp, in, mxy, minf, nullptr);
  if (rc) return rc;
  FnOrderStatus g{n, minf, status};
  bk.launch(g, n);
  return E_OK;
}

template <class BK>
template <int U>
int Engine<BK>::eddsa_chunk(size_t n, size_t o, const u8* msgs, const u64* off, size_t msg_len,
                            const u8* sigs, const u8* pubs, u8* ok, u8* err) {
  if (n <= coop_grid()) {
    u32* ext = claim<u32>(S_JAC, 2 * n * 3 * 8 * 4);
    u8* flags = claim<u8>(S_VALID, 2 * n);
    if (int rc = claimed()) return rc;
    FnEddsaPartsC fc{n, off ? msgs : msgs + o * msg_len, off ? off + o : nullptr, msg_len, sigs + o * 64,
                     pubs + o * 32, (const EdWork::P*)comb_[CURVE_ED25519], ext, flags};
    bk.launch_coop(fc, 2 * n);
    FnEddsaJoin fj{n, ext, flags, ok + o, err ? err + o : nullptr};
    bk.launch(fj, n);
    return E_OK;
  }
  auto* tbl = claim<EdWork::P>(S_TBL, n * 8 * sizeof(EdWork::P));
  if (int rc = claimed()) return rc;
  FnEddsaVerify f{n, off ? msgs : msgs + o * msg_len, off ? off + o : nullptr, msg_len,
                  sigs + o * 64, pubs + o * 32, (const EdWork::P*)comb_[CURVE_ED25519], tbl,
                  ok + o, err ? err + o : nullptr};
  bk.launch(f, n);
  return E_OK;
}

template <class BK>
template <int U>
int Engine<BK>::eddsa_base_chunk(size_t n, size_t o, const u8* msgs, const u64* off, size_t msg_len, const u8* sigs,
                                 const u64 (&aw)[4], const EdWork::P* tg, const EdWork::P* tq, u8* ok, u8* err) {
  FnEddsaBase f{n, off ? msgs : msgs + o * msg_len, off ? off + o : nullptr, msg_len, sigs + o * 64,
                {aw[0], aw[1], aw[2], aw[3]}, tg, tq, ok + o, err ? err + o : nullptr};
  bk.launch(f, n);
  return E_OK;
}

template <class BK>
template <int U>
int Engine<BK>::eddsa_sign_chunk(size_t n, size_t o, const u8* secrets, const u8* msgs, const u64* off,
                                 size_t msg_len, u8* sig, u8* pub) {
  u8* scal = claim<u8>(S_U12, 2 * n * 32);                        // a and r, big-endian
  u8* xy = claim<u8>(S_TBL, 2 * n * 64);                          // A = a G and R = r G, affine
  u8* inf = claim<u8>(S_VALID, 2 * n);
  if (int rc = claimed()) return rc;
  const u8* m0 = off ? msgs : msgs + o * msg_len;
  const u64* off0 = off ? off + o : nullptr;
  FnEddsaSignPre f1{n, secrets + o * 32, m0, off0, msg_len, scal};
  bk.launch(f1, n);
  int rc = ed_mul_fixed_chunk(2 * n, scal, xy, inf);
  if (rc) return rc;
  FnEddsaSignPost f2{n, m0, off0, msg_len, scal, xy, sig + o * 64, pub ? pub + o * 32 : nullptr};
  bk.launch(f2, n);
  return E_OK;
}

template <class BK>
template <class CV>
int Engine<BK>::sign_chunk(size_t n, const u8* hash, int hash_len, int shift, const u8* priv,
                           const u8* nonces, int canonical, u8* out_r, u8* out_s, u8* out_recid,
                           u8* out_ok) {
  typedef Work<CV> W;
  u32* jac = claim<u32>(S_JAC, n * 3 * W::NS * 4);
  u8* kg = claim<u8>(S_U12, n * (2 * W::BYTES + 1));             // k*G affine + infinity flags
  if (int rc = claimed()) return rc;
  u8* kg_inf = kg + n * 2 * W::BYTES;
  // a handful of items: k*G (comb + its own inversion) and k^-1 mod n on a wave each, one launch;
  // then the finish without an inversion of its own
  constexpr bool row_k256 = CV::ENDO && W::L <= 8 && CoopK256::AVAILABLE;
  constexpr bool row_nist = !CV::ENDO && CoopNist<CV>::AVAILABLE;
  if constexpr (row_k256 || row_nist) {
    if (n <= coop_grid_of<CV>()) {
      u32* kinv = claim<u32>(S_PRE, n * 2 * (W::LN > W::NS ? W::LN : W::NS) * 4);
      if (int rc = claimed()) return rc;
      u32* pre2 = kinv + n * (W::LN > W::NS ? W::LN : W::NS);
      typedef typename std::conditional<row_k256, CoopK256, CoopNist<CV>>::type CW;
      FnSignPartsC<CV, CW> fc{n, nonces, comb_of<CV>(), kg, kg_inf, kinv};
      bk.launch_coop(fc, 2 * n);
      // a geometry of its own, not scalar_inv()'s: k^-1 is there already (kinv), so the finish
      // shares no inversion -- one item per thread
      FnSignFinish<CV> f2{n, n, 1, hash, hash_len, shift, priv, nonces, kg, kg_inf, canonical, pre2,
                          out_r, out_s, out_recid, out_ok, kinv};
      return launch_fn(f2, n);
    }
  }
  launch_paired<FnSignMul, CV>(n, nonces, comb_of<CV>(), jac);
  int rc = normalize_chunk<CV>(n, jac, kg, kg_inf, nullptr);
  if (rc) return rc;
  u32* pre = claim<u32>(S_PRE, n * (W::LN > W::NS ? W::LN : W::NS) * 4);
  if ((rc = claimed())) return rc;
  return launch_inv<Route::unit, FnSignFinish<CV>>(scalar_inv(n), n, hash, hash_len, shift, priv, nonces, kg, kg_inf,
                                                   canonical, pre, out_r, out_s, out_recid, out_ok, nullptr);
}

}  // namespace ell
