// ellgpu -- explicit-instantiation plumbing so that the (curve x operation)
// kernels compile in separate translation units (inst.hip, built in parallel by
// elliptic_amd/build.py) instead of one 20-minute TU.
#pragma once

#include "hip_backend.h"

namespace ell {

#define ELL_FOR_SHORT_CURVES(X) X(CvSecp256k1) X(CvP192) X(CvP224) X(CvP256) X(CvP384) X(CvP521)

#define ELL_DECL_G0(KW, CV)                                                                        \
  KW template int Engine<HipBackend>::mul_var_chunk<CV>(size_t, const u8*, const u8*, u8*, u8*,    \
                                                        Work<CV>::A*);                             \
  KW template int Engine<HipBackend>::normalize_chunk<CV>(size_t, const u32*, u8*, u8*,            \
                                                          Work<CV>::A*);                           \
  KW template int Engine<HipBackend>::ensure_comb<CV>();
#define ELL_DECL_G1(KW, CV) \
  KW template int Engine<HipBackend>::mul_fixed_chunk<CV>(size_t, const u8*, const Work<CV>::A*,           \
                                                          const u8*, const Work<CV>::A*, u8*, u8*);        \
  KW template int Engine<HipBackend>::base_table<CV>(const u8*, int, Engine<HipBackend>::CombTable&); \
  KW template int Engine<HipBackend>::ecdsa_base_chunk<CV>(size_t, const u8*, int, int, const u8*, const u8*, \
                                                           const Work<CV>::A*, const Work<CV>::A*, u8*);
#define ELL_DECL_G2(KW, CV)                                                                  \
  KW template int Engine<HipBackend>::mul_add2_chunk<CV>(size_t, const u8*, const u8*,       \
                                                         const u8*, const u8*, u8*, u8*);    \
  KW template int Engine<HipBackend>::sum_chunk<CV>(size_t, size_t, const u8*, const u8*, u8*, u8*);
#define ELL_DECL_G3(KW, CV)                                                                   \
  KW template int Engine<HipBackend>::mul_add_g_chunk<CV>(size_t, const u8*, const u8*,       \
                                                          const u8*, u8*, u8*);
#define ELL_DECL_G4(KW, CV)                                                                       \
  KW template int Engine<HipBackend>::ecdsa_chunk<CV>(size_t, const u8*, int, int, const u8*,     \
                                                      const u8*, const u8*, u8*, u8*);

#define ELL_DECL_G5(KW, CV)                                                                       \
  KW template int Engine<HipBackend>::decompress_chunk<CV>(size_t, const u8*, const u8*, u8*, u8*); \
  KW template int Engine<HipBackend>::codec_chunk<CV>(int, size_t, const u8*, size_t, int,         \
                                                      const u8*, u8*, u8*);                         \
  KW template int Engine<HipBackend>::point_add_chunk<CV>(size_t, const u8*, const u8*, const u8*, \
                                                          const u8*, u8*, u8*);                     \
  KW template int Engine<HipBackend>::der_chunk<CV>(int, size_t, const u8*, const u8*, size_t,     \
                                                    u32*, u8*, u8*, u8*);                           \
  KW template int Engine<HipBackend>::sign_chunk<CV>(size_t, const u8*, int, int, const u8*,       \
                                                     const u8*, int, u8*, u8*, u8*, u8*);           \
  KW template int Engine<HipBackend>::recover_chunk<CV>(size_t, const u8*, int, const u8*,         \
                                                        const u8*, const u8*, u8*, u8*);           \
  KW template int Engine<HipBackend>::recid_chunk<CV>(size_t, const u8*, int, const u8*,           \
                                                      const u8*, const u8*, u8*, u8*);             \
  KW template int Engine<HipBackend>::sign_det_chunk<CV>(size_t, const u8*, int, int, const u8*,   \
                                                         int, u8*, u8*, u8*, u8*);
// scalar-field kernels (batched inversion / Montgomery arithmetic mod n): their own translation
// units, compiled with -mllvm -amdgpu-sched-strategy=max-ilp (build.py)
#define ELL_DECL_G6(KW, CV)                                                                        \
  KW template int Engine<HipBackend>::launch_fn<FnEcdsaPrep<CV>>(const FnEcdsaPrep<CV>&, size_t);   \
  KW template int Engine<HipBackend>::launch_fn<FnSignFinish<CV>>(const FnSignFinish<CV>&, size_t); \
  KW template int Engine<HipBackend>::launch_fn<FnRecoverPrep<CV>>(const FnRecoverPrep<CV>&, size_t); \
  KW template int Engine<HipBackend>::launch_fn<FnRecidPrep<CV>>(const FnRecidPrep<CV>&, size_t);
// the small-grid (WIDE) verify kernel of the endomorphism curve: its own translation unit
#define ELL_DECL_G7(KW)                                                                              \
  KW template int Engine<HipBackend>::launch_fn<FnEcdsaMain<CvSecp256k1, 3, true>>(                  \
      const FnEcdsaMain<CvSecp256k1, 3, true>&, size_t);                                             \
  KW template int Engine<HipBackend>::launch_fn<FnMulVar<CvSecp256k1, 3, true>>(                     \
      const FnMulVar<CvSecp256k1, 3, true>&, size_t);                                                \
  KW template int Engine<HipBackend>::launch_fn<FnEcdsaPrepTable<CvSecp256k1>>(                      \
      const FnEcdsaPrepTable<CvSecp256k1>&, size_t);                                                 \
  KW template int Engine<HipBackend>::launch_fn<FnEcdsaLadder<CvSecp256k1, true>>(                   \
      const FnEcdsaLadder<CvSecp256k1, true>&, size_t);
// the parted verify (three lanes per item: batches that leave most of the device idle)
#define ELL_DECL_G8(KW)                                                                              \
  KW template int Engine<HipBackend>::launch_fn<FnEcdsaParts<CvSecp256k1>>(                          \
      const FnEcdsaParts<CvSecp256k1>&, size_t);                                                     \
  KW template int Engine<HipBackend>::launch_fn<FnEcdsaJoin<CvSecp256k1>>(                           \
      const FnEcdsaJoin<CvSecp256k1>&, size_t);                                                      \
  KW template int Engine<HipBackend>::launch_fn<FnMulParts<CvSecp256k1>>(                            \
      const FnMulParts<CvSecp256k1>&, size_t);                                                       \
  KW template int Engine<HipBackend>::launch_fn<FnMulJoin<CvSecp256k1>>(                             \
      const FnMulJoin<CvSecp256k1>&, size_t);
// user-defined short curves (CvCustom): scalar multiplication, point addition and the wire
// formats (pointFromX, decodePoint, the DER parser, the wire verify's status), ECDH, key validation
// and SEC1 encoding; user-defined Edwards (edc_chunk, ed_sum_chunk<EdcWork>; the tables of caller-chosen bases: edc_base_*; the key
// side: edk_*_chunk) and Montgomery (montc_chunk) curves
#define ELL_DECL_CUSTOM(KW)                                                                          \
  KW template int Engine<HipBackend>::mul_var_chunk<CvCustom>(size_t, const u8*, const u8*, u8*, u8*, \
                                                              Work<CvCustom>::A*);                   \
  KW template int Engine<HipBackend>::normalize_chunk<CvCustom>(size_t, const u32*, u8*, u8*,        \
                                                                Work<CvCustom>::A*);                 \
  KW template int Engine<HipBackend>::mul_add2_chunk<CvCustom>(size_t, const u8*, const u8*,         \
                                                               const u8*, const u8*, u8*, u8*);      \
  KW template int Engine<HipBackend>::sum_chunk<CvCustom>(size_t, size_t, const u8*, const u8*, u8*, \
                                                          u8*);                                      \
  KW template int Engine<HipBackend>::point_add_chunk<CvCustom>(size_t, const u8*, const u8*, const u8*, \
                                                                const u8*, u8*, u8*);                \
  KW template int Engine<HipBackend>::edc_chunk<0>(int, size_t, const u8*, const u8*, const u8*,     \
                                                   const u8*, const u8*, const u8*, u8*, u8*);       \
  KW template int Engine<HipBackend>::ed_sum_chunk<EdcWork>(size_t, size_t, const u8*, const u8*,   \
                                                            u8*, u8*);                               \
  KW template int Engine<HipBackend>::edc_base_table<0>(const u8*, int, Engine<HipBackend>::CombTable&); \
  KW template int Engine<HipBackend>::edc_base_mul_chunk<0>(size_t, const u8*, const EdcWork::A*,    \
                                                            const u8*, const EdcWork::A*, u8*, u8*); \
  KW template int Engine<HipBackend>::montc_chunk<0>(int, size_t, const u8*, const u8*, u8*, u8*);   \
  KW template int Engine<HipBackend>::edk_point_chunk<0>(size_t, const u8*, const u8*, int, size_t,  \
                                                         u8*, u8*, u8*);                             \
  KW template int Engine<HipBackend>::edk_derive_chunk<0>(size_t, const u8*, const u8*, size_t, u8*, \
                                                          u8*, u8*);                                 \
  KW template int Engine<HipBackend>::edk_validate_chunk<0>(size_t, const u8*, const u8*, u8*);      \
  KW template int Engine<HipBackend>::edk_encode_chunk<0>(size_t, const u8*, int, u8*);              \
  KW template int Engine<HipBackend>::rt_wire_chunk<0>(int, size_t, const u8*, const u8*, size_t,    \
                                                       const u32*, u8*, u8*, u8*);                   \
  KW template int Engine<HipBackend>::rt_ecdh_ladder<0>(size_t, const u8*, const u8*, size_t, bool,  \
                                                        u8*&, u32*&);                                \
  KW template int Engine<HipBackend>::rt_derive_chunk<0>(size_t, const u8*, const u8*, size_t, u8*,  \
                                                         u8*, u8*);                                  \
  KW template int Engine<HipBackend>::rt_validate_chunk<0>(size_t, const u8*, const u8*, bool, u8*); \
  KW template int Engine<HipBackend>::rt_encode_chunk<0>(size_t, const u8*, int, u8*);
// user-defined ECDSA domains (CvCustomDomain): verify (per-item keys, and against a key's table),
// recovery, sign, k*G, k1*G + k2*Q and the tables of
// caller-chosen bases (on plain ids too: Engine::base_upload) -- their own translation
// unit (group 17, with its own parameter block); the window ladder of the comb build is CvCustom's
#define ELL_DECL_DOMAIN(KW)                                                                          \
  KW template int Engine<HipBackend>::ensure_comb<CvCustomDomain>();                                 \
  KW template int Engine<HipBackend>::normalize_chunk<CvCustomDomain>(size_t, const u32*, u8*, u8*,  \
                                                                      Work<CvCustomDomain>::A*);     \
  KW template int Engine<HipBackend>::mul_fixed_chunk<CvCustomDomain>(                               \
      size_t, const u8*, const Work<CvCustomDomain>::A*, const u8*, const Work<CvCustomDomain>::A*, u8*, u8*); \
  KW template int Engine<HipBackend>::base_table<CvCustomDomain>(const u8*, int,                     \
                                                                 Engine<HipBackend>::CombTable&);    \
  KW template int Engine<HipBackend>::mul_add_g_chunk<CvCustomDomain>(size_t, const u8*, const u8*,  \
                                                                      const u8*, u8*, u8*);          \
  KW template int Engine<HipBackend>::ecdsa_chunk<CvCustomDomain>(size_t, const u8*, int, int,       \
                                                                  const u8*, const u8*, const u8*,   \
                                                                  u8*, u8*);                         \
  KW template int Engine<HipBackend>::ecdsa_base_chunk<CvCustomDomain>(                              \
      size_t, const u8*, int, int, const u8*, const u8*, const Work<CvCustomDomain>::A*,             \
      const Work<CvCustomDomain>::A*, u8*);                                                          \
  KW template int Engine<HipBackend>::rt_recover_chunk<0>(size_t, const u8*, int, const u8*,         \
                                                          const u8*, const u8*, u8*, u8*);           \
  KW template int Engine<HipBackend>::rt_sign_chunk<0>(size_t, const u8*, int, int, const u8*,       \
                                                       const u8*, int, int, u8*, u8*, u8*, u8*);     \
  KW template int Engine<HipBackend>::launch_fn<FnEcdsaPrep<CvCustomDomain>>(                        \
      const FnEcdsaPrep<CvCustomDomain>&, size_t);                                                   \
  KW template int Engine<HipBackend>::launch_fn<FnRtSignNonce<Sha256>>(const FnRtSignNonce<Sha256>&, size_t); \
  KW template int Engine<HipBackend>::launch_fn<FnRtSignNonce<Sha384>>(const FnRtSignNonce<Sha384>&, size_t); \
  KW template int Engine<HipBackend>::launch_fn<FnRtSignNonce<Sha512>>(const FnRtSignNonce<Sha512>&, size_t); \
  KW template int Engine<HipBackend>::launch_fn<FnRtSignFinish>(const FnRtSignFinish&, size_t);
// ECDSA on user-defined Edwards domains (edcecdsa.h): G's table, the verify ladder and its two
// comparisons, k*G and its normalisation -- their own translation unit (group 18, with its own
// parameter block).  The scalar-field passes around them are the short domain's kernels, launched
// through the launch_fn instantiations of group 17 above: they read n from that unit's block.
#define ELL_DECL_EDDOMAIN(KW)                                                                        \
  KW template int Engine<HipBackend>::ensure_ed_gtable<0>();                                         \
  KW template int Engine<HipBackend>::edc_verify_chunk<0>(size_t, const u8*, int, int, const u8*,    \
                                                          const u8*, const u8*, u8*, u8*);           \
  KW template int Engine<HipBackend>::edc_sign_chunk<0>(size_t, const u8*, int, int, const u8*,      \
                                                        const u8*, int, int, u8*, u8*, u8*, u8*);
#define ELL_DECL_ED2(KW)                                                                            \
  KW template int Engine<HipBackend>::ed_decompress_chunk<0>(size_t, const u8*, const u8*, u8*, u8*); \
  KW template int Engine<HipBackend>::ed_codec_chunk<0>(int, size_t, const u8*, int, const u8*, u8*, u8*); \
  KW template int Engine<HipBackend>::ed_point_add_chunk<0>(size_t, const u8*, const u8*, const u8*,  \
                                                            const u8*, u8*, u8*);
#define ELL_DECL_ED3(KW)                                                                          \
  KW template int Engine<HipBackend>::eddsa_chunk<0>(size_t, size_t, const u8*, const u64*, size_t, \
                                                     const u8*, const u8*, u8*, u8*);               \
  KW template int Engine<HipBackend>::eddsa_base_chunk<0>(size_t, size_t, const u8*, const u64*, size_t, \
                                                          const u8*, const u64 (&)[4], const EdWork::P*,  \
                                                          const EdWork::P*, u8*, u8*);
#define ELL_DECL_ED4(KW)                                                                          \
  KW template int Engine<HipBackend>::eddsa_sign_chunk<0>(size_t, size_t, const u8*, const u8*,   \
                                                          const u64*, size_t, u8*, u8*);

#define ELL_DECL_ED0(KW)                                                                          \
  KW template int Engine<HipBackend>::ed_normalize_chunk<0>(size_t, const u32*, u8*, u8*,         \
                                                            EdWork::P*);                          \
  KW template int Engine<HipBackend>::ed_mul_var_chunk<0>(size_t, const u8*, const u8*, u8*, u8*, \
                                                          EdWork::P*);
#define ELL_DECL_ED1(KW)                                                                     \
  KW template int Engine<HipBackend>::ed_mul_fixed_chunk<0>(size_t, const u8*, u8*, u8*);    \
  KW template int Engine<HipBackend>::ensure_ed_comb<0>();                                   \
  KW template int Engine<HipBackend>::ed_base_table<0>(const u8*, bool, Engine<HipBackend>::CombTable&); \
  KW template int Engine<HipBackend>::ed_base_mul_chunk<0>(size_t, const u8*, const EdWork::P*, \
                                                           const u8*, const EdWork::P*, u8*, u8*); \
  KW template int Engine<HipBackend>::ed_mul_add2_chunk<0>(size_t, const u8*, const u8*,     \
                                                           const u8*, const u8*, u8*, u8*);  \
  KW template int Engine<HipBackend>::ed_sum_chunk<EdWork>(size_t, size_t, const u8*, const u8*, u8*, u8*);
#define ELL_DECL_X(KW) \
  KW template int Engine<HipBackend>::x25519_chunk<0>(size_t, const u8*, const u8*, u8*, u8*, u8*);

// everything is extern by default ...
#define ELL_EXT_ALL(CV) \
  ELL_DECL_G0(extern, CV) ELL_DECL_G1(extern, CV) ELL_DECL_G2(extern, CV) ELL_DECL_G3(extern, CV) ELL_DECL_G4(extern, CV) \
  ELL_DECL_G5(extern, CV) ELL_DECL_G6(extern, CV)
ELL_FOR_SHORT_CURVES(ELL_EXT_ALL)
ELL_DECL_ED0(extern)
ELL_DECL_ED1(extern)
ELL_DECL_X(extern)
ELL_DECL_ED2(extern)
ELL_DECL_ED3(extern)
ELL_DECL_ED4(extern)
ELL_DECL_CUSTOM(extern)
ELL_DECL_DOMAIN(extern)
ELL_DECL_EDDOMAIN(extern)
ELL_DECL_G7(extern)
ELL_DECL_G8(extern)

}  // namespace ell
