/* ellgpu_ext.h -- entry points of libellgpu.so added after the recorded prototype table.
 *
 * include/ellgpu.h and the binding table written against it are pinned, symbol for symbol, by a
 * recorded fixture.  An entry point that comes later is declared here: this header includes ellgpu.h
 * and adds to it; nothing it declares changes a prototype, a code or ELLGPU_VERSION.
 *
 * ---- fixed-base tables of caller-chosen points on Edwards curves ----------------------------------
 *
 * ellgpu_base_define (ellgpu.h) builds the comb of a point a caller uses repeatedly -- a Pedersen H, a
 * recipient's or a verifier's long-lived key, a static ECDH key -- on the short Weierstrass curves,
 * and refuses every other id.  ellgpu_ed_base_define is the same call for ed25519 and for
 * user-defined Edwards ids (ellgpu_curve_define_edwards, ellgpu_curve_define_edwards_domain): the
 * reference's BasePoint#precompute() on an Edwards point.  The handle it returns lives in the same
 * list as the short curves' handles (ELLGPU_BASE_MAX live bases per context in total, never reused)
 * and goes to the EXISTING calls:
 *
 *   ellgpu_mul_base    P.precompute(); P.mul(k).  k is 32 bytes per item, used as it stands,
 *                      neither reduced nor clamped.  out_xy / out_inf are byte for byte what
 *                      ellgpu_mul_var writes for the same k and the base's coordinates on the same
 *                      curve id: on ed25519 out_inf = 1 beside (0, 1) at the identity; on a
 *                      user-defined id out_inf = 0 always and Z = 0 (incomplete curves only) gives
 *                      a zeroed point.
 *   ellgpu_mul_base2   k1*B1 + k2*B2 (B1.mulAdd(k1, B2, k2) on two precomputed operands) = what
 *                      ellgpu_mul_add2 gives on the same operands.  Both handles on one curve, else
 *                      ELLGPU_E_ARG -- a short handle beside an Edwards handle counts as two
 *                      curves.  The two walks go into one accumulator with one normalisation;
 *                      base1 == base2 is allowed, two widths may be mixed.
 *   ellgpu_base_info, ellgpu_base_release
 *
 * Host and device memory (`mem`), streams and groups as for the short handles.  Every n runs one item
 * per lane: there is no lanes-per-item form for these handles.
 *
 * ellgpu_ed_base_define
 *   curve        ELLGPU_CURVE_ED25519 or a user-defined Edwards id, plain or domain.  Short ids (use
 *                ellgpu_base_define), curve25519 and user-defined Montgomery ids:
 *                ELLGPU_E_UNSUPPORTED; an unknown id: ELLGPU_E_ARG.
 *   xy           x || y, 32 + 32 bytes big-endian, host memory.  A coordinate >= p or a point off
 *                the curve: ELLGPU_E_ARG (tested on the device).  The identity (0, 1) and points of
 *                small order such as (0, p - 1) are accepted: under the unified Edwards law they are
 *                ordinary table entries.
 *                NULL: the curve's own generator; window_bits must then be 0.  On ed25519 the handle
 *                aliases the curve's own table (built at first use, never freed by
 *                ellgpu_base_release).  On an Edwards domain the handle owns a table of G built by
 *                this call at the default width; the domain's signing and verifying kernels do not
 *                use it.  On a plain Edwards id: ELLGPU_E_ARG.
 *   window_bits  ed25519: 0 or 16, the width of the curve's own comb (16 windows x 65 535 entries of
 *                128 bytes, 134 MB; 16 additions per item).
 *                User-defined: 0 (= 8), 8 or 16 -- an unsigned comb of 256 / bits windows x
 *                (2^bits - 1) affine entries of 64 bytes: 522 KB and 32 additions per item at 8 bits,
 *                67 MB and 16 additions at 16 bits.  ELLGPU_COMB_MAX_BYTES applies per table; a
 *                width that does not fit is ELLGPU_E_NOMEM.  Anything else: ELLGPU_E_ARG.
 *   out_base     the handle.  The same (curve, point, width in use) gives the same handle.  On a
 *                group either every member builds the table or none does.
 */
#ifndef ELLGPU_EXT_H
#define ELLGPU_EXT_H

#include "ellgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

int ellgpu_ed_base_define(ellgpu_ctx* ctx, int curve, const uint8_t* xy, int window_bits, int* out_base);

#ifdef __cplusplus
}
#endif
#endif /* ELLGPU_EXT_H */
