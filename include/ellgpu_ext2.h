/* ellgpu_ext2.h -- entry points of libellgpu.so added after the second recorded prototype table.
 *
 * include/ellgpu.h and include/ellgpu_ext.h, and the binding tables written against them, are
 * pinned symbol for symbol by recorded fixtures.  An entry point that comes later is declared here:
 * this header includes ellgpu_ext.h (which includes ellgpu.h) and adds to both; nothing it declares
 * changes a prototype, a code or ELLGPU_VERSION.
 *
 * ---- ECDSA verification against a fixed-base table of the signer's key ---------------------------
 *
 * ellgpu_base_define (ellgpu.h) builds the comb of a point a caller uses repeatedly; "a verifier's
 * long-lived key" is one: a CA, an oracle feed, a sequencer, a firmware vendor whose signatures
 * arrive as a stream.  ellgpu_ecdsa_verify_base is EC#verify with that handle as the key:
 *
 *   out_ok[i] = EC#verify(hash[i], {r[i], s[i]}, Q),  Q = the point of `base`,  strictly 0 / 1
 *
 * byte for byte what ellgpu_ecdsa_verify writes to out_ok for the same items with Q repeated in
 * pub_xy.  R = u1*G + u2*Q is two comb walks into one accumulator -- u1 over the curve's own table of
 * G at whatever width it has (ellgpu_ctx_comb_bits), u2 over the key's table at the width it was
 * defined with; the two widths may differ -- where ellgpu_ecdsa_verify runs the variable-base
 * ladder on every item's key.  s^-1 mod n, u1, u2, the truncation of the hash, the range tests of r
 * and s and the x = r (mod n) rule are the device's, as in ellgpu_ecdsa_verify.
 *
 *   base        a handle of ellgpu_base_define on one of the six short presets or on a user-defined
 *               short DOMAIN id (ellgpu_curve_define_short_domain).  The generator alias (xy == NULL
 *               at the define) is accepted: it is the key with d = 1.
 *               A handle on a plain user-defined short id: ELLGPU_E_UNSUPPORTED (ECDSA needs the
 *               domain, as in ellgpu_ecdsa_verify).  A handle of ellgpu_ed_base_define:
 *               ELLGPU_E_UNSUPPORTED.  An unknown or released handle: ELLGPU_E_ARG.
 *   hash, hash_len, msg_bits, r, s
 *               exactly as in ellgpu_ecdsa_verify: n hashes of hash_len bytes, the same truncation
 *               rule (_truncateToN) and the same refusal of a hash_len / msg_bits combination that
 *               leaves more bits than the order's width (ELLGPU_E_ARG); r and s are
 *               ellgpu_curve_order_bytes wide, big-endian.
 *   out_ok      n bytes.  There is no out_status: the key was tested against the curve when the handle
 *               was defined, so status 2 (ELLGPU_STATUS_OFF_CURVE) cannot occur.
 *   mem, stream as in ellgpu_mul_base: the call has one form and no _dev twin.  ELLGPU_MEM_HOST
 *               requires stream == NULL.  With ELLGPU_MEM_DEVICE the operands and out_ok must not
 *               overlap, else ELLGPU_E_ARG.  On a device group a host batch is sharded over the
 *               members as ellgpu_mul_base2's is.
 *   n == 0      ELLGPU_OK, nothing touched (the handle is still looked up).
 *
 * Every n runs one item per lane.
 *
 * Out of scope of this entry point:
 *   - ECDSA on a user-defined Edwards domain with a key handle (ellgpu_custom_ed_verify takes the
 *     key per item);
 *   - EdDSA with a key handle;
 *   - DER input: a caller runs ellgpu_sig_from_der first and passes its r / s;
 *   - a lanes-per-item form for calls of a few items;
 *   - routing from the JavaScript binding's install(): Engine#ecdsaVerifyBaseBatch is called directly.
 */
#ifndef ELLGPU_EXT2_H
#define ELLGPU_EXT2_H

#include "ellgpu_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

int ellgpu_ecdsa_verify_base(ellgpu_ctx* ctx, int base, size_t n, const uint8_t* hash, int hash_len, int msg_bits,
                             const uint8_t* r, const uint8_t* s, uint8_t* out_ok, int mem, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ELLGPU_EXT2_H */
