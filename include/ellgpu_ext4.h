/* ellgpu_ext4.h -- entry points of libellgpu.so added after the fourth recorded prototype table.
 *
 * include/ellgpu.h, include/ellgpu_ext.h, include/ellgpu_ext2.h and include/ellgpu_ext3.h, and the
 * binding tables written against them, are pinned symbol for symbol by recorded fixtures.  An entry
 * point that comes later is declared here: this header includes ellgpu_ext3.h (and through it the
 * other three) and adds to them; nothing it declares changes a prototype, a code or ELLGPU_VERSION.
 *
 * ---- The recovery id of an ECDSA signature under a known key, in one pass -------------------------
 *
 * ellgpu_ecdsa_recid is the reference's EC#getKeyRecoveryParam(e, signature, Q)
 * (ec/index.js:261-278) over a batch: for callers that hold (r, s) and the signer's key but no
 * recovery id -- signatures from an HSM or a remote signer, DER signatures on their way to
 * Ethereum's (r, s, v).  The reference calls recoverPubKey for j = 0 .. 3 and compares each result
 * with Q: up to four square roots, inversions mod n and double-scalar products.  On the presets
 * (cofactor 1, n prime) and for r in [1, n), s != 0 (mod n), the candidate R_j recovers Q exactly
 * when R_j = R' := s^-1 (e G + r Q), so at most one j matches and it is read off R':
 *
 *   x(R') = r                       j = parity of y(R')
 *   x(R') = r + n  (as integers)    j = 2 + parity of y(R')     (this implies r < p - n, the
 *                                   reference's 'sencond key candinate' test)
 *   otherwise, or R' = O            the reference throws 'Unable to find valid recovery factor'
 *
 * One double-scalar product, no square root, one inversion mod n shared by a group of items.
 *
 *   out_status[i] = 0  out_recid[i] is the id, 0 .. 3: what the reference returns
 *                   1  the reference throws: no j recovers the key (a wrong key, a tampered r, s or
 *                      hash, e G + r Q = O)
 *                   2  ELLGPU_STATUS_OFF_CURVE: the key is not on the curve (see DOMAIN in
 *                      ellgpu.h; coordinates >= p are reduced mod p first, as curve.point() does and
 *                      as in every other call)
 *                   3  outside the engine's domain: r = 0, r >= n or s = 0 (mod n).  The reference
 *                      goes through BN#invm of an unreduced or zero value there, or answers the first
 *                      j whose x lifts whatever the key is; callers run the reference on those items.
 *                      Such an item disturbs no other item of the batch.
 *   out_recid[i]  = 0 wherever out_status[i] != 0.
 *
 *   curve       one of the six short Weierstrass presets.  ed25519, curve25519 and every
 *               user-defined id: ELLGPU_E_UNSUPPORTED (a user-defined domain may have a cofactor, or
 *               n > p; with a cofactor s R_j = T has several solutions and the rule above is not the
 *               reference's loop -- run that loop over ellgpu_custom_recover).  An unknown id:
 *               ELLGPU_E_ARG.
 *   hash        n x hash_len bytes.  e = new BN(hash) mod n: NOT truncated to the order's bit
 *               length, exactly as in ellgpu_ecdsa_recover (recoverPubKey does not truncate) and
 *               unlike ellgpu_ecdsa_verify.  hash_len: 1 .. twice the order's width in 32-bit words
 *               x 4, as in ellgpu_ecdsa_recover.
 *   r, s        n x order_bytes each, big-endian.  s is reduced mod n before use (the reference's
 *               s.mul(rInv).umod(n) accepts s >= n).
 *   pub_xy      n x 2 field_bytes, the key x || y.
 *   out_recid, out_status
 *               n bytes each; neither may be NULL.
 *   mem, stream as in ellgpu_mul_base: the call has one form and no _dev twin.  ELLGPU_MEM_HOST
 *               requires stream == NULL.  With ELLGPU_MEM_DEVICE no input may overlap a result, nor
 *               the results each other, else ELLGPU_E_ARG.
 *   groups      a host batch is sharded over the members as ellgpu_ecdsa_verify_base shards its
 *               batch.
 *
 * Small and mid-size batches take the row, parted and wave-per-item forms that k1 G + k2 P
 * (ellgpu_mul_add2 without p1) takes at the same n.
 *
 * Out of scope of this entry point: DER input (ellgpu_sig_from_der first), the N-API addon, and
 * routing from the JavaScript binding's install() -- EC#getKeyRecoveryParam keeps reaching the patched
 * recoverPubKey there.
 */
#ifndef ELLGPU_EXT4_H
#define ELLGPU_EXT4_H

#include "ellgpu_ext3.h"

#ifdef __cplusplus
extern "C" {
#endif

int ellgpu_ecdsa_recid(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len, const uint8_t* r,
                       const uint8_t* s, const uint8_t* pub_xy, uint8_t* out_recid, uint8_t* out_status, int mem,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ELLGPU_EXT4_H */
