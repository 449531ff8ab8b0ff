/* ellgpu_addn.h -- entry points of libellgpu.so added after the fifth recorded prototype table.
 *
 * include/ellgpu.h and include/ellgpu_ext.h .. include/ellgpu_ext4.h, and the binding tables written
 * against them, are pinned symbol for symbol by recorded fixtures.  An entry point that comes later
 * is declared here: this header includes ellgpu_ext4.h (and through it the other five) and adds to
 * them; nothing it declares changes a prototype, a code or ELLGPU_VERSION.  (The name: the list of
 * files the library is built from keeps ellgpu_ext3.h and ellgpu_ext4.h last and everything before
 * them sorted, so this header sorts between ellgpu.h and ellgpu_ext.h.)
 *
 * ---- Sums of many k * P terms -------------------------------------------------------------------
 *
 * ellgpu_mul_sum computes n independent sums of m terms each,
 *
 *   out[j] = sum over i < m of k[j m + i] * P[j m + i]
 *
 * which is the reference's curve._wnafMulAdd(1, points, coeffs, m) (base.js:128-253; on secp256k1
 * _endoWnafMulAdd, short.js:452-507) for any number of points: vector commitments, aggregated keys,
 * the linear combinations of batch verification.  ellgpu_mul_add2 stops at two terms.  Here
 * neighbouring terms go through that call's two-term ladder (shared doublings), the partial sums stay
 * in Jacobian form on the device and are added there in halving steps, and every sum is normalised
 * once: one inversion share per sum, not one per pair.
 *
 * For one sum the result is byte for byte what ellgpu_mul_var on each term followed by the
 * reference's Point#add in order gives.
 *
 *   curve    one of the six short Weierstrass presets, or a user-defined short id (plain or domain).
 *            ed25519, user-defined Edwards ids, curve25519 and user-defined Montgomery ids:
 *            ELLGPU_E_UNSUPPORTED (sums on Edwards curves are a later change).  An unknown id:
 *            ELLGPU_E_ARG.
 *   n, m     n sums of m terms.  m == 0: ELLGPU_E_ARG.  n == 0: success, nothing is written.
 *            n m or n m 2 B overflowing size_t: ELLGPU_E_ARG.
 *   k        n m scalars of B bytes, big-endian, B = the curve's field bytes (32 on user-defined
 *            ids).  A scalar is used as it stands, as Point#mul uses it: it is not reduced mod n, so
 *            k >= n and all-ones are legal, and k = 0 contributes O.
 *   xy       n m points x || y of 2 B bytes.  Coordinates >= p are reduced first, as in every call.
 *   out_xy   n x 2 B bytes.
 *   out_inf  n bytes: 0 a point; 1 the sum is O, out_xy zeroed; 2 ELLGPU_STATUS_OFF_CURVE: at least
 *            one term's point is not on the curve (see DOMAIN in ellgpu.h), out_xy zeroed -- never a
 *            guess.  Such a sum disturbs no other sum of the batch.
 *            A null pointer among k, xy, out_xy, out_inf with n > 0: ELLGPU_E_ARG.
 *   mem, stream
 *            as in ellgpu_mul_base: the call has one form and no _dev twin.  ELLGPU_MEM_HOST requires
 *            stream == NULL.  With ELLGPU_MEM_DEVICE no input may overlap a result, nor the results
 *            each other, else ELLGPU_E_ARG.
 *   groups   a host batch is sharded over the members by whole sums, as ellgpu_ecdsa_recid shards its
 *            batch; with fewer sums than members the call runs on the first member.
 *
 * The kernels run one pair of terms (one addition of partial sums) per lane at every n: the
 * small-batch forms of ellgpu_mul_add2 are not consulted.  The developer override ELLGPU_SUM_SLICE
 * (read when the context is created) sets the most pairs one launch takes, minimum 1; a sum with more
 * pairs is walked in slices.
 *
 * Out of scope of this entry point: Edwards curves, a bucket (Pippenger) form for one long sum, terms
 * taken from fixed-base handles, scalars wider than B bytes, the N-API addon and the JavaScript
 * binding's install() -- mulAddMany there keeps pairing its points over ellgpu_mul_add2.
 */
#ifndef ELLGPU_ADDN_H
#define ELLGPU_ADDN_H

#include "ellgpu_ext4.h"

#ifdef __cplusplus
extern "C" {
#endif

int ellgpu_mul_sum(ellgpu_ctx* ctx, int curve, size_t n, size_t m, const uint8_t* k, const uint8_t* xy,
                   uint8_t* out_xy, uint8_t* out_inf, int mem, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ELLGPU_ADDN_H */
