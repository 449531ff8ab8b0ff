/* ellgpu_ext3.h -- entry points of libellgpu.so added after the third recorded prototype table.
 *
 * include/ellgpu.h, include/ellgpu_ext.h and include/ellgpu_ext2.h, and the binding tables written
 * against them, are pinned symbol for symbol by recorded fixtures.  An entry point that comes later
 * is declared here: this header includes ellgpu_ext2.h (and through it the other two) and adds to
 * them; nothing it declares changes a prototype, a code or ELLGPU_VERSION.
 *
 * ---- EdDSA verification against a fixed-base table of the signer's key ---------------------------
 *
 * ellgpu_ed_base_define (ellgpu_ext.h) builds the comb of an ed25519 point a caller uses repeatedly;
 * the key of a signer whose signatures arrive as a stream -- a firmware vendor, a sequencer, an
 * oracle feed, a CA -- is one.  ellgpu_eddsa_verify_base is the reference's
 * EDDSA#verify(message, sig, pub) with a Point as `pub` (eddsa/key.js:17-24: pubBytes() is then
 * encodePoint(point), the canonical encoding), A being the point of the handle:
 *
 *   out_ok[i]  = eddsa.verify(msg[i], sig[i], A)      strictly 0 / 1
 *   out_err[i] = 1 where the reference throws (R does not decode), else 0
 *
 * byte for byte what ellgpu_eddsa_verify writes to out_ok and out_err for the same items with
 * encodePoint(A) repeated in pubs.  The tests run in the order of eddsa/index.js:52-63:
 *
 *   1. S >= n: ok 0, err 0, nothing else counts.
 *   2. h = SHA-512(R bytes as given || encodePoint(A) || M) mod n.
 *   3. R is decoded as ellgpu_eddsa_verify decodes it: a non-canonical y >= p is reduced, x = 0 with
 *      the sign bit set is 'invalid point'.
 *   4. R does not decode: ok 0, err 1.
 *   5. ok = (R + h*A == S*G), compared projectively as Point#eq does.
 *
 * h walks the key's table and S the curve's own table of G, 16 additions each; A is never decoded,
 * no per-item window table is built and no ladder runs.  There is no term for the key: it was
 * tested against the curve when the handle was defined.  The addition law is unified, so a handle
 * that holds the identity, a point of order 2, 4 or 8, or a key with a torsion component is an
 * ordinary key and answers as the reference answers (with a torsion component the verdict depends
 * on h mod 8).
 *
 *   base        a handle of ellgpu_ed_base_define on ed25519.  The generator alias (xy == NULL at
 *               the define) is the key A = G: both walks then read the curve's own table.
 *               A handle of ellgpu_base_define (short curves): ELLGPU_E_UNSUPPORTED.  An Edwards
 *               handle on a user-defined id: ELLGPU_E_UNSUPPORTED (the engine has no EdDSA there).
 *               An unknown or released handle: ELLGPU_E_ARG.
 *   msgs, msg_off, msg_len, sigs
 *               exactly as in ellgpu_eddsa_verify: the messages concatenated, with n + 1 offsets in
 *               the memory the other operands are in, or a uniform stride msg_len where msg_off is
 *               NULL (msgs may then be NULL if msg_len is 0); sigs is n x 64 bytes, R || S.  A host
 *               call tests the offsets (decreasing: ELLGPU_E_ARG) and a null msgs with a non-zero
 *               total length (ELLGPU_E_ARG).
 *   out_ok      n bytes.
 *   out_err     n bytes, or NULL.
 *   mem, stream as in ellgpu_mul_base: the call has one form and no _dev twin.  ELLGPU_MEM_HOST
 *               requires stream == NULL.  With ELLGPU_MEM_DEVICE sigs and msgs (and msg_off) must
 *               not overlap out_ok or out_err, and out_ok must not overlap out_err, else
 *               ELLGPU_E_ARG.  (With offsets in device memory the host cannot read where the messages
 *               end: the test then covers the offsets' own array and the first message byte.)
 *   n == 0      ELLGPU_OK, nothing touched; the handle is looked up first, so the refusals above
 *               still apply.
 *   groups      msg_off == NULL: a host batch is sharded over the members as
 *               ellgpu_ecdsa_verify_base shards its batch (handles are defined on every member).
 *               With offsets the call runs on the first member.
 *
 * Every n runs one item per lane.
 *
 * Out of scope of this entry point:
 *   - EdDSA on user-defined Edwards curves (the engine has none, with or without a handle);
 *   - ECDSA on a user-defined Edwards domain with a key handle (ellgpu_custom_ed_verify takes the
 *     key per item; ellgpu_ecdsa_verify_base keeps refusing Edwards handles);
 *   - a lanes-per-item form for calls of a few items;
 *   - routing from the JavaScript binding's install(): Engine#eddsaVerifyBaseBatch is called directly.
 */
#ifndef ELLGPU_EXT3_H
#define ELLGPU_EXT3_H

#include "ellgpu_ext2.h"

#ifdef __cplusplus
extern "C" {
#endif

int ellgpu_eddsa_verify_base(ellgpu_ctx* ctx, int base, size_t n, const uint8_t* msgs, const uint64_t* msg_off,
                             size_t msg_len, const uint8_t* sigs, uint8_t* out_ok, uint8_t* out_err, int mem,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ELLGPU_EXT3_H */
