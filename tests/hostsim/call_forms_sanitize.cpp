// tests/hostsim -- the C layer's call helper (capi_common.h ell_call: the context's lock, the lane
// bookkeeping, finish) and the Engine's batch() under the host sanitizers.  A stand-alone program,
// CPU only, no part of the pytest suite:
//
//   g++ -O1 -g -std=c++17 -fno-strict-aliasing -pthread -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -DELL_COMB_BITS_256=8 -DELL_BOUNDS_CHECK=1 -DELL_COMB_SLICE=1000 \
//       tests/hostsim/hostsim.cpp tests/hostsim/call_forms_sanitize.cpp -o call_forms_sanitize
//   ./call_forms_sanitize
//
// One host call and one device call (on this build: host memory) of three entry points -- the
// host mul_var IN PLACE, operand = result, which only the host form allows -- on batches below and
// above the pipeline quantum of 8; the two forms must agree byte for byte.  Exit status 0 = clean.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/ellgpu.h"

typedef std::vector<uint8_t> Bytes;

static int fails = 0;
static void check(bool ok, const char* what, size_t n) {
  if (!ok) { fails++; printf("FAIL %s (n = %zu): %s\n", what, n, ellgpu_last_error()); }
}

int main() {
  ellgpu_ctx* ctx = nullptr;
  if (ellgpu_ctx_create(0, &ctx)) { printf("no context: %s\n", ellgpu_last_error()); return 2; }
  const int k1 = ellgpu_curve_id("secp256k1");
  const size_t sizes[] = {3, 20};
  for (size_t n : sizes) {
    Bytes k(n * 32), g(n * 64), out_h(n * 64), out_d(n * 64), inf_h(n), inf_d(n);
    for (size_t i = 0; i < k.size(); i++) k[i] = (uint8_t)(i * 37 + 11);
    // the generator of secp256k1 in every row
    static const uint8_t G[64] = {
        0x79, 0xbe, 0x66, 0x7e, 0xf9, 0xdc, 0xbb, 0xac, 0x55, 0xa0, 0x62, 0x95, 0xce, 0x87, 0x0b, 0x07,
        0x02, 0x9b, 0xfc, 0xdb, 0x2d, 0xce, 0x28, 0xd9, 0x59, 0xf2, 0x81, 0x5b, 0x16, 0xf8, 0x17, 0x98,
        0x48, 0x3a, 0xda, 0x77, 0x26, 0xa3, 0xc4, 0x65, 0x5d, 0xa4, 0xfb, 0xfc, 0x0e, 0x11, 0x08, 0xa8,
        0xfd, 0x17, 0xb4, 0x48, 0xa6, 0x85, 0x54, 0x19, 0x9c, 0x47, 0xd0, 0x8f, 0xfb, 0x10, 0xd4, 0xb8};
    for (size_t i = 0; i < n; i++) memcpy(&g[i * 64], G, 64);

    // Point#mul: the device form on separate buffers, the host form in place
    check(ellgpu_mul_var_dev(ctx, k1, n, k.data(), g.data(), out_d.data(), inf_d.data(), nullptr) == 0, "mul_var_dev", n);
    check(ellgpu_ctx_synchronize(ctx) == 0, "synchronize", n);
    out_h = g;
    check(ellgpu_mul_var(ctx, k1, n, k.data(), out_h.data(), out_h.data(), inf_h.data()) == 0, "mul_var in place", n);
    check(out_h == out_d && inf_h == inf_d, "mul_var: the two forms agree", n);
    check(ellgpu_mul_var_dev(ctx, k1, n, k.data(), out_h.data(), out_h.data(), inf_d.data(), nullptr) == ELLGPU_E_ARG,
          "mul_var_dev refuses in place", n);

    // BasePoint#encode of the results
    Bytes enc_h(n * 65), enc_d(n * 65);
    check(ellgpu_encode_points(ctx, k1, n, out_d.data(), 0, enc_h.data()) == 0, "encode_points", n);
    check(ellgpu_encode_points_dev(ctx, k1, n, out_d.data(), 0, enc_d.data(), nullptr) == 0, "encode_points_dev", n);
    check(enc_h == enc_d, "encode_points: the two forms agree", n);

    // the x25519 ladder (an absent optional output among its operands)
    Bytes x_h(n * 32), x_d(n * 32), xi_h(n), xi_d(n);
    check(ellgpu_x25519_ladder(ctx, n, k.data(), g.data(), x_h.data(), xi_h.data()) == 0, "x25519_ladder", n);
    check(ellgpu_x25519_ladder_dev(ctx, n, k.data(), g.data(), x_d.data(), xi_d.data(), nullptr) == 0, "x25519_ladder_dev", n);
    check(x_h == x_d && xi_h == xi_d, "x25519_ladder: the two forms agree", n);
  }
  // a null context, and a refused call: the helper's two early ways out
  check(ellgpu_mul_var(nullptr, k1, 0, nullptr, nullptr, nullptr, nullptr) == ELLGPU_E_ARG, "null context", 0);
  check(ellgpu_mul_var(ctx, 99, 0, nullptr, nullptr, nullptr, nullptr) == ELLGPU_E_ARG, "unknown curve", 0);
  ellgpu_ctx_destroy(ctx);
  printf(fails ? "%d checks failed\n" : "clean\n", fails);
  return fails ? 1 : 0;
}
