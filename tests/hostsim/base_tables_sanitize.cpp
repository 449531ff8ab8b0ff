// tests/hostsim -- the one builder of the fixed-base tables (Engine::build_table, checked_base,
// walk_tables) under the host sanitizers.  A stand-alone program, CPU only, no part of the pytest
// suite; built like call_forms_sanitize.cpp:
//
//   g++ -O1 -g -std=c++17 -fno-strict-aliasing -pthread -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -DELL_COMB_BITS_256=8 -DELL_BOUNDS_CHECK=1 -DELL_COMB_SLICE=1000 \
//       tests/hostsim/hostsim.cpp tests/hostsim/base_tables_sanitize.cpp -o base_tables_sanitize
//   ./base_tables_sanitize
//
// On each of the four families -- a preset short curve, a user-defined short domain, ed25519, a
// user-defined Edwards curve -- one define / mul_base / mul_base2 / release round and one refused
// define (a base off the curve); ed25519's own table through mul_fixed and the alias handle; then the
// context is destroyed.  Exit status 0 and no sanitizer report = clean.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/ellgpu.h"
#include "../../include/ellgpu_ext.h"

typedef std::vector<uint8_t> Bytes;

static int fails = 0;
static void check(bool ok, const char* what, const char* family) {
  if (!ok) { fails++; printf("FAIL %s (%s): %s\n", what, family, ellgpu_last_error()); }
}
static Bytes hex(const char* s) {
  Bytes b(strlen(s) / 2);
  for (size_t i = 0; i < b.size(); i++) {
    unsigned v = 0;
    sscanf(s + 2 * i, "%2x", &v);
    b[i] = (uint8_t)v;
  }
  return b;
}
static Bytes cat(const Bytes& a, const Bytes& b) {
  Bytes r(a);
  r.insert(r.end(), b.begin(), b.end());
  return r;
}

// define, walk one and two tables in both memory kinds, release; then a base off the curve
static void round_of(ellgpu_ctx* ctx, const char* family, int curve, bool ed, const Bytes& xy, int bits) {
  const size_t n = 11;
  Bytes k(n * 32), out_h(n * 64), out_d(n * 64), inf_h(n), inf_d(n);
  for (size_t i = 0; i < k.size(); i++) k[i] = (uint8_t)(i * 37 + 11);
  int h = -1;
  auto define = ed ? ellgpu_ed_base_define : ellgpu_base_define;
  check(define(ctx, curve, xy.data(), bits, &h) == 0, "define", family);
  check(ellgpu_mul_base(ctx, h, n, k.data(), out_h.data(), inf_h.data(), ELLGPU_MEM_HOST, nullptr) == 0, "mul_base", family);
  check(ellgpu_mul_base(ctx, h, n, k.data(), out_d.data(), inf_d.data(), ELLGPU_MEM_DEVICE, nullptr) == 0, "mul_base dev", family);
  check(ellgpu_ctx_synchronize(ctx) == 0, "synchronize", family);
  check(out_h == out_d && inf_h == inf_d, "mul_base: the two memory kinds agree", family);
  check(ellgpu_mul_base2(ctx, h, h, n, k.data(), k.data(), out_h.data(), inf_h.data(), ELLGPU_MEM_HOST, nullptr) == 0,
        "mul_base2", family);
  check(ellgpu_base_release(ctx, h) == 0, "release", family);
  Bytes bad(xy);
  bad[63] ^= 1;
  check(define(ctx, curve, bad.data(), bits, &h) == ELLGPU_E_ARG, "a base off the curve is refused", family);
}

int main() {
  ellgpu_ctx* ctx = nullptr;
  if (ellgpu_ctx_create(0, &ctx)) { printf("no context: %s\n", ellgpu_last_error()); return 2; }
  const Bytes kp = hex("fffffffffffffffffffffffffffffffffffffffffffffffffffffffefffffc2f");
  const Bytes kn = hex("fffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141");
  const Bytes kgx = hex("79be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798");
  const Bytes kgy = hex("483ada7726a3c4655da4fbfc0e1108a8fd17b448a68554199c47d08ffb10d4b8");
  Bytes zero(32, 0), seven(32, 0);
  seven[31] = 7;
  const Bytes ep = hex("7fffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffed");
  const Bytes ea = hex("7fffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffec");
  const Bytes ed = hex("52036cee2b6ffe738cc740797779e89800700a4d4141d8ab75eb4dca135978a3");
  const Bytes egx = hex("216936d3cd6e53fec0a4e231fdd6dc5c692cc7609525a7b2c9562d608f25d51a");
  const Bytes egy = hex("6666666666666666666666666666666666666666666666666666666666666658");

  round_of(ctx, "preset", ellgpu_curve_id("secp256k1"), false, cat(kgx, kgy), 4);
  int dom = -1;
  check(ellgpu_curve_define_short_domain(ctx, kp.data(), zero.data(), seven.data(), kn.data(), kgx.data(), kgy.data(), &dom) == 0,
        "define_short_domain", "short domain");
  round_of(ctx, "short domain", dom, false, cat(kgx, kgy), 8);
  round_of(ctx, "ed25519", ellgpu_curve_id("ed25519"), true, cat(egx, egy), 0);
  int edw = -1;
  check(ellgpu_curve_define_edwards(ctx, ep.data(), ea.data(), ed.data(), &edw) == 0, "define_edwards", "edwards");
  round_of(ctx, "edwards", edw, true, cat(egx, egy), 8);

  // ed25519's own table (built like a table of G by coordinates) and its alias handle
  Bytes k(32, 5), a(64), b(64), ia(1), ib(1);
  int alias = -1;
  check(ellgpu_mul_fixed(ctx, ellgpu_curve_id("ed25519"), 1, k.data(), a.data(), ia.data()) == 0, "mul_fixed", "ed25519");
  check(ellgpu_ed_base_define(ctx, ellgpu_curve_id("ed25519"), nullptr, 0, &alias) == 0, "alias", "ed25519");
  check(ellgpu_mul_base(ctx, alias, 1, k.data(), b.data(), ib.data(), ELLGPU_MEM_HOST, nullptr) == 0, "mul_base alias", "ed25519");
  check(a == b && ia == ib, "alias = mul_fixed", "ed25519");
  ellgpu_ctx_destroy(ctx);
  printf(fails ? "%d checks failed\n" : "clean\n", fails);
  return fails ? 1 : 0;
}
