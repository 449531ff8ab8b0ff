// tests/hostsim/k256_pair_probe -- CPU-only probes of FpK256's pair products and of the secp256k1
// group law built on them.
//
// TEST INFRASTRUCTURE, like hostsim.cpp: the device headers compiled with g++ (their portable
// path), here only fp.h / short.h / curves.h, so that tests/test_k256_pair_hostsim.py can put
// single field operations and single group operations next to Python integers.  Built by that
// test into tests/hostsim/_build/, never loaded by elliptic_amd.
//
// Field elements are 8 little-endian 32-bit words, canonical; a Jacobian point is X | Y | Z
// (24 words), an affine one x | y (16 words).
#include "../../elliptic_amd/csrc/curves.h"
#include "../../elliptic_amd/csrc/short.h"

using namespace ell;

typedef CvSecp256k1 CV;
typedef FpK256 F;
typedef ShortOps<CV> G;
static_assert(has_pair<F>::value, "FpK256 offers the pair products");

static F::El ld(const u32* w) {
  F::El e;
  for (int i = 0; i < 8; i++) e.v[i] = w[i];
  return e;
}
static void st(u32* w, const F::El& e) {
  for (int i = 0; i < 8; i++) w[i] = e.v[i];
}
static Jac<F> ldj(const u32* w) {
  Jac<F> p;
  p.X = ld(w); p.Y = ld(w + 8); p.Z = ld(w + 16);
  return p;
}
static void stj(u32* w, const Jac<F>& p) {
  st(w, p.X); st(w + 8, p.Y); st(w + 16, p.Z);
}
static Aff<F> lda(const u32* w) {
  Aff<F> q;
  q.x = ld(w); q.y = ld(w + 8);
  return q;
}

extern "C" {
// what the build compiled in: bit 0 ELL_K256_PAIR, bit 1 the pair doubling, bit 2 the pair mixed addition
int kp_config() { return (F::PAIR ? 1 : 0) | (pair_dbl<F>::value ? 2 : 0) | (G::PAIR_ADD ? 4 : 0); }

// n items of four operands a, b, c, d (8 words each, canonical):
//   op 0: mul_sub_mul(a, b, c, d)      op 1: mul_sub_sqr(a, b, c)      op 2: half(a)
//   op 3: sub(mul(a, b), mul(c, d))    op 4: sub(mul(a, b), sqr(c))    (the separate operations)
int kp_field_op(int op, size_t n, const u32* a, const u32* b, const u32* c, const u32* d, u32* r) {
  if (op < 0 || op > 4) return -1;
  for (size_t i = 0; i < n; i++) {
    const F::El x = ld(a + 8 * i), y = ld(b + 8 * i), z = ld(c + 8 * i), w = ld(d + 8 * i);
    F::El o;
    switch (op) {
      case 0: o = F::mul_sub_mul(x, y, z, w); break;
      case 1: o = F::mul_sub_sqr(x, y, z); break;
      case 2: o = F::half(x); break;
      case 3: o = F::sub(F::mul(x, y), F::mul(z, w)); break;
      default: o = F::sub(F::mul(x, y), F::sqr(z)); break;
    }
    st(r + 8 * i, o);
  }
  return 0;
}

// n doublings: out = 2 P
void kp_dbl(size_t n, const u32* p, u32* out) {
  for (size_t i = 0; i < n; i++) stj(out + 24 * i, G::dbl(ldj(p + 24 * i)));
}

// n mixed additions P + Q, Q affine and finite:
//   form 0: add_mixed_lean (pinf[i] = "P is O" going in, "the sum is O" coming out)
//   form 1: add_mixed      form 2: add_mixed_zr (no exceptional inputs; h[i] receives the ratio)
int kp_add_mixed(int form, size_t n, const u32* p, const u32* q, unsigned char* pinf, u32* h, u32* out) {
  if (form < 0 || form > 2) return -1;
  for (size_t i = 0; i < n; i++) {
    const Jac<F> P = ldj(p + 24 * i);
    const Aff<F> Q = lda(q + 16 * i);
    Jac<F> r;
    if (form == 0) {
      bool inf = pinf[i] != 0;
      r = G::add_mixed_lean(P, Q, inf, [&]() { return Q; });
      pinf[i] = inf ? 1 : 0;
    } else if (form == 1) {
      r = G::add_mixed(P, Q);
    } else {
      F::El hh;
      r = G::add_mixed_zr(P, Q, hh);
      st(h + 8 * i, hh);
    }
    stj(out + 24 * i, r);
  }
  return 0;
}
}
