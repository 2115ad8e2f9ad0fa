// TEST TOOLING ONLY: host (CPU) build of the hexad's direct line product
// (charon_amd/csrc/bls_hex.h hx_line_cb / hx_line_ca, the pieces
// hex_line_mul runs) for tests/test_hex_line_direct_host.py: the six lanes
// (q, c) of a hexad in a loop, the exchanges as array indexing, with the value
// bound checks (TBG_BOUNDS_CHECK) switched on.  Every value crosses this
// interface as 14 raw 28-bit-radix limbs in Montgomery form, exactly as a
// kernel holds it, so the caller chooses non-canonical values and limbs.
#include <cstdint>
#include "../../charon_amd/csrc/bls_pairing.h"
#include "../../charon_amd/csrc/bls_hex.h"

extern "C" unsigned long long tbg_mad_count = 0;

using namespace tbg;

namespace {

Fp ld(const uint32_t* p) {
  Fp r;
  for (int i = 0; i < NL; ++i) r.l[i] = p[i];
  return r;
}
void st_canon(uint32_t* p, const Fp& a) {
  const Fp c = fp_canon(a);
  for (int i = 0; i < NL; ++i) p[i] = c.l[i];
}
// quad order (bls_quad.h): A_q = [a.c0, a.c1, b.c0, b.c1] at 4 q
void ld_quad(const uint32_t* f, Fp4 (&A)[3]) {
  for (int q = 0; q < 3; ++q)
    A[q] = {{ld(f + (4 * q) * NL), ld(f + (4 * q + 1) * NL)}, {ld(f + (4 * q + 2) * NL), ld(f + (4 * q + 3) * NL)}};
}
void st_quad(uint32_t* out, const Fp4 (&C)[3]) {
  for (int q = 0; q < 3; ++q) {
    st_canon(out + (4 * q) * NL, C[q].a.c0);
    st_canon(out + (4 * q + 1) * NL, C[q].a.c1);
    st_canon(out + (4 * q + 2) * NL, C[q].b.c0);
    st_canon(out + (4 * q + 3) * NL, C[q].b.c1);
  }
}
Fp4h lane_of(const Fp4& A, uint32_t c) { return c ? Fp4h{A.a.c1, A.b.c1} : Fp4h{A.a.c0, A.b.c0}; }
// lane (., c)'s view of a value whose components the two lanes of a pair hold
Fp2o view(uint32_t c, const Fp& own, const Fp& partners) { return {own, hx_to_partner(c ^ 1u, partners)}; }

// the six lanes of the direct form: the exchanges as array indexing
void line_direct(const Fp4 (&A)[3], const Fp2& l0, const Fp2& l1, const Fp2& l4, Fp4h (&R)[3][2]) {
  Fp4h H[3][2];
  for (int q = 0; q < 3; ++q)
    for (uint32_t c = 0; c < 2; ++c) H[q][c] = lane_of(A[q], c);
  for (int q = 0; q < 3; ++q)
    for (uint32_t c = 0; c < 2; ++c) {
      const int s = (q + 1) % 3;
      const Fp4o Av = {view(c, H[q][c].a, H[q][c ^ 1].a), view(c, H[q][c].b, H[q][c ^ 1].b)};
      const Fp2o U = view(c, hx_line_u_src(s, H[s][c]), hx_line_u_src(s, H[s][c ^ 1]));
      const Fp2o V = view(c, hx_line_v_src(s, H[s][c]), hx_line_v_src(s, H[s][c ^ 1]));
      R[q][c].b = hx_line_cb(Av, U, l0, l1, l4);
      R[q][c].a = hx_line_ca(q, Av, V, l0, l1, l4);
    }
}
// ... and of the retained Karatsuba form (as tests/hostcheck hc_hex_line)
void line_kara(const Fp4 (&A)[3], const Fp2& l0, const Fp2& l1, const Fp2& l4, Fp4h (&R)[3][2]) {
  HxLine r[3][2];
  for (int q = 0; q < 3; ++q)
    for (uint32_t c = 0; c < 2; ++c) {
      hx_line_u(c, hx_view4(c, A[(q + 1) % 3]), hx_view(c, l1), r[q][c]);
      hx_line_t(c, q, hx_view4(c, A[q]), hx_view(c, l0), hx_view(c, l4), r[q][c]);
    }
  for (int q = 0; q < 3; ++q)
    for (uint32_t c = 0; c < 2; ++c) R[q][c] = hx_line2(c, q, r[q][c], r[q][c ^ 1].W);
}

}  // namespace

extern "C" {

// f (168 words, quad order) times the line (84 words: l0, l1, l4, each c0 then
// c1).  pt = (-x, y) (28 words): the line is stored unevaluated and lane
// (0, c) forms l1_c (-x), lane (1, c) l4_c y, as hex_line_at_v; pt = null:
// the line is evaluated already (hex_line_folded).  Three results, each 168
// canonical Montgomery words: the direct form lane by lane, the retained
// Karatsuba form lane by lane, and fp12_mul by the sparse element in the
// tower.  raw (168 words, or null): the direct form's words as the lanes
// leave them.  Returns 0.
int hxl_hc_line(const uint32_t* f, const uint32_t* line, const uint32_t* pt, uint32_t* direct, uint32_t* kara,
                uint32_t* tower, uint32_t* raw) {
  Fp4 A[3];
  ld_quad(f, A);
  const Fp2 l0 = {ld(line), ld(line + NL)};
  Fp2 l1 = {ld(line + 2 * NL), ld(line + 3 * NL)}, l4 = {ld(line + 4 * NL), ld(line + 5 * NL)};
  if (pt) {
    const Fp nx = ld(pt), y = ld(pt + NL);
    l1 = {fp_mul(l1.c0, nx), fp_mul(l1.c1, nx)};  // lanes (0, 0), (0, 1)
    l4 = {fp_mul(l4.c0, y), fp_mul(l4.c1, y)};    // lanes (1, 0), (1, 1)
  }
  Fp4h R[3][2];
  line_direct(A, l0, l1, l4, R);
  Fp4 C[3];
  for (int q = 0; q < 3; ++q) C[q] = {{R[q][0].a, R[q][1].a}, {R[q][0].b, R[q][1].b}};
  st_quad(direct, C);
  if (raw)
    for (int q = 0; q < 3; ++q)
      for (int k = 0; k < 4; ++k) {
        const Fp& v = k == 0 ? C[q].a.c0 : k == 1 ? C[q].a.c1 : k == 2 ? C[q].b.c0 : C[q].b.c1;
        for (int i = 0; i < NL; ++i) raw[(4 * q + k) * NL + i] = v.l[i];
      }

  line_kara(A, l0, l1, l4, R);
  for (int q = 0; q < 3; ++q) C[q] = {{R[q][0].a, R[q][1].a}, {R[q][0].b, R[q][1].b}};
  st_quad(kara, C);

  const Fp2 z = {fp_zero(), fp_zero()};
  const Fp12 sparse = {{l0, l1, z}, {z, l4, z}};
  const Fp12 t = fp12_mul(quad_to_fp12(A[0], A[1], A[2]), sparse);
  for (int q = 0; q < 3; ++q) C[q] = quad_from_fp12(q, t);
  st_quad(tower, C);
  return 0;
}

// one hx_line_sum6 on raw operands: left = x0.o, x0.p, x1.o, x1.p, x2.o, x2.p,
// right = y0.c0, y0.c1, ... (6 x 14 words each); out: the 14 words as formed
int hxl_hc_sum6(const uint32_t* left, const uint32_t* right, uint32_t* out) {
  Fp2o x[3];
  Fp2 y[3];
  for (int k = 0; k < 3; ++k) {
    x[k] = {ld(left + 2 * k * NL), ld(left + (2 * k + 1) * NL)};
    y[k] = {ld(right + 2 * k * NL), ld(right + (2 * k + 1) * NL)};
  }
  const Fp r = hx_line_sum6(x[0], y[0], x[1], y[1], x[2], y[2]);
  for (int i = 0; i < NL; ++i) out[i] = r.l[i];
  return 0;
}

// u32 multiply-adds of one line product over the six lanes (a TBG_COUNT_OPS
// build: tools/count_work.py; 0 otherwise): form 0 direct, 1 Karatsuba
unsigned long long hxl_hc_count(int form) {
  Fp4 A[3];
  for (int q = 0; q < 3; ++q) A[q] = {{fp_one(), fp_one()}, {fp_one(), fp_one()}};
  const Fp2 l = {fp_one(), fp_one()};
  Fp4h R[3][2];
  tbg_mad_count = 0;
  if (form == 0) line_direct(A, l, l, l, R);
  else line_kara(A, l, l, l, R);
  return tbg_mad_count;
}

// fp_mul_sum's column check on a sum of a b products (bls_field.h)
int hxl_hc_columns_fit(double ab_products) { return fp_columns_fit(ab_products) ? 1 : 0; }

// the lazy negation's limbs (16p - a, unnormalised)
int hxl_hc_neg_l(const uint32_t* a, uint32_t* out) {
  const Fp r = fp_neg_l(ld(a));
  for (int i = 0; i < NL; ++i) out[i] = r.l[i];
  return 0;
}
}
