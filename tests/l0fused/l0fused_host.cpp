// TEST TOOLING ONLY: host (CPU) build of the fused level 0's math
// (charon_amd/csrc/bls_rlc.h l0f_*, bls_pair.h l0f_mul13_add / l0f_term) for
// tests/test_l0_fused_host.py, lane pairs emulated (Fp2p), with the value
// bound checks (TBG_BOUNDS_CHECK) switched on.  Modelled on tests/hostcheck.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../charon_amd/csrc/bls_pairing.h"
#include "../../charon_amd/csrc/bls_h2c.h"
#include "../../charon_amd/csrc/bls_rlc.h"
#include "../../charon_amd/csrc/bls_pair.h"

extern "C" unsigned long long tbg_mad_count = 0;

using namespace tbg;

extern "C" {

// digits of partial i under the seed (sgb_digits)
void l0f_hc_digits(const uint32_t* seed8, uint32_t i, int32_t* out18) {
  uint32_t seed[8];
  for (int k = 0; k < 8; ++k) seed[k] = seed8[k];
  int32_t c[18];
  sgb_digits(seed, i, c);
  for (int k = 0; k < 18; ++k) out18[k] = c[k];
}

// n digit vectors (18 each) -> a_j (4 each) and u_j (4 each)
void l0f_hc_scalars(const int32_t* c18, uint32_t n, int32_t* a4, uint32_t* u4) {
  for (uint32_t i = 0; i < n; ++i) {
    int32_t c[18], a[4];
    uint32_t u[4];
    for (int k = 0; k < 18; ++k) c[k] = c18[18ull * i + k];
    l0f_scalar(c, a);
    l0f_digits(c, u);
    for (int j = 0; j < 4; ++j) {
      a4[4ull * i + j] = a[j];
      u4[4ull * i + j] = u[j];
    }
  }
}

// [r_i] pk by the 10 + 8 windows of the key's table (built entry by entry as
// k_pubkey_tables does), compressed; returns 0, or a negative error
int l0f_hc_g1(const uint8_t* pk48, const int32_t* c18, uint8_t* out48) {
  G1A pk;
  if (g1_decompress(pk48, pk) != DEC_OK) return -1;
  G1A xpk;
  if (!jac_to_aff(jac_neg(jac_mul_xabs(jac_from_aff(pk))), xpk)) return -2;
  G1A tab[PK_TAB_W2];
  for (int k = 0; k < (int)PK_TAB_W2; ++k)
    if (!jac_to_aff(rlc_key_table_w2_entry(pk, xpk, k), tab[k])) return -2;
  int32_t c[18];
  for (int k = 0; k < 18; ++k) c[k] = c18[k];
  uint32_t u[4];
  l0f_digits(c, u);
  G1A r;
  const bool fin = jac_to_aff(rlc_mul_key_l0f(tab, fp_from_const(G1_BETA), u), r);
  g1_compress(r, !fin, out48);
  return 0;
}

// S of n G2 points in subgroup groups of m (partials i0 .. i0 + n - 1 under
// the seed): per group the 18 sums Q_k = sum c_ik s_i and the plain sum T,
// added over the groups, then the Horner form S = sum_j psi^j(2 A_j + T)
// exactly as k_l0f_horner runs it.  Compressed; 0, or a negative error.
int l0f_hc_g2(const uint8_t* sigs96, uint32_t n, uint32_t m, const uint32_t* seed8, uint32_t i0, uint8_t* out96) {
  if (!m) return -1;
  uint32_t seed[8];
  for (int k = 0; k < 8; ++k) seed[k] = seed8[k];
  std::vector<Jac<Fp2p>> col(19, jac_inf<Fp2p>());
  for (uint32_t g0 = 0; g0 < n; g0 += m) {
    Jac<Fp2p> q[19];
    for (auto& x : q) x = jac_inf<Fp2p>();
    for (uint32_t i = g0; i < n && i < g0 + m; ++i) {
      G2A s;
      if (g2_decompress(sigs96 + 96ull * i, s) != DEC_OK) return -2;
      int32_t c[18];
      sgb_digits(seed, i0 + i, c);
      const Aff<Fp2p> p{pp_from(s.x), f_reduce(pp_from(s.y))};
      const Aff<Fp2p> np{p.x, f_reduce(f_neg(p.y))};
      for (int k = 0; k < 18; ++k)
        for (int r = 0; r < (c[k] < 0 ? -c[k] : c[k]); ++r) q[k] = jac_add_aff_in(q[k], c[k] < 0 ? np : p);
      q[18] = jac_add_aff_in(q[18], p);
    }
    for (int k = 0; k < 19; ++k) col[k] = jac_add_in<Fp2p, true>(col[k], q[k]);
  }
  Jac<Fp2p> S = jac_inf<Fp2p>();
  for (int j = 0; j < 4; ++j) {
    const int e0 = l0f_first(j), e1 = l0f_first(j + 1);
    Jac<Fp2p> acc = col[e1 - 1];
    for (int e = e1 - 2; e >= e0; --e) acc = l0f_mul13_add(acc, col[e]);
    S = jac_add_in<Fp2p, true>(S, l0f_term(acc, col[18], j));
  }
  G2A a{};
  bool fin = !jac_is_inf(S);
  if (fin) {
    const Fp2p zi = f_inv(S.Z), zi2 = f_sqr(zi);
    a = G2A{pp_to(f_mul(S.X, zi2)), pp_to(f_mul(S.Y, f_mul(zi2, zi)))};
  }
  g2_compress(a, !fin, out96);
  return 0;
}

// Work-model probes (tools/count_work.py builds this file with TBG_COUNT_OPS):
// one item of k_rlc_g1_l0's fused product on a key table set up beforehand,
// and k_l0f_horner's whole chain on 19 copies of a point.
unsigned long long l0f_hc_count_get(void) { return tbg_mad_count; }
void l0f_hc_count_reset(void) { tbg_mad_count = 0; }
static G1A g_tab[PK_TAB_W2];
static G2A g_pt;
int l0f_hc_probe_setup(const uint8_t* pk48, const uint8_t* sig96) {
  G1A pk, xpk;
  if (g1_decompress(pk48, pk) != DEC_OK || g2_decompress(sig96, g_pt) != DEC_OK) return -1;
  if (!jac_to_aff(jac_neg(jac_mul_xabs(jac_from_aff(pk))), xpk)) return -2;
  for (int k = 0; k < (int)PK_TAB_W2; ++k)
    if (!jac_to_aff(rlc_key_table_w2_entry(pk, xpk, k), g_tab[k])) return -2;
  return 0;
}
int l0f_hc_probe_g1(const int32_t* c18) {
  int32_t c[18];
  for (int k = 0; k < 18; ++k) c[k] = c18[k];
  uint32_t u[4];
  l0f_digits(c, u);
  return jac_is_inf(rlc_mul_key_l0f(g_tab, fp_from_const(G1_BETA), u)) ? 1 : 0;
}
int l0f_hc_probe_horner(void) {
  Jac<Fp2p> q = jac_from_aff(Aff<Fp2p>{pp_from(g_pt.x), f_reduce(pp_from(g_pt.y))});
  q = jac_dbl_in(q);  // (a Jacobian point with Z != 1, as the column totals are)
  Jac<Fp2p> S = jac_inf<Fp2p>();
  for (int j = 0; j < 4; ++j) {
    Jac<Fp2p> acc = q;
    for (int e = l0f_first(j + 1) - 2; e >= l0f_first(j); --e) acc = l0f_mul13_add(acc, q);
    S = jac_add_in<Fp2p, true>(S, l0f_term(acc, q, j));
  }
  const Fp2p zi = f_inv(S.Z);
  return f_is_zero(f_mul(S.X, f_sqr(zi))) ? 1 : 0;
}

}  // extern "C"
