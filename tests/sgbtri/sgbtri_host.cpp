// TEST TOOLING ONLY: host (CPU) twin of the batched subgroup test's triple
// schedule (charon_amd/csrc/k_sgb.hip, bls_sgb.h sgb_tri_*) for
// tests/test_sgb_tri_host.py, lane pairs emulated (Fp2p), with the value
// bound checks (TBG_BOUNDS_CHECK) switched on.  Modelled on tests/sgbpair.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../charon_amd/csrc/bls_pairing.h"
#include "../../charon_amd/csrc/bls_h2c.h"
#include "../../charon_amd/csrc/bls_rlc.h"
#include "../../charon_amd/csrc/bls_sgb.h"

extern "C" unsigned long long tbg_mad_count = 0;

using namespace tbg;

namespace {

constexpr int K = 18, TRIPLES = 6, MAX_N = 32768;

void put(const Jac<Fp2p>& q, uint8_t* out96) {
  G2A a{};
  const bool fin = !jac_is_inf(q);
  if (fin) {
    const Fp2p zi = f_inv(q.Z), zi2 = f_sqr(zi);
    a = G2A{pp_to(f_mul(q.X, zi2)), pp_to(f_mul(q.Y, f_mul(zi2, zi)))};
  }
  g2_compress(a, !fin, out96);
}

// psi(Q) == [x] Q as k_sgb_test decides it
bool in_g2(const Jac<Fp2p>& q) {
  if (jac_is_inf(q)) return true;
  bool exc = false;
  const Jac<Fp2p> m = jac_mul_xabs_x(q, exc);
  if (exc || jac_is_inf(m)) return false;
  const Jac<Fp2p> ps = g2_psi_g(q);
  const Fp2p z1 = f_sqr(ps.Z), z2 = f_sqr(m.Z);
  return f_eq(f_mul(ps.X, z2), f_mul(m.X, z1)) &&
         f_eq(f_mul(f_mul(ps.Y, m.Z), z2), f_reduce(f_neg(f_mul(f_mul(m.Y, ps.Z), z1))));
}

}  // namespace

extern "C" {

// sgb_tri_code of three digits (bucket index | negated << 11, 0xFFFFFFFF for (0, 0, 0))
uint32_t st_code(int32_t c0, int32_t c1, int32_t c2) { return sgb_tri_code(c0, c1, c2); }

// The triple schedule on one group: the n 96-byte signatures of partials
// i0 .. i0 + n - 1 decoded WITHOUT the subgroup check (a decode failure
// leaves the partial out, as in the kernels); per triple of combinations the
// 1,098 bucket sums in member order (k_sgb_bucket), the first pass's 168 sums
// P, E and the second's 18 sums R_a, D_v, D_v (k_sgb_tri_fold) and the three
// running sums (k_sgb_combine) by the kernels' own templates -- additions
// without the doubling branch, a sum that met equal operands redone with the
// complete formulas -- then psi(Q_k) == [x] Q_k.  q18x96 (may be null)
// receives the 18 sums Q_k compressed; *max_bucket (may be null) the members
// of the fullest bucket.  Returns the bit mask of the combinations that
// failed (-1: bad argument); *n_redo (may be null) counts the sums that were
// redone; redo = 0 is the control: a sum that met equal operands then fails
// the combinations it feeds.
int st_group(const uint8_t* sigs96, int n, const uint32_t* seed8, uint32_t i0, int redo, int* n_redo,
             uint8_t* q18x96, int* max_bucket) {
  if (n < 0 || n > MAX_N) return -1;
  uint32_t seed[8];
  for (int k = 0; k < 8; ++k) seed[k] = seed8[k];
  std::vector<G2A> pts(n);
  std::vector<uint8_t> ok(n);
  std::vector<int32_t> dig((size_t)n * K);
  for (int i = 0; i < n; ++i) {
    ok[i] = g2_decompress_t<false, false>(sigs96 + 96 * i, pts[i]) == DEC_OK;
    int32_t c[18];
    sgb_digits(seed, i0 + (uint32_t)i, c);
    for (int k = 0; k < K; ++k) dig[(size_t)i * K + k] = c[k];
  }
  int mask = 0, redone = 0, fullest = 0;
  for (int t = 0; t < TRIPLES; ++t) {
    std::vector<Jac<Fp2p>> bk(SGBT_B, jac_inf<Fp2p>());
    std::vector<int> cnt(SGBT_B, 0);
    for (int i = 0; i < n; ++i) {
      if (!ok[i]) continue;
      const int32_t* d = &dig[(size_t)i * K + 3 * t];
      const uint32_t cd = sgb_tri_code(d[0], d[1], d[2]);
      if (cd == SGBT_NONE) continue;
      const uint32_t b = cd & (SGBT_NEG - 1);
      if (b >= SGBT_B) return -1;
      Aff<Fp2p> s{pp_from(pts[i].x), f_reduce(pp_from(pts[i].y))};
      if (cd & SGBT_NEG) s.y = f_reduce(f_neg(s.y));
      bk[b] = jac_add_aff_in(bk[b], s);
      if (++cnt[b] > fullest) fullest = cnt[b];
    }
    // which combinations of the triple a first-pass sum feeds: P both of the
    // pair's, E the third
    bool failed[3] = {false, false, false};
    std::vector<Jac<Fp2p>> s1(SGBT_SUMS1);
    auto bucket = [&](uint32_t idx) { return bk.at(idx); };
    for (uint32_t j = 0; j < SGBT_SUMS1; ++j) {
      bool exc = false;
      s1[j] = sgb_tri_sum1_g<Fp2p, true>(bucket, j, exc);
      if (exc && redo) { s1[j] = sgb_tri_sum1_g<Fp2p, false>(bucket, j, exc); ++redone; }
      else if (exc) { if (j < SGBP_B) failed[0] = failed[1] = true; else failed[2] = true; }
    }
    Jac<Fp2p> s2[SGBT_SUMS2];
    auto sum1 = [&](uint32_t idx) { return s1.at(idx); };
    for (uint32_t j = 0; j < SGBT_SUMS2; ++j) {
      bool exc = false;
      s2[j] = sgb_tri_sum2_g<Fp2p, true>(sum1, j, exc);
      if (exc && redo) { s2[j] = sgb_tri_sum2_g<Fp2p, false>(sum1, j, exc); ++redone; }
      else if (exc) failed[j / SGBP_V] = true;
    }
    for (int h = 0; h < 3; ++h) {
      bool exc = false;
      auto ld = [&](uint32_t v) { return s2[SGBP_V * h + v]; };
      Jac<Fp2p> q = sgb_running_sums_g<Fp2p, true>(ld, SGBP_V, exc);
      if (exc && redo) { q = sgb_running_sums_g<Fp2p, false>(ld, SGBP_V, exc); ++redone; }
      else if (exc) failed[h] = true;
      if (q18x96) put(q, q18x96 + 96 * (3 * t + h));
      if (failed[h] || !in_g2(q)) mask |= 1 << (3 * t + h);
    }
  }
  if (n_redo) *n_redo = redone;
  if (max_bucket) *max_bucket = fullest;
  return mask;
}

// The reference the twin is compared with: Q_k = sum_i c_ik s_i over the
// same members, the multiples [1..6] s_i and every sum formed with the
// complete addition (jac_add: doubling and infinity cases included), no
// buckets.  q18x96 receives the 18 sums compressed; 0, or -1.
int st_reference(const uint8_t* sigs96, int n, const uint32_t* seed8, uint32_t i0, uint8_t* q18x96) {
  if (n < 0 || n > MAX_N || !q18x96) return -1;
  uint32_t seed[8];
  for (int k = 0; k < 8; ++k) seed[k] = seed8[k];
  Jac<Fp2p> q[K];
  for (auto& x : q) x = jac_inf<Fp2p>();
  for (int i = 0; i < n; ++i) {
    G2A s;
    if (g2_decompress_t<false, false>(sigs96 + 96 * i, s) != DEC_OK) continue;
    int32_t c[18];
    sgb_digits(seed, i0 + (uint32_t)i, c);
    Jac<Fp2p> mult[7];
    mult[0] = jac_inf<Fp2p>();
    mult[1] = jac_from_aff(Aff<Fp2p>{pp_from(s.x), f_reduce(pp_from(s.y))});
    for (int v = 2; v <= 6; ++v) mult[v] = jac_add(mult[v - 1], mult[1]);
    for (int k = 0; k < K; ++k) {
      const Jac<Fp2p>& t = mult[c[k] < 0 ? -c[k] : c[k]];
      q[k] = jac_add(q[k], c[k] < 0 ? jac_neg(t) : t);
    }
  }
  for (int k = 0; k < K; ++k) put(q[k], q18x96 + 96 * k);
  return 0;
}

}  // extern "C"
