// TEST TOOLING ONLY: host (CPU) twin of the batched subgroup test's paired
// schedule (charon_amd/csrc/k_sgb.hip, bls_sgb.h sgb_pair_*) for
// tests/test_sgb_pair_host.py, lane pairs emulated (Fp2p), with the value
// bound checks (TBG_BOUNDS_CHECK) switched on.  Modelled on tests/hostcheck.
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

constexpr int K = 18, PAIRS = 9, MAX_N = 1024;

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

// sgb_pair_code of two digits (bucket index | negated << 7, 0xFF for (0, 0))
uint32_t sp_code(int32_t c0, int32_t c1) { return sgb_pair_code(c0, c1); }

// The paired schedule on one group: the n 96-byte signatures of partials
// i0 .. i0 + n - 1 decoded WITHOUT the subgroup check (a decode failure
// leaves the partial out, as in the kernels); per pair of combinations the 84
// bucket sums in member order (k_sgb_bucket), the 12 sums R_a, D_v
// (k_sgb_fold) and the two running sums (k_sgb_combine) by the kernels' own
// templates -- additions without the doubling branch, a sum that met equal
// operands redone with the complete formulas -- then psi(Q_k) == [x] Q_k.
// q18x96 (may be null) receives the 18 sums Q_k compressed.  Returns the bit
// mask of the combinations that failed (-1: bad argument); *n_redo (may be
// null) counts the sums that were redone; redo = 0 is the control: a sum that
// met equal operands then fails its combination.
int sp_group(const uint8_t* sigs96, int n, const uint32_t* seed8, uint32_t i0, int redo, int* n_redo,
             uint8_t* q18x96) {
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
  int mask = 0, redone = 0;
  for (int p = 0; p < PAIRS; ++p) {
    std::vector<Jac<Fp2p>> bk(SGBP_B, jac_inf<Fp2p>());
    for (int i = 0; i < n; ++i) {
      if (!ok[i]) continue;
      const uint32_t cd = sgb_pair_code(dig[(size_t)i * K + 2 * p], dig[(size_t)i * K + 2 * p + 1]);
      if (cd == SGBP_NONE) continue;
      Aff<Fp2p> s{pp_from(pts[i].x), f_reduce(pp_from(pts[i].y))};
      if (cd >> 7) s.y = f_reduce(f_neg(s.y));
      bk[cd & 0x7Fu] = jac_add_aff_in(bk[cd & 0x7Fu], s);
    }
    bool failed[2] = {false, false};
    Jac<Fp2p> sums[SGBP_SUMS];
    auto bucket = [&](uint32_t idx) { return bk[idx]; };
    for (uint32_t j = 0; j < SGBP_SUMS; ++j) {
      bool exc = false;
      sums[j] = sgb_pair_sum_g<Fp2p, true>(bucket, j, exc);
      if (exc && redo) { sums[j] = sgb_pair_sum_g<Fp2p, false>(bucket, j, exc); ++redone; }
      else if (exc) failed[j / SGBP_V] = true;
    }
    for (int h = 0; h < 2; ++h) {
      bool exc = false;
      auto ld = [&](uint32_t v) { return sums[SGBP_V * h + v]; };
      Jac<Fp2p> q = sgb_running_sums_g<Fp2p, true>(ld, SGBP_V, exc);
      if (exc && redo) { q = sgb_running_sums_g<Fp2p, false>(ld, SGBP_V, exc); ++redone; }
      else if (exc) failed[h] = true;
      if (q18x96) put(q, q18x96 + 96 * (2 * p + h));
      if (failed[h] || !in_g2(q)) mask |= 1 << (2 * p + h);
    }
  }
  if (n_redo) *n_redo = redone;
  return mask;
}

// The reference the twin is compared with: Q_k = sum_i c_ik s_i over the
// same members, the multiples [1..6] s_i and every sum formed with the
// complete addition (jac_add: doubling and infinity cases included), no
// buckets.  q18x96 receives the 18 sums compressed; 0, or -1.
int sp_reference(const uint8_t* sigs96, int n, const uint32_t* seed8, uint32_t i0, uint8_t* q18x96) {
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
