// The batched subgroup test's sums over a group's bucket (slice) sums
// (k_sgb.hip), written for any Fp2 representation so that the kernels (Fp2x,
// the lane pair) and the host twins (Fp2p: tests/hostcheck hc_sgb_group for
// the classic schedule, tests/sgbpair sp_group for the paired one,
// tests/sgbtri st_group for the triple one) run the same code.
//
// FAST = true adds with jac_add_x (bls_pair.h): no doubling branch, `exc` set
// when an addition met two equal operands, the result then unusable.  Equal
// operands are NOT rare here: with the highest non-empty bucket B_v the
// running sums hold run == q == B_v, and an empty bucket v - 1 adds them --
// a short last group has empty buckets almost surely -- and replayed
// (duplicated) signatures make equal slice and bucket sums.  So on `exc` the
// caller redoes that one sum with FAST = false, the complete formulas, out
// of line (the fast loop keeps its registers); a group of G2 points never
// fails for this reason.
#pragma once
#include "bls_pair.h"

namespace tbg {

template <class F, bool FAST>
TBG_HD Jac<F> sgb_add_g(const Jac<F>& p, const Jac<F>& q, bool& exc) {
  if constexpr (FAST) return jac_add_x(p, q, exc);
  else return jac_add(p, q);  // (complete; out-of-line calls on the device)
}

// The sum of a bucket's n_slices slice sums (k_sgb_fold); slice(sl) loads
// slice sl.
template <class F, bool FAST, class L>
TBG_HD Jac<F> sgb_fold_g(L&& slice, uint32_t n_slices, bool& exc) {
  Jac<F> acc = slice(0u);
#pragma unroll 1
  for (uint32_t sl = 1; sl < n_slices; ++sl) acc = sgb_add_g<F, FAST>(acc, slice(sl), exc);
  return acc;
}

// Q = sum_v v B_v over a combination's n_v folded buckets by running sums
// from the highest bucket down (k_sgb_combine); bucket(v) loads B_(v + 1).
template <class F, bool FAST, class L>
TBG_HD Jac<F> sgb_running_sums_g(L&& bucket, uint32_t n_v, bool& exc) {
  Jac<F> run = jac_inf<F>(), q = run;
#pragma unroll 1
  for (int v = (int)n_v; v >= 1; --v) {
    run = sgb_add_g<F, FAST>(run, bucket((uint32_t)(v - 1)), exc);
    q = sgb_add_g<F, FAST>(q, run, exc);
  }
  return q;
}

// ---- paired schedule (k_sgb.hip): buckets over two combinations' digits ----
// Member i of a group goes, for the pair p of combinations (2p, 2p + 1), into
// the bucket (a, b) = +-(c_i,2p, c_i,2p+1), the sign -- the member's point is
// negated with it -- chosen so that a > 0, or a = 0 and b > 0; (0, 0) is in
// no sum.  The 84 buckets of a pair: a = 0 with b = 1..6, then the rows
// a = 1..6 with b = -6..6.
constexpr uint32_t SGBP_V = 6;                           // digits -6..6
constexpr uint32_t SGBP_ROW = 2 * SGBP_V + 1;            // buckets of a row a >= 1
constexpr uint32_t SGBP_B = SGBP_V + SGBP_V * SGBP_ROW;  // buckets per pair
constexpr uint32_t SGBP_SUMS = 2 * SGBP_V;               // R_1..R_6, D_1..D_6
constexpr uint32_t SGBP_NONE = 0xFFu;                    // sgb_pair_code of (0, 0)
// (a, b) normalised as above -> the bucket's index in its pair
TBG_HD uint32_t sgb_pair_index(uint32_t a, int32_t b) {
  return a ? SGBP_V + (a - 1) * SGBP_ROW + (uint32_t)(b + (int32_t)SGBP_V) : (uint32_t)b - 1;
}
// digits (c0, c1) of a member -> bucket index | negated << 7, or SGBP_NONE
TBG_HD uint32_t sgb_pair_code(int32_t c0, int32_t c1) {
  if (!c0 && !c1) return SGBP_NONE;
  const bool neg = c0 < 0 || (!c0 && c1 < 0);
  return sgb_pair_index((uint32_t)(neg ? -c0 : c0), neg ? -c1 : c1) | (neg ? 0x80u : 0u);
}
// The pair's two combinations from its bucket sums B(a, b), as the classic
// schedule's folded buckets (k_sgb_fold; sgb_running_sums_g then gives
//   Q_2p = sum_a a R_a,  Q_2p+1 = sum_v v D_v):
//   sum j = a - 1 (a = 1..6):      R_a = sum_b B(a, b)
//   sum j = 6 + v - 1 (v = 1..6):  D_v = sum_(a = 0..6) B(a, v) - sum_(a = 1..6) B(a, -v)
// 13 terms each; bucket(idx) loads the pair's bucket idx.  Empty buckets
// (infinity) are common and handled by the additions; two equal operands
// set `exc` under FAST, as in the sums above.
template <class F, bool FAST, class L>
TBG_HD Jac<F> sgb_pair_sum_g(L&& bucket, uint32_t j, bool& exc) {
  Jac<F> acc = jac_inf<F>();
#pragma unroll 1
  for (uint32_t t = 0; t < SGBP_ROW; ++t) {
    uint32_t idx;
    bool neg = false;
    if (j < SGBP_V) {
      idx = sgb_pair_index(j + 1, (int32_t)t - (int32_t)SGBP_V);
    } else {
      const int32_t v = (int32_t)(j - SGBP_V) + 1;
      neg = t > SGBP_V;
      idx = t == 0 ? sgb_pair_index(0, v) : sgb_pair_index(neg ? t - SGBP_V : t, neg ? -v : v);
    }
    Jac<F> x = bucket(idx);
    if (neg) x = jac_neg(x);
    acc = sgb_add_g<F, FAST>(acc, x, exc);
  }
  return acc;
}

// ---- triple schedule (k_sgb.hip): buckets over three combinations' digits ----
// Member i of a group goes, for the triple t of combinations (3t, 3t + 1,
// 3t + 2), into the bucket (a, b, c) = +-(c_i,3t, c_i,3t+1, c_i,3t+2), the sign
// chosen so that the first non-zero digit is positive; (0, 0, 0) is in no sum.
// The (13^3 - 1) / 2 = 1,098 buckets of a triple: a = 0 holds a pair's 84
// buckets (b, c) in the pair's own order, then the planes a = 1..6 with
// (b, c) in -6..6 squared, c fastest.
constexpr uint32_t SGBT_B = SGBP_B + SGBP_V * SGBP_ROW * SGBP_ROW;  // buckets per triple
constexpr uint32_t SGBT_ESUMS = SGBP_V * 2 * (SGBP_V + 1);          // E(v, a, sign): 84
constexpr uint32_t SGBT_SUMS1 = SGBP_B + SGBT_ESUMS;                // the first pass's sums: P, then E
constexpr uint32_t SGBT_SUMS2 = 3 * SGBP_V;                         // R_1..6, D_1..6 of the pair, D_1..6 of the third
constexpr uint32_t SGBT_NEG = 1u << 11;                             // sgb_tri_code's sign bit
constexpr uint32_t SGBT_NONE = 0xFFFFFFFFu;                         // sgb_tri_code of (0, 0, 0)
static_assert(SGBT_B <= SGBT_NEG, "a bucket index fits under the sign bit");
// (a, b, c) normalised as above -> the bucket's index in its triple
TBG_HD uint32_t sgb_tri_index(uint32_t a, int32_t b, int32_t c) {
  return a ? SGBP_B + ((a - 1) * SGBP_ROW + (uint32_t)(b + (int32_t)SGBP_V)) * SGBP_ROW + (uint32_t)(c + (int32_t)SGBP_V)
           : sgb_pair_index((uint32_t)b, c);
}
// digits (c0, c1, c2) of a member -> bucket index | SGBT_NEG if negated, or SGBT_NONE
TBG_HD uint32_t sgb_tri_code(int32_t c0, int32_t c1, int32_t c2) {
  if (!c0 && !c1 && !c2) return SGBT_NONE;
  const bool neg = c0 < 0 || (!c0 && (c1 < 0 || (!c1 && c2 < 0)));
  return sgb_tri_index((uint32_t)(neg ? -c0 : c0), neg ? -c1 : c1, neg ? -c2 : c2) | (neg ? SGBT_NEG : 0u);
}
// The triple's three combinations from its bucket sums B(a, b, c) in two
// passes of chains of at most 14 terms (k_sgb_fold).  First pass, sum j:
//   j < 84:  P_j = sum_c B(a, b, c) for the pair bucket j = (a, b) -- the 13
//            consecutive buckets from 6 + 13 j (the six buckets (0, 0, c)
//            come first and belong to no P).  P is exactly the paired
//            schedule's bucket array of the combinations (3t, 3t + 1).
//   j = 84 + 14 (v - 1) + 2 a + s (v = 1..6, a = 0..6, s = 0, 1):
//            E = sum_b B(a, b, +v) (s = 0) or sum_b B(a, b, -v) (s = 1);
//            a = 0 has b = 0..6 (s = 0) or b = 1..6 (s = 1), a >= 1 has
//            b = -6..6.
// Second pass, sum j (bucket(idx) then loads the FIRST pass's sum idx):
//   j < 12:  the paired schedule's R_a, D_v over P (sgb_pair_sum_g)
//   j = 12 + v - 1:  D_v = sum_a (E(v, a, 0) - E(v, a, 1)), 14 terms,
//            Q_3t+2 = sum_v v D_v
// -- the 18 sums are the classic schedule's folded buckets of the three
// combinations, in order.
template <class F, bool FAST, class L>
TBG_HD Jac<F> sgb_tri_sum1_g(L&& bucket, uint32_t j, bool& exc) {
  Jac<F> acc = jac_inf<F>();
  const uint32_t e = j - SGBP_B;  // (j >= SGBP_B)
  const int32_t v = (int32_t)(e / (2 * (SGBP_V + 1))) + 1;
  const uint32_t a = (e % (2 * (SGBP_V + 1))) >> 1;
  const bool neg = e & 1u;
#pragma unroll 1
  for (uint32_t t = 0; t < SGBP_ROW; ++t) {
    uint32_t idx;
    if (j < SGBP_B) {
      idx = SGBP_V + SGBP_ROW * j + t;
    } else if (a) {
      idx = sgb_tri_index(a, (int32_t)t - (int32_t)SGBP_V, neg ? -v : v);
    } else {  // b = 0..6 with +v, b = 1..6 with -v
      if (t + (neg ? 1u : 0u) > SGBP_V) break;
      idx = sgb_tri_index(0, (int32_t)t + (neg ? 1 : 0), neg ? -v : v);
    }
    acc = sgb_add_g<F, FAST>(acc, bucket(idx), exc);
  }
  return acc;
}
template <class F, bool FAST, class L>
TBG_HD Jac<F> sgb_tri_sum2_g(L&& sum1, uint32_t j, bool& exc) {
  if (j < SGBP_SUMS) return sgb_pair_sum_g<F, FAST>(sum1, j, exc);
  Jac<F> acc = jac_inf<F>();
#pragma unroll 1
  for (uint32_t r = 0; r < 2 * (SGBP_V + 1); ++r) {
    Jac<F> x = sum1(SGBP_B + 2 * (SGBP_V + 1) * (j - SGBP_SUMS) + r);
    if (r & 1u) x = jac_neg(x);
    acc = sgb_add_g<F, FAST>(acc, x, exc);
  }
  return acc;
}

}  // namespace tbg
