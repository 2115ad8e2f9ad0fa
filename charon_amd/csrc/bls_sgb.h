// The batched subgroup test's sums over a group's bucket slices (k_sgb.hip),
// written for any Fp2 representation so that the kernels (Fp2x, the lane
// pair) and the host twin (Fp2p, tests/hostcheck hc_sgb_group) run the same
// code.
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

}  // namespace tbg
