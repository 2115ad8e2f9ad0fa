// Fused level 0's signature side as ONE ROLE of the key-side kernel's grid
// (k_rlc_g1_l0, k_msm.hip): in launches of at least l0_tail_partials partials
// (l0_tail, tbls_launch.h; smaller ones keep k_l0f_reduce / _fold / _horner)
// the first l0t_blocks() workgroups of that launch form
//   S = sum_j psi^j(2 A_j + T),  A_j = sum_e 13^e Qbar_(first_j + e)
// (bls_rlc.h, top) from the batched subgroup test's sums while every other
// workgroup runs the key side, so the chain below no longer stands alone on
// the launch's serial path with the machine idle.
//
// A block is one wave of L0T_PAIRS lane pairs.  Block b sums one chunk of
// L0T_CHUNK points of a column (the 18 columns Q_k over the groups, then the
// slices of T): L0T_PER points per pair, then a tree over the pairs.  The
// stages hand over by LAST ARRIVER only:
//   - every block stores its chunk sum, publishes it and adds 1 to its
//     column's counter; the block that draws chunks(col) - 1 sums the
//     column's chunk sums, stores the total, publishes it and adds 1 to the
//     columns-done counter;
//   - the block that draws L0T_COLS - 1 there runs the Horner steps, the tree
//     over j and S's affine conversion.
// No block polls or waits for another, so none depends on another being
// resident, and any dispatch order gives the same S.  Dependent additions:
// 4 + 5, then at most ceil(chunks / 32) + 5, then the Horner chain.
//
// The role does not read CNT_L0_BAD: the key role of the same launch sets it
// on ERR_PUBKEY while this one runs, so it is not uniform here, and a void
// launch costs the role the same as a clean one.  It only sets the flag when
// S is the point at infinity.
//
// The block function is written over an environment Env, so that the device
// (L0tDev, k_msm.hip: lanes, LDS tree, agent-scope publish / acquire) and the
// host tests (tests/l0tail: all pairs of a block in a loop, plain counters,
// TBG_BOUNDS_CHECK) run the same code:
//   Env::F                         the field type of one pair's value
//   Env::V                         one Jac<F> per lane pair of the block
//   V per_pair(n, f)               f(pr) for the pairs pr < n, infinity above
//   Jac<F> tree(v, n)              the sum of pairs [0, n) of v (pair 0's lanes)
//   Jac<F> load_q(g, col), load_t(a), load_sum(i)
//   void store_sum(i, p)           (pair 0's lanes store)
//   uint32_t arrive_col(col), arrive_done()   publish this block's stores, then
//                                  the counter's value before this block's add
//   void acquire()                 before any load of another block's sums
//   void finish(S)                 S affine, or the flag when it is infinity
// Every addition is the complete one (jac_add: equal operands do occur, small
// multiples of one point), out of line: this body is a callee of kernels that
// must keep two waves per SIMD.
#pragma once
#include "bls_rlc.h"
#include "bls_pair.h"

namespace tbg {

constexpr uint32_t L0T_QCOLS = 18;               // the columns Q_k (SGB_K, tbls_launch.h)
constexpr uint32_t L0T_COLS = L0T_QCOLS + 1;     // then T
constexpr uint32_t L0T_PAIRS = 32, L0T_PER = 4;  // lane pairs per block (one wave), points per pair
constexpr uint32_t L0T_CHUNK = L0T_PAIRS * L0T_PER;

// n_sg subgroup groups with n_t slices of T each; wq / wt chunks per Q column / of T
struct L0tShape { uint32_t n_sg, n_t, wq, wt; };
TBG_HD uint32_t l0t_chunks(uint32_t points) { return (points + L0T_CHUNK - 1) / L0T_CHUNK; }
TBG_HD L0tShape l0t_shape(uint32_t n_sg, uint32_t n_t) { return {n_sg, n_t, l0t_chunks(n_sg), l0t_chunks(n_sg * n_t)}; }
TBG_HD uint32_t l0t_blocks(const L0tShape& s) { return L0T_QCOLS * s.wq + s.wt; }
// l0f_sum: the chunk sums by block, then the L0T_COLS column totals
TBG_HD uint32_t l0t_sum_entries(const L0tShape& s) { return l0t_blocks(s) + L0T_COLS; }

// The Horner step 13 acc + q and the term psi^j(2 A + T) of bls_pair.h
// (l0f_mul13_add, l0f_term) through the out-of-line addition and doubling:
// the same formulas, so the same values.
template <class F>
TBG_HD Jac<F> l0t_mul13_add(const Jac<F>& acc, const Jac<F>& q) {
  Jac<F> t = jac_add(jac_dbl(acc), acc);  // 3 acc
  t = jac_add(jac_dbl(jac_dbl(t)), acc);  // 13 acc
  return jac_add(t, q);
}
template <class F>
TBG_HD Jac<F> l0t_term(const Jac<F>& A, const Jac<F>& T, int j) {
  Jac<F> r = jac_add(jac_dbl(A), T);
  for (int k = 0; k < j; ++k) r = g2_psi_g(r);
  return r;
}

template <class Env>
TBG_HD void l0t_block(Env& env, const L0tShape& sh, uint32_t b) {
  using F = typename Env::F;
  using P = Jac<F>;
  // this block's chunk of its column
  const bool qcol = b < L0T_QCOLS * sh.wq;
  const uint32_t col = qcol ? b / sh.wq : L0T_QCOLS, chunk = qcol ? b % sh.wq : b - L0T_QCOLS * sh.wq;
  const uint32_t count = qcol ? sh.n_sg : sh.n_sg * sh.n_t;
  typename Env::V v = env.per_pair(L0T_PAIRS, [&](uint32_t pr) {
    const uint32_t a0 = chunk * L0T_CHUNK + pr * L0T_PER;
    P acc = jac_inf<F>();
#pragma unroll 1
    for (uint32_t a = a0; a < a0 + L0T_PER && a < count; ++a)  // (pair-uniform)
      acc = jac_add(acc, qcol ? env.load_q(a, col) : env.load_t(a));
    return acc;
  });
  env.store_sum(b, env.tree(v, L0T_PAIRS));
  const uint32_t n_chunks = qcol ? sh.wq : sh.wt;
  if (env.arrive_col(col) != n_chunks - 1) return;

  // last of its column: the column's total
  env.acquire();
  const uint32_t first = qcol ? col * sh.wq : L0T_QCOLS * sh.wq;
  v = env.per_pair(L0T_PAIRS, [&](uint32_t pr) {
    P acc = jac_inf<F>();
#pragma unroll 1
    for (uint32_t a = pr; a < n_chunks; a += L0T_PAIRS) acc = jac_add(acc, env.load_sum(first + a));
    return acc;
  });
  const uint32_t tot = l0t_blocks(sh);
  env.store_sum(tot + col, env.tree(v, L0T_PAIRS));
  if (env.arrive_done() != L0T_COLS - 1) return;

  // last of all: one pair per j runs A_j's Horner steps and psi^j(2 A_j + T)
  env.acquire();
  v = env.per_pair(4, [&](uint32_t j) {
    const int e0 = l0f_first((int)j), e1 = l0f_first((int)j + 1);
    P acc = env.load_sum(tot + (uint32_t)e1 - 1);
#pragma unroll 1
    for (int e = e1 - 2; e >= e0; --e) acc = l0t_mul13_add(acc, env.load_sum(tot + (uint32_t)e));  // (pair-uniform)
    return l0t_term(acc, env.load_sum(tot + L0T_QCOLS), (int)j);
  });
  env.finish(env.tree(v, 4));
}

}  // namespace tbg
