// The RLC products [r_i] s_i (G2) of the failed groups' candidates, one lane
// per list entry for the Fp-level work and one lane PAIR for the G2 point work
// (bls_pair.h: halves the G2 state per lane so the kernel fits two waves per
// SIMD, which on gfx950 issue the multiply-adds ~1.7x faster than one).
//
//   phase 1, lane L owns list entry L: the G2 table's slope inversion batched
//            over the workgroup;
//   phase 2, lanes (2k, 2k+1) run the G2 table and its 15 doublings + 31
//            additions for entry 2k, then for 2k+1, with the Fp2
//            coordinates split over the pair and the owner's inverse and
//            digits handed over by DPP.
//
// Measured and rejected: separate G1 / pair-G2 kernels with inversion-free
// Jacobian tables (bls_rlc.h *_j) -- 446 spilled VGPRs in the pair kernel,
// 3.19 ms against 2.85 ms for the fused single-lane kernel.
#define TBG_ADD_DBL_INLINE 1
#ifndef TBG_SCHED_FENCE
#define TBG_SCHED_FENCE 1  // products in program order: fits the pair kernel in 256 VGPRs (bls_field.h)
#endif
#include "tbls_launch.h"
#include "bls_rlc.h"
#include "bls_pair.h"
#include "bls_batchinv.h"

namespace tbg {

// The pair-owner's Fp2 value (owner = the lane of parity j) in pair form:
// every lane sends the component its partner needs, the owner keeps its own.
__device__ __forceinline__ Fp2x px_from_owner(const Fp2& own, uint32_t j) {
  const uint32_t par = pair_par();
  const Fp recv = pair_xch(par ? own.c0 : own.c1);  // the partner's value, component par
  return {par == j ? (par ? own.c1 : own.c0) : recv};
}
__device__ __forceinline__ uint32_t u32_from_owner(uint32_t own, uint32_t j) {
  const uint32_t recv = pair_u32(own);
  return pair_par() == j ? own : recv;
}

// r_i s_i for the candidates of failed groups only (k_gmsm.hip: gm_list,
// CNT_LAZY entries), after the group checks; the G1 products and the key
// marks are made, the group's lead is gm_lead.  Lane L owns list entry
// base + L (its slope denominator in the workgroup's batched inversion), the
// lane pair runs the G2 products of its two entries (one entry per pair
// measured 4.7 vs 4.2 ms at 1 % invalid: the inversion amortised over half
// the partials).  No early return inside the loop: both lanes of every pair
// must reach the DPP exchanges and every thread the workgroup's batched
// inversion.  Grid-stride over the list with a workgroup-uniform trip count.
__global__ void __launch_bounds__(BINV_BLOCK, TBG_PAIR_WAVES) k_rlc_partial2_list(DevBatch B) {
  if (B.counters[CNT_L0_OK]) return;
  const uint32_t nl = B.counters[CNT_LAZY];
#pragma unroll 1
  for (uint32_t base = blockIdx.x * blockDim.x; base < nl; base += gridDim.x * blockDim.x) {
    const uint32_t t = base + threadIdx.x;
    const bool active = t < nl;
    const uint32_t i = active ? B.gm_list[t] : 0u;
    const bool lead = active && B.gm_lead[B.partial_duty[i] / B.rlc_group] == i;
    const bool work = active && !lead;
    uint32_t a[4] = {0, 0, 0, 0};
    Fp2 dx2 = fp2_one();
    if (lead) {
      B.part_s[i] = jac_from_aff(B.sig_aff[i]);
    } else if (work) {
      rlc_digits(rlc_scalar(B.rlc_seed, i), a);
      const G2A s = B.sig_aff[i];
      dx2 = fp2_reduce(fp2_sub(fp2_mul(fp2_conj(s.x), fp2_from_const(PSI_X)), s.x));  // psi(s).x - s.x
    }
    const Fp2 inv2 = block_batch_inv2<BINV_WAVES>(dx2, work);  // every thread of the workgroup
    for (uint32_t j = 0; j < 2; ++j) {
      if (!u32_from_owner(work ? 1u : 0u, j)) continue;  // pair-uniform
      const uint32_t owner = u32_from_owner(i, j);  // the listed partial of the pair's lane j
      const Fp2x ix = px_from_owner(inv2, j);
      uint32_t u[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) u[k] = u32_from_owner(a[k], j);
      const Aff<Fp2x> s = px_load(B.sig_aff[owner]);
      const Aff<Fp2x> ps{f_mulc(f_conj(s.x), PSI_X), f_mulc(f_conj(s.y), PSI_Y)};  // psi(s) = [x] s
      Aff<Fp2x> ap, am;
      rlc_pair_from_inv(s, ps, ix, ap, am);
      px_store(B.part_s[owner], rlc_mul_table(ap, am, fp_from_const(PSI2_X), u));
    }
  }
}

void launch_rlc_partials_list(const DevBatch& B, const G1A* pk_aff, hipStream_t st) {
  (void)pk_aff;
  uint32_t blocks = (B.n_partials + BINV_BLOCK - 1) / BINV_BLOCK;
  if (blocks > 4096) blocks = 4096;
  if (blocks) TBG_KLAUNCH(k_rlc_partial2_list, dim3(blocks), dim3(BINV_BLOCK), st, B);
}

}  // namespace tbg
