// Level 0 of the RLC schedule: the whole device batch (every caller batch
// packed into one launch) as ONE product check
//   prod_d e(P_d, H(m_d)) * e(-g1, S) == 1,  P_d = sum_i r_i pk_i,  S = sum_i r_i s_i,
// before any group check (reference: the per-partial CoreVerify calls of
// tbls.Verify / VerifyAndAggregate, tbls/tss.go:153-197, all of which a pass
// accepts; any failure falls through to the group levels of k_rlc.hip, so
// every verdict stays the exact per-item one).
//
// The signature side is the bucket MSM of bls_msm.h: 4 mixed additions per
// partial instead of a 64-bit G2 scalar multiplication (15 doublings, 31
// additions and a field inversion per partial at the group levels); the key
// side uses per-key window tables (bls_rlc.h rlc_mul_key_w2) computed once
// when the key table is loaded, so P_d needs no inversion per partial either.
//
//   k_rlc_g1_l0      one lane per partial: r_i, [r_i] pk_i, bucket sizes
//   k_msm_scan       bucket offsets (one workgroup)
//   k_msm_scatter    bucket entries
//   k_msm_bucket_part  one lane PAIR per quarter of a bucket: its sum
//   k_msm_bucket     one lane PAIR per bucket: the quarters' sum times (2j + 1)
//   k_msm_tree, k_msm_tree_final  the sum of the scaled buckets (LDS trees), S affine
// While the batched subgroup test runs for the launch (l0_fused, tbls_launch.h)
// the k_msm_* kernels do not run: r_i is a form of the partial's subgroup
// digits (bls_rlc.h, top) and S comes from that test's sums, formed by the
// first workgroups of k_rlc_g1_l0's own grid -- see "the S role" below -- or, in
// launches too small to hide it there, by k_l0f_reduce, k_l0f_fold, k_l0f_horner.
#define TBG_ADD_DBL_INLINE 1
#ifndef TBG_SCHED_FENCE
#define TBG_SCHED_FENCE 1  // products in program order: fits the pair kernels in 256 VGPRs (bls_field.h)
#endif
#include "tbls_launch.h"
#include "bls_msm.h"
#include "bls_pair.h"
#include "bls_batchinv.h"
#include "bls_l0tail.h"

namespace tbg {

// ------------------------------------------------------------ the S role
// Fused level 0's signature side (bls_l0tail.h): S from the batched subgroup
// test's sums -- the 18 columns Qbar_k = sum over the groups of Q_k
// (k_sgb_combine left Q_k in the first slot of combination k's buckets,
// k_sgb_test proved it in G2) and the column T (k_sgb_bucket's slice sums).
// In a fused launch of at least l0_tail_partials partials (l0_tail,
// tbls_launch.h) the key-side grid below starts with l0f_s_blocks()
// workgroups that run l0f_s_role and return; every other workgroup runs the
// key side on blockIdx.x - n_s.  The role reads nothing the key side writes
// and writes only l0f_sum, its counters, batch_pt and (S = 0) CNT_L0_BAD.
// A failed subgroup group voids level 0 (its Q_k are not in G2 and its
// members are about to be tested alone: k_sgb.hip sets the flag with
// sgb_bad), as does a key mark and S = 0; the role runs all the same.
//
// Hand-off between workgroups, which run on different XCDs with private L2s:
// plain stores, the wave's s_waitcnt vmcnt(0), lane 0's agent-scope release
// fence, s_waitcnt vmcnt(0) again, then a relaxed agent-scope fetch_add; the
// last arriver runs an agent-scope acquire fence, s_waitcnt vmcnt(0) and the
// workgroup barrier before it loads another workgroup's sums.
static_assert(L0T_QCOLS == SGB_K && L0T_COLS == L0F_COLS && L0T_PAIRS == L0F_PAIRS && L0T_PER == L0F_PER,
              "bls_l0tail.h: the chunking of tbls_launch.h");
struct L0tDev {
  using F = Fp2x;
  using V = Jac<Fp2x>;
  const G2J* sgb_part;
  const G2J* sgb_t;
  G2J* sum;
  uint32_t* counters;
  G2A* batch_pt;
  uint32_t sgb_m, sgb_split;
  Jac<Fp2x>* lds;  // [kBlock]

  template <class Fn>
  TBG_DEV V per_pair(uint32_t n, Fn&& f) const {
    const uint32_t pr = threadIdx.x >> 1;
    V acc = jac_inf<Fp2x>();
    if (pr < n) acc = f(pr);
    return acc;
  }
  // (every lane of the wave calls it; the barrier is the one wave's own)
  TBG_DEV V tree(V acc, uint32_t n) const {
    const uint32_t t = threadIdx.x, pr = t >> 1;
#pragma unroll 1
    for (uint32_t s = 1; s < n; s <<= 1) {
      lds[t] = acc;
      __syncthreads();
      if ((pr & (2 * s - 1)) == 0 && pr + s < n) {
        const V o = lds[t + 2 * s];
        acc = jac_add(acc, o);
      }
      __syncthreads();
    }
    return acc;
  }
  TBG_DEV V load_q(uint32_t g, uint32_t col) const { return px_load(sgb_part[sgb_q_slot(sgb_m, sgb_split, g, col)]); }
  TBG_DEV V load_t(uint32_t a) const { return px_load(sgb_t[a]); }
  TBG_DEV V load_sum(uint32_t i) const { return px_load(sum[i]); }
  TBG_DEV void store_sum(uint32_t i, const V& p) const {
    if ((threadIdx.x >> 1) == 0) px_store(sum[i], p);
  }
  TBG_DEV uint32_t arrive(uint32_t* counter) const {
    __asm__ __volatile__("s_waitcnt vmcnt(0)" ::: "memory");  // the storing wave (there is one)
    uint32_t ticket = 0;
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      __asm__ __volatile__("s_waitcnt vmcnt(0)" ::: "memory");  // (the compiler may drop the fence's own wait)
      ticket = __hip_atomic_fetch_add((__attribute__((address_space(1))) uint32_t*)counter, 1u, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);  // (a global access, not a flat one)
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)ticket);
  }
  TBG_DEV uint32_t arrive_col(uint32_t col) const { return arrive(counters + CNT_L0F_COL + col); }
  TBG_DEV uint32_t arrive_done() const { return arrive(counters + CNT_L0F_DONE); }
  TBG_DEV void acquire() const {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    __asm__ __volatile__("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  TBG_DEV void finish(const V& S) const {
    if ((threadIdx.x >> 1) != 0) return;
    if (jac_is_inf(S)) {
      if (pair_par() == 0) counters[CNT_L0_BAD] = 1;  // S = 0: no lines; the group levels decide
      return;
    }
    const Fp2x zi = f_inv(S.Z);
    const Fp2x zi2 = f_sqr(zi);
    px_store(*batch_pt, Aff<Fp2x>{f_mul(S.X, zi2), f_mul(S.Y, f_mul(zi2, zi))});
  }
};

// Out of line: its registers and spills stay its own, the key role's code is
// what it was.  (Block-uniform: a whole workgroup is in the role or not.)
__device__ __noinline__ void l0f_s_role(const G2J* sgb_part, const G2J* sgb_t, G2J* sum, uint32_t* counters,
                                        G2A* batch_pt, uint32_t sgb_m, uint32_t sgb_split, uint32_t n_sg) {
  __shared__ Jac<Fp2x> lds[kBlock];
  L0tDev env{sgb_part, sgb_t, sum, counters, batch_pt, sgb_m, sgb_split, lds};
  l0t_block(env, l0t_shape(n_sg, sgb_t_slices(sgb_m)), blockIdx.x);
}
// true: this workgroup was one of the launch's n_s S-role workgroups and is done
TBG_DEV bool l0f_s_block(const DevBatch& B, uint32_t n_s) {
  if (blockIdx.x >= n_s) return false;
  TBG_URGENT();  // a few waves with a long chain beside thousands of key waves
  l0f_s_role(B.sgb_part, B.sgb_t, B.l0f_sum, B.counters, B.batch_pt, B.sgb_m, B.sgb_split,
             sgb_groups(B.n_partials, B.sgb_m));
  return true;
}

// Table of every usable key (k_rlc_g1_l0, k_rlc_g1): the window table of
// bls_rlc.h (e0 pk + e1 [x]pk, e0 in {1, 3}, e1 in {+-1, +-3}), each entry's
// affine conversion batched over the workgroup (bls_batchinv.h).
__global__ void __launch_bounds__(BINV_BLOCK) k_pubkey_tables(const G1A* pk, const G1A* xpk, const int32_t* status,
                                                              uint32_t n, G1A* tab) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n;
  const bool ok = in && status[i] == DEC_OK;
  G1A p0{fp_zero(), fp_zero()}, x0 = p0;
  if (ok) {
    p0 = pk[i];
    x0 = xpk[i];
  }
  // e0 pk + e1 [x]pk is never the identity for a prime-order key (it would
  // need x = -e0 / e1 mod r); every thread runs every batched conversion
#pragma unroll 1
  for (int k = 0; k < (int)PK_TAB; ++k) {
    const G1J e = ok ? rlc_key_table_w2_entry(p0, x0, k) : jac_inf<Fp>();
    G1A a{fp_zero(), fp_zero()};
    const bool got = block_jac_to_aff<BINV_WAVES>(e, ok, a);
    if (in) tab[(size_t)PK_TAB * i + k] = got ? a : G1A{fp_zero(), fp_zero()};
  }
}

// Level-0 G1 side, one lane per partial: unusable keys are marked, every
// candidate's r_i is drawn (no group lead: at level 0 two r = 1 partials of
// different groups could cancel) and [r_i] pk_i computed from the key's window
// table; the four digits count into their buckets.
// (Fused launches of at least l0_duty_partials partials run l0duty::k_rlc_g1_l0
// below instead.)  The first n_s workgroups of a fused launch run the S role
// (0 without the batched subgroup test: the bucket MSM below forms S).
__global__ void TBG_LAUNCH_N(TBG_PAIR_WAVES) k_rlc_g1_l0(DevBatch B, const G1A* tab, const int32_t* pk_status,
                                                          uint32_t n_pk, uint32_t n_s) {
  if (l0f_s_block(B, n_s)) return;
  const uint32_t i = (blockIdx.x - n_s) * blockDim.x + threadIdx.x;
  if (i >= B.n_partials || B.partial_status[i] != TBG_PS_NOT_VERIFIED) return;
  const uint32_t pid = B.pubkey_ids[i];
  const bool fused = l0_fused(B);
  if (pid >= n_pk || pk_status[pid] != DEC_OK) {
    B.partial_status[i] = TBG_PS_ERR_PUBKEY;
    if (fused) B.counters[CNT_L0_BAD] = 1;  // the fused S holds this partial: level 0 is void
    return;
  }
  if (fused) {  // r_i from the subgroup digits (k_sgb_sort stored its u_j): nothing kept for an MSM
    const uint4 v = *(const uint4*)(B.l0f_u + 4ull * i);
    const uint32_t uf[4] = {v.x, v.y, v.z, v.w};
    B.part_p[i] = rlc_mul_key_l0f(tab + (size_t)PK_TAB * pid, fp_from_const(G1_BETA), uf);
    return;
  }
  const uint64_t r = rlc_scalar(B.rlc_seed, i);
  uint32_t u[4];
  rlc_digits(r, u);
  B.msm_r[i] = r;
  B.part_p[i] = rlc_mul_key(tab + (size_t)PK_TAB * pid, u);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    bool neg;
    atomicAdd(&B.msm_off[msm_bucket(u[k], neg)], 1u);
  }
}

// Level-0 G1 side of a fused launch of at least l0_duty_partials partials
// (l0_per_duty): a kernel of its own behind the same profile name, so that
// the per-partial kernel above compiles as it always did.  One lane per
// DUTY: the key marks of the duty's partials, then P_d in Straus' joint form
// over its candidates (rlc_duty_keys_l0f: the 18 doublings once per duty, not
// once per candidate; part_p is not written), its affine conversion batched
// over the workgroup, and dv_p / dv_state as k_rlc_duty_sum<DSUM_L0_P> writes
// them -- that kernel is not launched then.  (Two lanes per duty, each with
// every second partial and one Jacobian addition to join them, measured a
// smaller headline gain: DESIGN section 6-r11.)
// A duty has no bound on its partials, so the candidates' ids and digits are
// read again in every window (one uint4 and two words per candidate, beside
// its two table entries).
namespace l0duty {
static_assert(BINV_BLOCK == kBlock, "k_rlc_g1_l0: the workgroup of the batched inversion");
__global__ void TBG_LAUNCH_N(TBG_PAIR_WAVES) k_rlc_g1_l0(DevBatch B, const G1A* tab, const int32_t* pk_status,
                                                          uint32_t n_pk, uint32_t n_s) {
  if (l0f_s_block(B, n_s)) return;  // (before the workgroup's batched inversion: block-uniform)
  const uint32_t d = (blockIdx.x - n_s) * blockDim.x + threadIdx.x;
  const bool in = d < B.n_duties;
  uint32_t i0 = 0, n = 0, cand = 0;
  if (in) {
    i0 = B.duty_first[d];
    n = B.duty_first[d + 1] - i0;
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t i = i0 + k;
      if (B.partial_status[i] != TBG_PS_NOT_VERIFIED) continue;
      const uint32_t pid = B.pubkey_ids[i];
      if (pid >= n_pk || pk_status[pid] != DEC_OK) {
        B.partial_status[i] = TBG_PS_ERR_PUBKEY;
        B.counters[CNT_L0_BAD] = 1;  // the fused S holds this partial: level 0 is void
        continue;
      }
      ++cand;
    }
  }
  G1J P = jac_inf<Fp>();
  if (cand)
    P = rlc_duty_keys_l0f<Fp>(n, fp_from_const(G1_BETA), [&](uint32_t k, const G1A*& e, uint32_t (&u)[4]) {
      const uint32_t i = i0 + k;
      if (B.partial_status[i] != TBG_PS_NOT_VERIFIED) return false;  // (this lane's own marks included)
      e = tab + (size_t)PK_TAB * B.pubkey_ids[i];
      const uint4 v = *(const uint4*)(B.l0f_u + 4ull * i);
      u[0] = v.x;
      u[1] = v.y;
      u[2] = v.z;
      u[3] = v.w;
      return true;
    });
  G1A Pa;
  const bool aff = block_jac_to_aff<BINV_WAVES>(P, cand > 0, Pa);  // every thread of the workgroup
  if (!in) return;
  if (cand == 0) {
    B.dv_state[d] = RLC_NONE;
    return;
  }
  if (!aff) {
    B.dv_state[d] = RLC_EACH;  // degenerate combination: check the partials one by one
    B.counters[CNT_L0_BAD] = 1;
    return;
  }
  B.dv_p[d] = G1A{fp_reduce(fp_neg(Pa.x)), Pa.y};  // (-x, y): the Miller steps' evaluation operands
  B.dv_state[d] = RLC_COMBINED;
}
}  // namespace l0duty

// Exclusive scan of the bucket sizes into offsets (msm_off) and cursors
// (msm_cur): one workgroup of 1024 lanes, 32 buckets per lane.
constexpr int kScanBlock = 1024;
__global__ void __launch_bounds__(kScanBlock) k_msm_scan(DevBatch B) {
  TBG_URGENT();
  __shared__ uint32_t part[kScanBlock];
  constexpr uint32_t per = MSM_BUCKETS / kScanBlock;
  const uint32_t t = threadIdx.x, j0 = t * per;
  uint32_t sum = 0;
  for (uint32_t j = 0; j < per; ++j) sum += B.msm_off[j0 + j];
  part[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < kScanBlock; d <<= 1) {  // inclusive Hillis-Steele scan
    const uint32_t v = t >= d ? part[t - d] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = part[t] - sum;
  for (uint32_t j = 0; j < per; ++j) {
    const uint32_t c = B.msm_off[j0 + j];
    B.msm_off[j0 + j] = run;
    B.msm_cur[j0 + j] = run;
    run += c;
  }
  if (t == kScanBlock - 1) B.msm_off[MSM_BUCKETS] = run;
}

__global__ void TBG_LAUNCH k_msm_scatter(DevBatch B) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B.n_partials || B.partial_status[i] != TBG_PS_NOT_VERIFIED) return;
  uint32_t u[4];
  rlc_digits(B.msm_r[i], u);
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    bool neg;
    const uint32_t j = msm_bucket(u[k], neg);
    B.msm_ent[atomicAdd(&B.msm_cur[j], 1u)] = msm_entry(i, k, neg);
  }
}

// psi^k(s) (bls_msm.h) with the Fp2 coordinates split over the lane pair.
__device__ __forceinline__ Aff<Fp2x> px_psi_k(const G2A& s, uint32_t k, bool neg) {
  Aff<Fp2x> p = px_load(s);
  p.y = f_reduce(p.y);  // decoded coordinates may be up to 16p (a negated root)
  if (k & 1) p = Aff<Fp2x>{f_mulc(f_conj(p.x), PSI_X), f_mulc(f_conj(p.y), PSI_Y)};
  const bool ny = ((k & 2) != 0) != neg;
  if (k & 2) p.x = f_mulfp(p.x, fp_from_const(PSI2_X));
  if (ny) p.y = f_reduce(f_neg(p.y));
  return p;
}

// Bucket sums in two kernels so that no lane pair runs a long chain: a pair
// per (bucket j, slice of its entries) adds its slice (~20 mixed additions),
// then a pair per bucket adds the MSM_SPLIT slice sums and multiplies by
// (2j + 1) (one pair per bucket running all ~80 additions and the scaling
// took 5.0 ms per 160k-DV launch, latency-bound on 1,024 waves).
__global__ void TBG_LAUNCH_N(TBG_PAIR_WAVES) k_msm_bucket_part(DevBatch B) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;  // both lanes of a pair take the same branches
  if (w >= MSM_BUCKETS * MSM_SPLIT) return;
  if (B.counters[CNT_L0_BAD]) return;
  const uint32_t j = w / MSM_SPLIT, sl = w % MSM_SPLIT;
  const uint32_t o0 = B.msm_off[j], n = B.msm_off[j + 1] - o0;
  const uint32_t e0 = o0 + (n * sl) / MSM_SPLIT, e1 = o0 + (n * (sl + 1)) / MSM_SPLIT;
  Jac<Fp2x> acc = jac_inf<Fp2x>();
#pragma unroll 1
  for (uint32_t e = e0; e < e1; ++e) {
    const uint32_t v = B.msm_ent[e];
    acc = jac_add_aff_in(acc, px_psi_k(B.sig_aff[v >> 3], (v >> 1) & 3u, (v & 1u) != 0));
  }
  px_store(B.msm_part[w], acc);
}

// [2j + 1] (sum of bucket j's slices): FAST = the additions without the
// doubling branch (`exc` set when one needed it), else the complete formulas
// (out-of-line calls)
template <bool FAST>
__device__ __forceinline__ Jac<Fp2x> msm_bucket_scaled(const DevBatch& B, uint32_t j, bool& exc) {
  Jac<Fp2x> acc = px_load(B.msm_part[MSM_SPLIT * j]);
#pragma unroll 1
  for (uint32_t sl = 1; sl < MSM_SPLIT; ++sl) {
    const Jac<Fp2x> q = px_load(B.msm_part[MSM_SPLIT * j + sl]);
    acc = FAST ? jac_add_x(acc, q, exc) : jac_add(acc, q);
  }
  const uint32_t m = 2 * j + 1;
  if (m > 1 && !jac_is_inf(acc)) {
    // the base waits in the output slot, read where it is added (held in
    // registers across the ladder it spilled ~40 words per step)
    px_store(B.msm_bkt[j], acc);
    const int top = 31 - __builtin_clz(m);
#pragma unroll 1
    for (int bit = top - 1; bit >= 0; --bit) {
      acc = jac_dbl_in(acc);
      if ((m >> bit) & 1u) {
        __asm__ __volatile__("" ::: "memory");
        const Jac<Fp2x> b = px_load(B.msm_bkt[j]);
        acc = FAST ? jac_add_x(acc, b, exc) : jac_add(acc, b);
      }
    }
  }
  return acc;
}
// the doubling case of an addition (equal slice sums: crafted signatures
// only) redone with the complete formulas, out of line
__device__ __noinline__ Jac<Fp2x> msm_bucket_complete(const DevBatch& B, uint32_t j) {
  bool unused = false;
  return msm_bucket_scaled<false>(B, j, unused);
}

// (the additions without the doubling branch: the complete formulas inline
// spilled 139 VGPRs on this latency-bound tail kernel)
__global__ void TBG_LAUNCH_N(TBG_PAIR_WAVES) k_msm_bucket(DevBatch B) {
  TBG_URGENT();
  const uint32_t j = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  if (j >= MSM_BUCKETS) return;
  if (B.counters[CNT_L0_BAD]) return;
  bool exc = false;
  Jac<Fp2x> acc = msm_bucket_scaled<true>(B, j, exc);
  if (!pair_all(!exc)) acc = msm_bucket_complete(B, j);  // (pair-uniform)
  px_store(B.msm_bkt[j], acc);
}

// Tree sum of the scaled buckets in TWO kernels (four passes of 16-point
// chains took 60 dependent additions, ~1.8 ms of a launch's critical path):
// a lane pair adds MSM_TREE_PER points, then the workgroup halves its pairs
// through LDS (log2 levels); the first kernel leaves one point per
// workgroup, the second sums those the same way and writes S in affine form
// (or flags level 0 when S is the point at infinity): 3 + 7 + 1 + 5 = 16
// dependent additions.
constexpr uint32_t MSM_TREE_PAIRS = 128;  // lane pairs per workgroup of the first kernel
constexpr uint32_t MSM_TREE_PER = 4;      // points per pair in the first kernel
constexpr uint32_t MSM_TREE_WG = MSM_BUCKETS / (MSM_TREE_PAIRS * MSM_TREE_PER);  // 64 partial sums
static_assert(MSM_TREE_WG <= 2 * 64 && MSM_TREE_WG <= MSM_SUM_ENTRIES, "second tree kernel: one workgroup");

// acc summed over the workgroup's PAIRS lane pairs (every thread calls it;
// pair 0 ends with the total)
template <uint32_t PAIRS>
__device__ __forceinline__ Jac<Fp2x> pair_tree_sum(Jac<Fp2x> acc, Jac<Fp2x>* lds) {
  const uint32_t t = threadIdx.x, pr = t >> 1;
#pragma unroll 1
  for (uint32_t s = 1; s < PAIRS; s <<= 1) {
    lds[t] = acc;
    __syncthreads();
    if ((pr & (2 * s - 1)) == 0 && pr + s < PAIRS) acc = jac_add_in<Fp2x, true>(acc, lds[t + 2 * s]);
    __syncthreads();
  }
  return acc;
}

__global__ void __launch_bounds__(2 * MSM_TREE_PAIRS) k_msm_tree(DevBatch B) {
  TBG_URGENT();
  __shared__ Jac<Fp2x> lds[2 * MSM_TREE_PAIRS];
  if (B.counters[CNT_L0_BAD]) return;  // (grid-uniform)
  const uint32_t pr = threadIdx.x >> 1;
  const uint32_t a0 = (blockIdx.x * MSM_TREE_PAIRS + pr) * MSM_TREE_PER;
  Jac<Fp2x> acc = px_load(B.msm_bkt[a0]);
#pragma unroll 1
  for (uint32_t a = a0 + 1; a < a0 + MSM_TREE_PER; ++a) acc = jac_add_in<Fp2x, true>(acc, px_load(B.msm_bkt[a]));
  acc = pair_tree_sum<MSM_TREE_PAIRS>(acc, lds);
  if (pr == 0) px_store(B.msm_sum[blockIdx.x], acc);
}

__global__ void __launch_bounds__(MSM_TREE_WG) k_msm_tree_final(DevBatch B) {
  TBG_URGENT();
  constexpr uint32_t PAIRS = MSM_TREE_WG / 2;
  __shared__ Jac<Fp2x> lds[2 * PAIRS];
  if (B.counters[CNT_L0_BAD]) return;
  const uint32_t pr = threadIdx.x >> 1;
  Jac<Fp2x> acc = jac_add_in<Fp2x, true>(px_load(B.msm_sum[2 * pr]), px_load(B.msm_sum[2 * pr + 1]));
  acc = pair_tree_sum<PAIRS>(acc, lds);
  if (pr != 0) return;
  if (jac_is_inf(acc)) {
    if (pair_par() == 0) B.counters[CNT_L0_BAD] = 1;  // S = 0: no lines; the group levels decide
    return;
  }
  const Fp2x zi = f_inv(acc.Z);
  const Fp2x zi2 = f_sqr(zi);
  px_store(*B.batch_pt, Aff<Fp2x>{f_mul(acc.X, zi2), f_mul(acc.Y, f_mul(zi2, zi))});
}

// ------------------------------------------ fused level 0, smaller launches
// Below l0_tail_partials (l0_tail, tbls_launch.h) S keeps its three kernels
// behind the key side and the aggregation, as before the S role existed.
// S from the batched subgroup test's sums (bls_rlc.h, top): the 18 columns
// Qbar_k = sum over the groups of Q_k (k_sgb_combine left Q_k in the first
// slot of combination k's buckets, k_sgb_test proved it in G2) and the
// column T (k_sgb_bucket's slice sums), then
//   S = sum_j psi^j(2 A_j + T),  A_j = sum_e 13^e Qbar_(first_j + e).
//   k_l0f_reduce  one workgroup per L0FK_CHUNK points of a column: their sum
//   k_l0f_fold    one workgroup per column: the sum of its chunk sums
//   k_l0f_horner  one lane pair per j: A_j by Horner steps, psi^j(2 A_j + T); S affine
// A failed subgroup group voids level 0 (its Q_k are not in G2 and its
// members are about to be tested alone: k_sgb.hip sets the flag with
// sgb_bad), as does a key mark made after the sort (k_rlc_g1_l0) and S = 0.  Every addition takes the complete formulas:
// small multiples of one point (equal signatures) do meet the doubling case.
__global__ void __launch_bounds__(2 * L0FK_PAIRS) k_l0f_reduce(DevBatch B, uint32_t n_sg, uint32_t wq, uint32_t n_t) {
  __shared__ Jac<Fp2x> lds[2 * L0FK_PAIRS];
  if (B.counters[CNT_L0_BAD]) return;  // (grid-uniform: set before this kernel starts)
  const uint32_t pr = threadIdx.x >> 1, b = blockIdx.x;
  const bool qcol = b < SGB_K * wq;
  const uint32_t col = qcol ? b / wq : SGB_K, chunk = qcol ? b % wq : b - SGB_K * wq;
  const uint32_t count = qcol ? n_sg : n_sg * n_t;
  const uint32_t a0 = chunk * L0FK_CHUNK + pr * L0FK_PER, a1 = min(a0 + L0FK_PER, count);
  Jac<Fp2x> acc = jac_inf<Fp2x>();
#pragma unroll 1
  for (uint32_t a = a0; a < a1; ++a) {  // (pair-uniform)
    if (qcol) {
      acc = jac_add_in<Fp2x, true>(acc, px_load(B.sgb_part[sgb_q_slot(B, a, col)]));
    } else {
      acc = jac_add_in<Fp2x, true>(acc, px_load(B.sgb_t[a]));
    }
  }
  acc = pair_tree_sum<L0FK_PAIRS>(acc, lds);
  if (pr == 0) px_store(B.l0f_sum[b], acc);
}

__global__ void __launch_bounds__(2 * L0FK_PAIRS) k_l0f_fold(DevBatch B, uint32_t wq, uint32_t wt) {
  TBG_URGENT();
  __shared__ Jac<Fp2x> lds[2 * L0FK_PAIRS];
  if (B.counters[CNT_L0_BAD]) return;  // (grid-uniform)
  const uint32_t pr = threadIdx.x >> 1, col = blockIdx.x;
  const uint32_t first = col < SGB_K ? col * wq : SGB_K * wq, count = col < SGB_K ? wq : wt;
  Jac<Fp2x> acc = jac_inf<Fp2x>();
#pragma unroll 1
  for (uint32_t a = pr; a < count; a += L0FK_PAIRS) acc = jac_add_in<Fp2x, true>(acc, px_load(B.l0f_sum[first + a]));
  acc = pair_tree_sum<L0FK_PAIRS>(acc, lds);
  if (pr == 0) px_store(B.l0f_sum[SGB_K * wq + wt + col], acc);
}

constexpr uint32_t L0F_HORNER_THREADS = 8;  // four lane pairs, one per j
__global__ void __launch_bounds__(64) k_l0f_horner(DevBatch B, uint32_t base) {
  TBG_URGENT();
  __shared__ Jac<Fp2x> lds[L0F_HORNER_THREADS];
  if (B.counters[CNT_L0_BAD]) return;
  const int j = (int)(threadIdx.x >> 1);
  const G2J* tot = B.l0f_sum + base;  // the column totals
  const int e0 = l0f_first(j), e1 = l0f_first(j + 1);
  Jac<Fp2x> acc = px_load(tot[e1 - 1]);
#pragma unroll 1
  for (int e = e1 - 2; e >= e0; --e) acc = l0f_mul13_add(acc, px_load(tot[e]));  // (pair-uniform trip counts)
  acc = l0f_term(acc, px_load(tot[SGB_K]), j);
  acc = pair_tree_sum<L0F_HORNER_THREADS / 2>(acc, lds);
  if (j != 0) return;
  if (jac_is_inf(acc)) {
    if (pair_par() == 0) B.counters[CNT_L0_BAD] = 1;  // S = 0: no lines; the group levels decide
    return;
  }
  const Fp2x zi = f_inv(acc.Z);
  const Fp2x zi2 = f_sqr(zi);
  px_store(*B.batch_pt, Aff<Fp2x>{f_mul(acc.X, zi2), f_mul(acc.Y, f_mul(zi2, zi))});
}

void launch_pubkey_tables(const G1A* pk, const G1A* xpk, const int32_t* status, uint32_t n, G1A* tab, hipStream_t st) {
  if (n) TBG_KLAUNCH(k_pubkey_tables, dim3((n + BINV_BLOCK - 1) / BINV_BLOCK), dim3(BINV_BLOCK), st, pk, xpk, status, n,
                     tab);
}

// Level 0's key side: G1 products, bucket sizes, and the ERR_PUBKEY marks
// (after it the candidates are final: the speculative aggregation may run).
// With l0_tail(B) a fused launch's grid starts with the S role's workgroups:
// S is formed beside the key side, before the aggregation and long before
// k_l0_lines reads it.
void launch_l0_keys(const DevBatch& B, const G1A* pk_tab, const int32_t* pk_status, uint32_t n_pk, hipStream_t st) {
  // (msm_off and the S role's counters were zeroed by k_decode_sigs, the chain's first kernel)
  const uint32_t n_s = l0_tail(B) ? l0f_s_blocks(B) : 0u;
  if (l0_per_duty(B)) {  // P_d and dv_state too; the same name in the per-kernel profile
    using l0duty::k_rlc_g1_l0;
    TBG_KLAUNCH(k_rlc_g1_l0, dim3(n_s + grid_for(B.n_duties).x), dim3(kBlock), st, B, pk_tab, pk_status, n_pk, n_s);
    return;
  }
  if (B.n_partials)
    TBG_KLAUNCH(k_rlc_g1_l0, dim3(n_s + grid_for(B.n_partials).x), dim3(kBlock), st, B, pk_tab, pk_status, n_pk, n_s);
}

// Level 0's signature side: the bucket MSM up to S (affine).
void launch_l0_msm(const DevBatch& B, hipStream_t st) {
  TBG_KLAUNCH(k_msm_scan, dim3(1), dim3(kScanBlock), st, B);
  if (B.n_partials) TBG_KLAUNCH(k_msm_scatter, grid_for(B.n_partials), dim3(kBlock), st, B);
  TBG_KLAUNCH(k_msm_bucket_part, grid_for(2 * MSM_BUCKETS * MSM_SPLIT), dim3(kBlock), st, B);
  TBG_KLAUNCH(k_msm_bucket, grid_for(2 * MSM_BUCKETS), dim3(kBlock), st, B);
  TBG_KLAUNCH(k_msm_tree, dim3(MSM_TREE_WG), dim3(2 * MSM_TREE_PAIRS), st, B);
  TBG_KLAUNCH(k_msm_tree_final, dim3(1), dim3(MSM_TREE_WG), st, B);
}

// Fused level 0's signature side in launches below l0_tail_partials: S from the subgroup test's sums.
void launch_l0_fused_s(const DevBatch& B, hipStream_t st) {
  const uint32_t n_sg = sgb_groups(B.n_partials, B.sgb_m), n_t = sgb_t_slices(B.sgb_m);
  const uint32_t wq = l0fk_q_chunks(n_sg), wt = l0fk_t_chunks(n_sg, B.sgb_m);
  TBG_KLAUNCH(k_l0f_reduce, dim3(SGB_K * wq + wt), dim3(2 * L0FK_PAIRS), st, B, n_sg, wq, n_t);
  TBG_KLAUNCH(k_l0f_fold, dim3(L0F_COLS), dim3(2 * L0FK_PAIRS), st, B, wq, wt);
  TBG_KLAUNCH(k_l0f_horner, dim3(1), dim3(L0F_HORNER_THREADS), st, B, SGB_K * wq + wt);
}

}  // namespace tbg
