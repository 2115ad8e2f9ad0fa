// Batched subgroup test of the decoded signatures: the
// per-signature check psi(s) == [x] s (k_subgroup_sigs: 63 doublings + 5
// additions per signature) runs only for the members of groups whose
// random combinations fail.  Reference: tblsconv.SigFromCore's subgroup
// check (tblsconv/tblsconv.go:125-132) -- every partial still gets the exact
// per-item verdict.
//
// E2(Fp2) = G2 x H with |H| the G2 cofactor h2, whose smallest prime factor
// is 13.  Write s_i = g_i + t_i (t_i in H).  For a group of SGB_M consecutive
// partials and SGB_K combinations
//   Q_k = sum_i c_ik s_i,   c_ik uniform in {-6, ..., 6} (distinct mod 13),
// Q_k is in G2 iff sum_i c_ik t_i = 0.  If some t_j != 0, fix every other
// coefficient: c t_j takes 13 distinct values (ord t_j has no prime factor
// below 13), so at most one value of c_jk cancels -- probability <= 1/13 per
// combination, 13^-18 < 2^-66 for all 18.  The coefficients come from the
// batch's secret seed (sgb_digits, bls_rlc.h), so a submitter cannot aim at
// them.  Each Q_k is a bucket sum: bucket (k, v) adds +-s_i over the members
// with |c_ik| = v, and Q_k = sum_v v B_(k,v) by running sums -- ~16.6 mixed
// additions per signature instead of ~68 group operations, plus 18 tests per
// group of 1,024.
//
//   k_sgb_sort    one workgroup per group: digits, bucket counts and entries in LDS
//   k_sgb_bucket  one lane PAIR per (group, bucket, slice): the slice's sum
//   k_sgb_fold    one lane PAIR per (group, bucket): the sum of its slices
//   k_sgb_combine one lane PAIR per (group, combination): Q_k from its buckets
//   k_sgb_test    one lane PAIR per (group, combination): psi(Q_k) == [x] Q_k
// then k_subgroup_sigs tests the members of failed groups one by one.
//
// Paired schedule (groups of SGB_PAIR_M = 256 members and more; tbls_launch.h,
// bls_sgb.h).  The one-dimensional buckets (k, |c_ik|) are Pippenger with the
// smallest window.  The 18 sums are separate outputs, but a member may be
// sorted by two of its digits at once: for the pairs (2p, 2p + 1), p = 0..8,
// member i goes into bucket (a, b) = +-(c_i,2p, c_i,2p+1) with the sign (and
// the point) chosen so that a > 0, or a = 0 and b > 0 -- 84 buckets per pair,
// 756 per group, one mixed addition per member per PAIR: 9 x 168/169 = 8.9
// instead of 16.6.  Both sums come out of the 84 bucket sums B(a, b):
//   R_a = sum_b B(a, b),                                Q_2p   = sum_a a R_a
//   D_v = sum_(a>=0) B(a, v) - sum_(a>=1) B(a, -v),     Q_2p+1 = sum_v v D_v
// (k_sgb_fold: 12 sums of 13 terms per pair, written where the classic
// schedule leaves its folded buckets, so k_sgb_combine and k_sgb_test run
// unchanged).  Every Q_k is the same group element as in the classic
// schedule, so the soundness argument above and the fused level 0 carry over
// word for word.  A bucket holds ~6 members of 1,024 with a wide spread
// (0..15), and a wave runs as long as its longest bucket: k_sgb_sort also
// ranks the group's buckets by entry count (a counting sort in LDS) and
// k_sgb_bucket hands the 32 lane pairs of a wave consecutive ranks -- 9.4
// wave iterations per member instead of 14.9 in index order (19.3 classic;
// DESIGN section 4 has the table and the threshold).
//
// Triple schedule (groups larger than SGB_M: SGB_TRI_M = 16,384 members in
// clean launches of at least tbg_config.sgb_tri_partials partials;
// tbls_launch.h, bls_sgb.h).  The same step once more: for the triples
// (3t, 3t + 1, 3t + 2), t = 0..5, member i goes into bucket
// (a, b, c) = +-(c_i,3t, c_i,3t+1, c_i,3t+2), the first non-zero digit made
// positive -- 1,098 buckets per triple, 6,588 per group, 6 x 2196/2197 = 6.0
// mixed additions per member.  Such groups do not fit LDS, so the sort runs in
// global memory:
//   k_sgb_tri_count    one lane per member: digits, l0f_u, six bucket codes; the
//                      group's counters by atomicAdd, whose result is the member's
//                      place in its bucket
//   k_sgb_tri_scan     one workgroup per group: counts -> offsets, buckets ranked
//   k_sgb_tri_scatter  one lane per member: its entries to offset + place
// k_sgb_bucket takes the ranked buckets as on the paired schedule, and
//   k_sgb_tri_fold     pass 1: per triple P(a, b) = sum_c B(a, b, c) -- the paired
//                      schedule's 84 buckets of (3t, 3t + 1) -- and the partial sums
//                      E(v, a, +-) = sum_b B(a, b, +-v) of the third combination;
//                      pass 2: the pair's R_a, D_v over P, and
//                      D_v = sum_a (E(v, a, +) - E(v, a, -)) for the third
// leaves the same 108 folded sums per group (chains of at most 14 terms;
// ~2,350 additions per triple whatever the group's size, which is why only
// large groups take it: DESIGN section 4).  The order inside a bucket follows
// the atomics; the sums are group elements, so verdicts and bytes do not
// depend on it.
//
// With the fused level 0 (bls_rlc.h, top) the same sums serve level 0's
// S = sum r_i s_i: k_sgb_sort also stores the digits of r_i, k_sgb_bucket also
// adds the group's unweighted sum T, and a failed group voids level 0.
#define TBG_ADD_DBL_INLINE 1
#ifndef TBG_SCHED_FENCE
#define TBG_SCHED_FENCE 1  // products in program order: fits the pair kernels in 256 VGPRs (bls_field.h)
#endif
#include "tbls_launch.h"
#include "bls_rlc.h"
#include "bls_sgb.h"

namespace tbg {

#ifndef TBG_SGB_SORT_BLOCK
#define TBG_SGB_SORT_BLOCK 256
#endif
constexpr uint32_t kSgbSortBlock = TBG_SGB_SORT_BLOCK;  // threads per group's sort

static_assert(SGBP_B == SGB_PB && SGBP_V == SGB_V && SGBP_SUMS * SGB_PAIRS == SGB_BUCKETS, "bls_sgb.h's pair layout");
static_assert(SGBT_B == SGB_TB && SGBT_SUMS1 == SGB_TF1 && SGBT_SUMS2 * SGB_TRIPLES == SGB_BUCKETS, "bls_sgb.h's triple layout");
static_assert((kSgbSortBlock & (kSgbSortBlock - 1)) == 0, "sgb_block_scan: a power of two");
constexpr uint32_t SGB_RANK_KEYS = 256;  // bucket sizes 0..254 apart, larger ones together

// a[0..N) -> its exclusive prefix sums, a[N] = the total; every thread of the
// workgroup calls it (each scans ceil(N / block) consecutive values, the
// block's partial sums by doubling steps in tmp[block])
template <uint32_t N>
__device__ __forceinline__ void sgb_block_scan(uint32_t* a, uint32_t* tmp) {
  constexpr uint32_t PER = (N + kSgbSortBlock - 1) / kSgbSortBlock;
  const uint32_t t = threadIdx.x, b0 = t * PER;
  uint32_t sum = 0;
  for (uint32_t j = 0; j < PER; ++j)
    if (b0 + j < N) sum += a[b0 + j];
  tmp[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < kSgbSortBlock; d <<= 1) {
    const uint32_t x = t >= d ? tmp[t - d] : 0u;
    __syncthreads();
    tmp[t] += x;
    __syncthreads();
  }
  uint32_t run = tmp[t] - sum;
  for (uint32_t j = 0; j < PER; ++j)
    if (b0 + j < N) {
      const uint32_t x = a[b0 + j];
      a[b0 + j] = run;
      run += x;
    }
  if (t == kSgbSortBlock - 1) a[N] = tmp[t];
  __syncthreads();
}

// k_sgb_sort for a group on the paired schedule: SGB_PAIRS entries per
// member, SGB_PBUCKETS buckets, and the buckets ranked by decreasing entry
// count for k_sgb_bucket; `lds` is the workgroup's digit array, reused for
// one byte per (member, pair) and the sort's own arrays
__device__ __forceinline__ void sgb_sort_paired(const DevBatch& B, uint8_t* lds) {
  // (carved from the classic schedule's digit array: the kernel's LDS, and with it its occupancy, stay)
  uint8_t* code = lds;                                        // [SGB_M][SGB_PAIRS]
  uint32_t* cnt = (uint32_t*)(lds + SGB_M * SGB_PAIRS);       // [SGB_PBUCKETS + 1]
  uint32_t* hist = cnt + SGB_PBUCKETS + 1;                    // [SGB_RANK_KEYS + 1]
  uint32_t* tmp = hist + SGB_RANK_KEYS + 1;                   // [kSgbSortBlock]
  uint8_t* key = (uint8_t*)(tmp + kSgbSortBlock);             // [SGB_PBUCKETS]
  static_assert((SGB_M * SGB_PAIRS) % 4 == 0 &&
                    SGB_M * SGB_PAIRS + 4 * (SGB_PBUCKETS + 1 + SGB_RANK_KEYS + 1 + kSgbSortBlock) + SGB_PBUCKETS <=
                        SGB_M * SGB_K,
                "the paired sort's arrays fit the digit array");
  const uint32_t g = blockIdx.x, t = threadIdx.x, m = B.sgb_m;
  const uint32_t i0 = g * m;
  const uint32_t n = min(m, B.n_partials - i0);
  for (uint32_t b = t; b < SGB_PBUCKETS; b += kSgbSortBlock) cnt[b] = 0;
  for (uint32_t b = t; b < SGB_RANK_KEYS; b += kSgbSortBlock) hist[b] = 0;
  if (t == 0) B.sgb_bad[g] = 0;
  const bool fused = l0_fused(B);
  __syncthreads();
  for (uint32_t li = t; li < n; li += kSgbSortBlock) {
    const bool ok = B.partial_status[i0 + li] == TBG_PS_NOT_VERIFIED;
    int32_t c[SGB_K];
    sgb_digits(B.sgb_seed, i0 + li, c);
    if (fused) {  // (as in k_sgb_sort below)
      uint32_t u[4];
      l0f_digits(c, u);
      *(uint4*)(B.l0f_u + 4ull * (i0 + li)) = make_uint4(u[0], u[1], u[2], u[3]);
    }
#pragma unroll
    for (uint32_t p = 0; p < SGB_PAIRS; ++p) {
      const uint32_t cd = ok ? sgb_pair_code(c[2 * p], c[2 * p + 1]) : SGBP_NONE;
      code[li * SGB_PAIRS + p] = (uint8_t)cd;
      if (cd != SGBP_NONE) atomicAdd(&cnt[p * SGB_PB + (cd & 0x7Fu)], 1u);
    }
  }
  __syncthreads();
  for (uint32_t b = t; b < SGB_PBUCKETS; b += kSgbSortBlock) {  // larger buckets first
    const uint32_t k = SGB_RANK_KEYS - 1 - min(cnt[b], SGB_RANK_KEYS - 1);
    key[b] = (uint8_t)k;
    atomicAdd(&hist[k], 1u);
  }
  __syncthreads();
  sgb_block_scan<SGB_PBUCKETS>(cnt, tmp);
  sgb_block_scan<SGB_RANK_KEYS>(hist, tmp);
  uint32_t* goff = B.sgb_off + (size_t)(SGB_PBUCKETS + 1) * g;
  uint32_t* rank = B.sgb_rank + (size_t)SGB_PBUCKETS * g;
  for (uint32_t b = t; b <= SGB_PBUCKETS; b += kSgbSortBlock) {
    goff[b] = cnt[b];
    if (b < SGB_PBUCKETS) rank[atomicAdd(&hist[key[b]], 1u)] = b;  // (every rank 0..755 once)
  }
  __syncthreads();  // cnt: now the scatter cursors
  uint32_t* ent = B.sgb_ent + (size_t)sgb_ent_stride(m) * g;
  for (uint32_t li = t; li < n; li += kSgbSortBlock) {
#pragma unroll 1
    for (uint32_t p = 0; p < SGB_PAIRS; ++p) {
      const uint32_t cd = code[li * SGB_PAIRS + p];
      if (cd == SGBP_NONE) continue;
      const uint32_t pos = atomicAdd(&cnt[p * SGB_PB + (cd & 0x7Fu)], 1u);
      ent[pos] = (li << 1) | (cd >> 7);
    }
  }
}

__global__ void __launch_bounds__(kSgbSortBlock) k_sgb_sort(DevBatch B) {
  __shared__ uint32_t cnt[SGB_BUCKETS];
  __shared__ uint32_t off[SGB_BUCKETS + 1];
  __shared__ __attribute__((aligned(16))) int8_t dig[SGB_M * SGB_K];  // (the largest group)
  if (sgb_paired(B.sgb_m)) {  // (grid-uniform)
    sgb_sort_paired(B, (uint8_t*)dig);
    return;
  }
  const uint32_t g = blockIdx.x, t = threadIdx.x, m = B.sgb_m;
  const uint32_t i0 = g * m;
  const uint32_t n = min(m, B.n_partials - i0);
  for (uint32_t b = t; b < SGB_BUCKETS; b += kSgbSortBlock) cnt[b] = 0;
  if (t == 0) B.sgb_bad[g] = 0;
  const bool fused = l0_fused(B);
  __syncthreads();
  for (uint32_t li = t; li < n; li += kSgbSortBlock) {
    const bool ok = B.partial_status[i0 + li] == TBG_PS_NOT_VERIFIED;
    int32_t c[SGB_K];
    sgb_digits(B.sgb_seed, i0 + li, c);
    if (fused) {  // level 0's scalar of the partial is a form of these digits (bls_rlc.h; k_rlc_g1_l0 reads it)
      uint32_t u[4];
      l0f_digits(c, u);
      *(uint4*)(B.l0f_u + 4ull * (i0 + li)) = make_uint4(u[0], u[1], u[2], u[3]);
    }
#pragma unroll
    for (uint32_t k = 0; k < SGB_K; ++k) {
      const int32_t d = ok ? c[k] : 0;
      dig[li * SGB_K + k] = (int8_t)d;
      if (d) atomicAdd(&cnt[k * SGB_V + (uint32_t)(d < 0 ? -d : d) - 1], 1u);
    }
  }
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0;
    for (uint32_t b = 0; b < SGB_BUCKETS; ++b) {
      off[b] = run;
      run += cnt[b];
    }
    off[SGB_BUCKETS] = run;
  }
  __syncthreads();
  uint32_t* goff = B.sgb_off + (size_t)(SGB_BUCKETS + 1) * g;
  for (uint32_t b = t; b <= SGB_BUCKETS; b += kSgbSortBlock) {
    goff[b] = off[b];
    if (b < SGB_BUCKETS) cnt[b] = off[b];  // scatter cursors
  }
  __syncthreads();
  uint32_t* ent = B.sgb_ent + (size_t)m * SGB_K * g;
  for (uint32_t li = t; li < n; li += kSgbSortBlock) {
#pragma unroll 1
    for (uint32_t k = 0; k < SGB_K; ++k) {
      const int32_t d = dig[li * SGB_K + k];
      if (!d) continue;
      const uint32_t pos = atomicAdd(&cnt[k * SGB_V + (uint32_t)(d < 0 ? -d : d) - 1], 1u);
      ent[pos] = (li << 1) | (d < 0 ? 1u : 0u);
    }
  }
}

// ---- triple schedule: the sort in global memory (groups past SGB_M do not fit LDS) ----
// k_sgb_tri_count, one lane per member: the digits once, l0f_u as k_sgb_sort
// writes it, and per triple the member's bucket code.  The group's counters
// are its sgb_off row (zeroed by the launcher); the count the atomicAdd
// returns is the member's place in its bucket, kept in the code, so the
// scatter needs no second round of atomics and no cursors.  (A workgroup's 256
// members make 1,536 entries over 6,588 buckets: counting in LDS first would
// merge next to nothing.)  The order inside a bucket follows the atomics and
// differs from run to run; the sums are group elements, so verdicts and
// bytes do not.
__global__ void __launch_bounds__(kSgbSortBlock) k_sgb_tri_count(DevBatch B) {
  const uint32_t i = blockIdx.x * kSgbSortBlock + threadIdx.x;
  if (i >= B.n_partials) return;
  const uint32_t g = i / B.sgb_m;
  const bool ok = B.partial_status[i] == TBG_PS_NOT_VERIFIED;
  int32_t c[SGB_K];
  sgb_digits(B.sgb_seed, i, c);
  if (l0_fused(B)) {  // (as in k_sgb_sort)
    uint32_t u[4];
    l0f_digits(c, u);
    *(uint4*)(B.l0f_u + 4ull * i) = make_uint4(u[0], u[1], u[2], u[3]);
  }
  uint32_t* cnt = B.sgb_off + (size_t)(SGB_TBUCKETS + 1) * g;
#pragma unroll
  for (uint32_t t = 0; t < SGB_TRIPLES; ++t) {
    uint32_t cd = ok ? sgb_tri_code(c[3 * t], c[3 * t + 1], c[3 * t + 2]) : SGBT_NONE;
    if (cd != SGBT_NONE) cd |= atomicAdd(&cnt[t * SGB_TB + (cd & (SGBT_NEG - 1))], 1u) << 12;
    B.sgb_code[(size_t)SGB_TRIPLES * i + t] = cd;
  }
}

// k_sgb_tri_scan, one workgroup per group: its 6,588 counts -> offsets (in
// place), and its buckets ranked by decreasing count for k_sgb_bucket (the
// counting sort of the paired schedule, more keys)
__global__ void __launch_bounds__(kSgbSortBlock) k_sgb_tri_scan(DevBatch B) {
  __shared__ uint32_t cnt[SGB_TBUCKETS + 1];
  __shared__ uint32_t hist[SGB_RANK_KEYS + 1];
  __shared__ uint32_t tmp[kSgbSortBlock];
  __shared__ uint8_t key[SGB_TBUCKETS];
  const uint32_t g = blockIdx.x, t = threadIdx.x;
  uint32_t* goff = B.sgb_off + (size_t)(SGB_TBUCKETS + 1) * g;
  uint32_t* rank = B.sgb_rank + (size_t)SGB_TBUCKETS * g;
  for (uint32_t b = t; b < SGB_RANK_KEYS; b += kSgbSortBlock) hist[b] = 0;
  if (t == 0) B.sgb_bad[g] = 0;
  __syncthreads();
  for (uint32_t b = t; b < SGB_TBUCKETS; b += kSgbSortBlock) {  // larger buckets first
    const uint32_t n = goff[b];
    cnt[b] = n;
    const uint32_t k = SGB_RANK_KEYS - 1 - min(n, SGB_RANK_KEYS - 1);
    key[b] = (uint8_t)k;
    atomicAdd(&hist[k], 1u);
  }
  __syncthreads();
  sgb_block_scan<SGB_TBUCKETS>(cnt, tmp);
  sgb_block_scan<SGB_RANK_KEYS>(hist, tmp);
  for (uint32_t b = t; b <= SGB_TBUCKETS; b += kSgbSortBlock) {
    goff[b] = cnt[b];
    if (b < SGB_TBUCKETS) rank[atomicAdd(&hist[key[b]], 1u)] = b;  // (every rank 0..6587 once)
  }
}

// k_sgb_tri_scatter, one lane per member: its (member, sign) entries, one per
// triple, to the places k_sgb_tri_count drew
__global__ void __launch_bounds__(kSgbSortBlock) k_sgb_tri_scatter(DevBatch B) {
  const uint32_t i = blockIdx.x * kSgbSortBlock + threadIdx.x;
  if (i >= B.n_partials) return;
  const uint32_t m = B.sgb_m, g = i / m, li = i - g * m;
  const uint32_t* goff = B.sgb_off + (size_t)(SGB_TBUCKETS + 1) * g;
  uint32_t* ent = B.sgb_ent + (size_t)sgb_ent_stride(m) * g;
#pragma unroll
  for (uint32_t t = 0; t < SGB_TRIPLES; ++t) {
    const uint32_t cd = B.sgb_code[(size_t)SGB_TRIPLES * i + t];
    if (cd == SGBT_NONE) continue;
    ent[goff[t * SGB_TB + (cd & (SGBT_NEG - 1))] + (cd >> 12)] = (li << 1) | ((cd / SGBT_NEG) & 1u);
  }
}

// one lane pair per (group, bucket, slice) -- on the paired schedule per
// (group, rank): the SGB_PRANK = 768 pairs of a group take its 756 buckets in
// the order of k_sgb_sort's ranking, so the 32 pairs of a wave hold buckets
// of near-equal length (the last 12 are idle), and on the triple schedule the
// SGB_TRANK = 6,592 pairs its 6,588 buckets in the same way; with the fused level 0 further
// pairs, one per (group, SGB_T_PER consecutive members), add the group's
// unweighted sum T: one more bucket with coefficient +1 whose members are the
// candidates at sort time (nothing changes a status between the two kernels)
__global__ void TBG_LAUNCH_N(TBG_PAIR_WAVES) k_sgb_bucket(DevBatch B, uint32_t n_sg, uint32_t n_t) {
  uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;  // both lanes of a pair take the same branches
  const uint32_t S = B.sgb_split, m = B.sgb_m;
  const bool triple = sgb_triple(m);
  const bool paired = sgb_paired(m) || triple;  // (ranked buckets; grid-uniform)
  const uint32_t n_rank = triple ? SGB_TBUCKETS : SGB_PBUCKETS;  // the ranked schedules' buckets per group
  const uint32_t per_g = triple ? SGB_TRANK : paired ? SGB_PRANK : SGB_BUCKETS * S;
  // T's pairs: after the buckets' on the classic schedule; FIRST on the paired
  // one, whose bucket chains (~12 additions a wave, the last waves of a group
  // next to none) are shorter than T's 32 -- started last, T's waves were the
  // grid's tail, a fifth of the kernel's time
  const bool is_t = paired ? w < n_sg * n_t : w >= n_sg * per_g;
  if (is_t) {
    const uint32_t wt = paired ? w : w - n_sg * per_g;
    if (wt >= n_sg * n_t) return;
    const uint32_t i0 = (wt / n_t) * m + (wt % n_t) * SGB_T_PER;
    const uint32_t i1 = min(min(i0 + SGB_T_PER, (wt / n_t + 1) * m), B.n_partials);
    Jac<Fp2x> acc = jac_inf<Fp2x>();
#pragma unroll 1
    for (uint32_t i = i0; i < i1; ++i) {  // (i0 >= n_partials in the last group's tail: an empty slice)
      if (B.partial_status[i] != TBG_PS_NOT_VERIFIED) continue;
      Aff<Fp2x> p = px_load(B.sig_aff[i]);
      p.y = f_reduce(p.y);
      acc = jac_add_aff_in(acc, p);
    }
    px_store(B.sgb_t[wt], acc);
    return;
  }
  if (paired) w -= n_sg * n_t;
  if (w >= n_sg * per_g) return;  // (the grid's last wave)
  const uint32_t g = w / per_g;
  uint32_t e0, e1;
  size_t out;
  if (paired) {
    const uint32_t r = w % per_g;
    if (r >= n_rank) return;
    const uint32_t b = B.sgb_rank[(size_t)n_rank * g + r];
    const uint32_t* goff = B.sgb_off + (size_t)(n_rank + 1) * g;
    e0 = goff[b];
    e1 = goff[b + 1];
    out = (size_t)sgb_part_stride(m) * g + b;
  } else {
    const uint32_t b = (w / S) % SGB_BUCKETS, sl = w % S;
    const uint32_t* goff = B.sgb_off + (size_t)(SGB_BUCKETS + 1) * g;
    const uint32_t o0 = goff[b], n = goff[b + 1] - o0;
    e0 = o0 + (n * sl) / S;
    e1 = o0 + (n * (sl + 1)) / S;
    out = w;
  }
  const uint32_t* ent = B.sgb_ent + (size_t)sgb_ent_stride(m) * g;
  const G2A* sig = B.sig_aff + (size_t)m * g;
  Jac<Fp2x> acc = jac_inf<Fp2x>();
#pragma unroll 1
  for (uint32_t e = e0; e < e1; ++e) {
    const uint32_t v = ent[e];
    Aff<Fp2x> p = px_load(sig[v >> 1]);
    p.y = f_reduce(p.y);  // decoded coordinates may be up to 16p (a negated root)
    if (v & 1u) p.y = f_reduce(f_neg(p.y));
    acc = jac_add_aff_in(acc, p);
  }
  px_store(B.sgb_part[out], acc);
}

// A failed group (k_sgb_test alone decides): its members are tested alone, and
// the fused level 0, whose S is built from the groups' sums (k_msm.hip), is
// void for the launch.
__device__ __forceinline__ void sgb_fail(const DevBatch& B, uint32_t g) {
  B.sgb_bad[g] = 1u;
  if (l0_fused(B)) B.counters[CNT_L0_BAD] = 1u;
}

// one lane pair per (group, bucket): the bucket's SGB_SPLIT slice sums into
// its first slice, so the running sums below are 2 x SGB_V additions deep
// instead of (SGB_SPLIT + 1) x SGB_V (a latency-bound kernel: few waves,
// each one serial chain).  The additions skip the doubling case (bls_pair.h
// jac_add_x: fewer live values than the complete formulas).  Two equal
// operands are no sign of a bad signature: a short last group's empty
// buckets make the running sums meet them almost surely, and replayed
// signatures make equal slice and bucket sums.  The pair that met them redoes
// its one sum with the complete formulas, out of line (bls_sgb.h); only
// k_sgb_test fails a group.
__device__ __noinline__ Jac<Fp2x> sgb_fold_complete(const G2J* part, uint32_t S) {
  bool unused = false;
  return sgb_fold_g<Fp2x, false>([&](uint32_t sl) { return px_load(part[sl]); }, S, unused);
}

// Paired schedule: one lane pair per (group, pair of combinations, one of its
// 12 sums R_a, D_v), each 13 bucket sums of which many are empty (bls_sgb.h
// sgb_pair_sum_g), stored after the group's bucket sums in the layout of the
// classic schedule's folded buckets.  Equal operands (replayed signatures)
// are redone in the same way.
__device__ __noinline__ Jac<Fp2x> sgb_pair_sum_complete(const G2J* bk, uint32_t j) {
  bool unused = false;
  return sgb_pair_sum_g<Fp2x, false>([&](uint32_t idx) { return px_load(bk[idx]); }, j, unused);
}

__global__ void TBG_LAUNCH_N(TBG_PAIR_WAVES) k_sgb_fold(DevBatch B, uint32_t n_sg) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;  // both lanes of a pair take the same branches
  if (w >= n_sg * SGB_BUCKETS) return;
  if (sgb_paired(B.sgb_m)) {
    const uint32_t g = w / SGB_BUCKETS, p = (w % SGB_BUCKETS) / SGBP_SUMS, j = w % SGBP_SUMS;
    G2J* grp = B.sgb_part + (size_t)sgb_part_stride(B.sgb_m) * g;
    const G2J* bk = grp + (size_t)SGB_PB * p;
    bool exc = false;
    Jac<Fp2x> acc = sgb_pair_sum_g<Fp2x, true>([&](uint32_t idx) { return px_load(bk[idx]); }, j, exc);
    if (!pair_all(!exc)) acc = sgb_pair_sum_complete(bk, j);  // (pair-uniform)
    px_store(grp[SGB_PBUCKETS + w % SGB_BUCKETS], acc);
    return;
  }
  const uint32_t S = B.sgb_split;
  G2J* part = B.sgb_part + (size_t)w * S;
  bool exc = false;
  Jac<Fp2x> acc = sgb_fold_g<Fp2x, true>([&](uint32_t sl) { return px_load(part[sl]); }, S, exc);
  if (!pair_all(!exc)) acc = sgb_fold_complete(part, S);  // (pair-uniform)
  px_store(part[0], acc);
}

// Triple schedule's fold in two passes (bls_sgb.h sgb_tri_sum1_g, _sum2_g).
// Pass 1, one lane pair per (group, triple, one of its 168 sums P, E): chains
// of at most 13 bucket sums, stored after the group's bucket sums.  Pass 2,
// one lane pair per (group, triple, one of its 18 sums R_a, D_v, D_v): chains
// of 13 or 14 first-pass sums, stored in the layout of the classic
// schedule's folded buckets.  Equal operands are redone as above.
__device__ __noinline__ Jac<Fp2x> sgb_tri_sum_complete(const G2J* src, uint32_t j, uint32_t pass) {
  bool unused = false;
  auto ld = [&](uint32_t idx) { return px_load(src[idx]); };
  return pass == 1 ? sgb_tri_sum1_g<Fp2x, false>(ld, j, unused) : sgb_tri_sum2_g<Fp2x, false>(ld, j, unused);
}

__global__ void TBG_LAUNCH_N(TBG_PAIR_WAVES) k_sgb_tri_fold(DevBatch B, uint32_t n_sg, uint32_t pass) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;  // both lanes of a pair take the same branches
  const uint32_t per_t = pass == 1 ? SGB_TF1 : SGBT_SUMS2, per_g = SGB_TRIPLES * per_t;
  if (w >= n_sg * per_g) return;
  const uint32_t g = w / per_g, t = (w % per_g) / per_t, j = w % per_t;
  G2J* grp = B.sgb_part + (size_t)sgb_part_stride(B.sgb_m) * g;
  const G2J* src = pass == 1 ? grp + (size_t)SGB_TB * t : grp + SGB_TBUCKETS + (size_t)SGB_TF1 * t;
  auto ld = [&](uint32_t idx) { return px_load(src[idx]); };
  bool exc = false;
  Jac<Fp2x> acc = pass == 1 ? sgb_tri_sum1_g<Fp2x, true>(ld, j, exc) : sgb_tri_sum2_g<Fp2x, true>(ld, j, exc);
  if (!pair_all(!exc)) acc = sgb_tri_sum_complete(src, j, pass);  // (pair-uniform)
  px_store(grp[(pass == 1 ? SGB_TBUCKETS : SGB_TFOLD) + w % per_g], acc);
}

// one lane pair per (group, combination): Q_k = sum_v v B_v by running sums
// from v = 6 down over the folded buckets, stored over the combination's
// first bucket (only this pair reads those buckets)
__device__ __noinline__ Jac<Fp2x> sgb_combine_complete(const G2J* part, uint32_t S) {
  bool unused = false;
  return sgb_running_sums_g<Fp2x, false>([&](uint32_t v) { return px_load(part[(size_t)v * S]); }, SGB_V, unused);
}

__global__ void TBG_LAUNCH_N(TBG_PAIR_WAVES) k_sgb_combine(DevBatch B, uint32_t n_sg) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;  // both lanes of a pair take the same branches
  if (w >= n_sg * SGB_K) return;
  const uint32_t g = w / SGB_K, k = w % SGB_K, S = sgb_paired(B.sgb_m) || sgb_triple(B.sgb_m) ? 1u : B.sgb_split;
  G2J* part = B.sgb_part + sgb_q_slot(B, g, k);
  bool exc = false;
  Jac<Fp2x> q = sgb_running_sums_g<Fp2x, true>([&](uint32_t v) { return px_load(part[(size_t)v * S]); }, SGB_V, exc);
  if (!pair_all(!exc)) q = sgb_combine_complete(part, S);  // (pair-uniform)
  px_store(part[0], q);
}

// one lane pair per (group, combination): psi(Q) == [x] Q; a failure (or the
// doubling case in the [|x|] chain, which only points of tiny order reach)
// fails the group
__global__ void TBG_LAUNCH_N(TBG_PAIR_WAVES) k_sgb_test(DevBatch B, uint32_t n_sg) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  if (w >= n_sg * SGB_K) return;
  const uint32_t g = w / SGB_K, k = w % SGB_K;
  const G2J& slot = B.sgb_part[sgb_q_slot(B, g, k)];
  bool ok = true;
  if (!jac_is_inf(px_load(slot))) {
    // [|x|] Q with Q re-read from its slot where it is added (held across the
    // doublings it went through scratch every step)
    bool exc = false;
    Jac<Fp2x> m = px_load(slot);
#pragma unroll 1
    for (int i = 62; i >= 0; --i) {
      m = jac_dbl_lo(m);
      if ((X_ABS >> i) & 1) {
        __asm__ __volatile__("" ::: "memory");
        m = jac_add_x(m, px_load(slot), exc);
      }
    }  // psi(Q) == [x] Q == -m
    if (exc || jac_is_inf(m)) {
      ok = false;
    } else {
      __asm__ __volatile__("" ::: "memory");
      const Jac<Fp2x> ps = g2_psi_g(px_load(slot));
      const Fp2x z1 = f_sqr(ps.Z), z2 = f_sqr(m.Z);
      ok = f_eq(f_mul(ps.X, z2), f_mul(m.X, z1)) &&
           f_eq(f_mul(f_mul(ps.Y, m.Z), z2), f_reduce(f_neg(f_mul(f_mul(m.Y, ps.Z), z1))));
    }
  }
  if (!ok && pair_par() == 0) sgb_fail(B, g);
}

void launch_subgroup_batch(const DevBatch& B, hipStream_t st) {
  if (!B.sgb) return;
  const uint32_t n_sg = sgb_groups(B.n_partials, B.sgb_m);
  if (!n_sg) return;
  const bool triple = sgb_triple(B.sgb_m), paired = sgb_paired(B.sgb_m);
  if (triple) {
    const dim3 per_member((B.n_partials + kSgbSortBlock - 1) / kSgbSortBlock);
    (void)hipMemsetAsync(B.sgb_off, 0, 4ull * (SGB_TBUCKETS + 1) * n_sg, st);  // k_sgb_tri_count's counters
    TBG_KLAUNCH(k_sgb_tri_count, per_member, dim3(kSgbSortBlock), st, B);
    TBG_KLAUNCH(k_sgb_tri_scan, dim3(n_sg), dim3(kSgbSortBlock), st, B);
    TBG_KLAUNCH(k_sgb_tri_scatter, per_member, dim3(kSgbSortBlock), st, B);
  } else {
    TBG_KLAUNCH(k_sgb_sort, dim3(n_sg), dim3(kSgbSortBlock), st, B);
  }
  const uint32_t n_t = l0_fused(B) ? sgb_t_slices(B.sgb_m) : 0u;  // the slices of T per group
  // k_sgb_bucket's lane pairs per group
  const uint32_t per_g = triple ? SGB_TRANK : paired ? SGB_PRANK : SGB_BUCKETS * B.sgb_split;
  TBG_KLAUNCH(k_sgb_bucket, grid_for(2 * n_sg * (per_g + n_t)), dim3(kBlock), st, B, n_sg, n_t);
  if (triple) {
    TBG_KLAUNCH(k_sgb_tri_fold, grid_for(2 * n_sg * SGB_TRIPLES * SGB_TF1), dim3(kBlock), st, B, n_sg, 1u);
    TBG_KLAUNCH(k_sgb_tri_fold, grid_for(2 * n_sg * SGB_BUCKETS), dim3(kBlock), st, B, n_sg, 2u);
  } else if (paired || B.sgb_split > 1) {
    TBG_KLAUNCH(k_sgb_fold, grid_for(2 * n_sg * SGB_BUCKETS), dim3(kBlock), st, B, n_sg);
  }
  TBG_KLAUNCH(k_sgb_combine, grid_for(2 * n_sg * SGB_K), dim3(kBlock), st, B, n_sg);
  TBG_KLAUNCH(k_sgb_test, grid_for(2 * n_sg * SGB_K), dim3(kBlock), st, B, n_sg);
}

}  // namespace tbg
