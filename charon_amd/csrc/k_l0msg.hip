// Level 0 by message (tbls_launch.h l0_by_msg): in a fused launch whose
// duties share messages, the duties' key sums P_d are added per distinct
// message (bls_l0msg.h) and level 0's Miller side pairs ONE point Q_m with
// each H(m):
//
//   prod_m e(Q_m, H(m)) * e(-g1, S) == 1,   Q_m = sum_(d: m_d = m) P_d.
//
// k_l0m_chunks / k_l0m_msgs form Q_m after P_d is written (launch_rlc_prepare);
// k_l0m_miller is k_miller_hex<MILLER_L0>'s body (k_miller_hex.hip) with the
// duty d, its P_d and its message replaced by the message slot m, Q_m and m;
// k_l0m_fold is k_l0_fold over groups of message slots.  Their products go
// to chunk_f / grp_f in the layout of the per-duty form for ceil(n_msgs / G)
// groups, and the product tree, the final exponentiation and k_l0_after run
// unchanged (k_rlc.hip).  A void or failed fused level 0 keeps none of this.
// Reference: the pairing products behind tbls.Verify (tbls/tss.go:190-197).
#ifndef TBG_SCHED_FENCE
#define TBG_SCHED_FENCE 1  // products in program order, as k_miller_hex.hip
#endif
#include "tbls_launch.h"
#include "bls_lines.h"
#include "bls_hex.h"
#include "bls_batchinv.h"
#include "bls_l0msg.h"

namespace tbg {

static_assert(L0M_COMBINED == RLC_COMBINED, "bls_l0msg.h names the combined state by value");
constexpr int L0M_QUAD_WORDS = 4 * NL;
constexpr uint32_t L0M_HOIST_MAX = 16;  // (k_miller_hex.hip HEX_HOIST_MAX)
// k_l0m_miller keeps the index of H(m)'s lines apart from the slot index of
// Q_m, as k_miller_hex has a duty and its message: told that they are one
// value, the register allocator merges the two address chains and spills 7
// VGPRs where that kernel spills 2; with the message index opaque, none.
#define L0M_OPAQUE(v) asm volatile("" : "+v"(v))

__device__ __forceinline__ L0mView l0m_view(const DevBatch& B) {
  return L0mView{B.n_msgs, B.msg_first, B.msg_duty, B.l0m_chunk_first, B.l0m_chunk_msg,
                 B.dv_p,   B.dv_state,  B.l0m_part, B.l0m_cnt};
}

// One lane per chunk of a message's duties: the chunk's sum of P_d.
__global__ void TBG_LAUNCH k_l0m_chunks(DevBatch B) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  // (a void level 0 -- set by an earlier kernel: grid-uniform -- has no P_d to sum)
  if (c >= B.l0m_n_chunks || B.counters[CNT_L0_BAD]) return;
  l0m_chunk_lane(l0m_view(B), c);
}

// A message's chunk sums folded and made affine, in bounded passes: `last`
// = 0 is a fold pass at `stride` (one lane per chunk, most idle: L0M_FAN
// additions at the most per lane), `last` = 1 the final pass (one lane per
// message: the <= L0M_FAN sums left, Q_m by one batched inversion per
// workgroup, the message's state; a degenerate sum voids level 0).
__global__ void __launch_bounds__(BINV_BLOCK) k_l0m_msgs(DevBatch B, uint32_t stride, uint32_t last) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const L0mView V = l0m_view(B);
  if (!last) {
    if (t < B.l0m_n_chunks && !B.counters[CNT_L0_BAD]) l0m_fold_lane(V, t, stride);
    return;
  }
  // (no early return on CNT_L0_BAD: other workgroups of this kernel set it,
  // and every thread must reach the batched inversion's barriers; a lane that
  // sees it set only skips its sums, which nothing reads after a void level 0)
  const bool in = t < B.n_msgs && !B.counters[CNT_L0_BAD];
  G1J sum = jac_inf<Fp>();
  const int32_t state = in ? l0m_msg_lane(V, t, stride, sum) : (int32_t)L0M_EMPTY;
  const bool present = state == L0M_SUMMED;
  const Fp zi = block_batch_inv<BINV_WAVES>(sum.Z, present);
  if (!in) return;
  B.l0m_state[t] = state;
  if (present) B.l0m_q[t] = l0m_operand(sum, zi);
  if (state == L0M_DEGENERATE) B.counters[CNT_L0_BAD] = 1;
}

// One hexad per (group of G message slots, chunk of C of them), then ONE S
// hexad for the batch-wide S (batch lines, -g1 folded in) in a wave of its
// own.  A slot runs when its message has a sum and a usable H(m); a summed
// message whose H(m) is unusable fails the check in k_l0m_fold.
__global__ void TBG_LAUNCH_N(TBG_HEX_WAVES) k_l0m_miller(DevBatch B) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t G = B.rlc_group, C = B.rlc_chunk;
  const uint32_t n_groups = (B.n_msgs + G - 1) / G;
  const uint32_t nch = (G + C - 1) / C, nq = nch + 1;
  const uint32_t np_q = n_groups * nch;
  const uint32_t qd = hex_slot(t);
  if (qd == 0xFFFFFFFFu || qd > np_q) return;
  // a void fused level 0 keeps nothing
  if (B.counters[CNT_L0_BAD]) return;
  const bool s_quad = qd == np_q;
  const uint32_t* ls = nullptr;
  uint32_t* dst;
  uint32_t m0 = 0, m1 = 0;
  if (s_quad) {
    ls = B.batch_lines;
    dst = B.batch_f;
  } else {
    const uint32_t g = qd / nch, c = qd % nch;
    m0 = g * G + c * C;
    m1 = min(m0 + C, min(g * G + G, B.n_msgs));
    if (m0 > m1) m0 = m1;  // (a chunk past the last group's messages)
    dst = B.chunk_f + (size_t)3 * L0M_QUAD_WORDS * (g * nq + c);
  }
  Fp4h f = hex_one();
  int idx = 0;
  // The chunk's slots are decided once, not at every one of the 68 steps: a
  // bit per slot whose line products run.  Chunks longer than L0M_HOIST_MAX
  // slots keep the per-step test.
  __shared__ uint32_t s_msg[kBlock * L0M_HOIST_MAX];
  uint32_t* my_msg = s_msg + L0M_HOIST_MAX * threadIdx.x;
  const bool hoist = m1 - m0 <= L0M_HOIST_MAX;
  uint32_t run = 0;
  if (hoist) {
    for (uint32_t m = m0; m < m1; ++m) {
      if (B.l0m_state[m] != L0M_SUMMED) continue;
      uint32_t hm = m;  // the slot's message is the slot itself
      L0M_OPAQUE(hm);
      if (B.h_status[hm] != 0) continue;
      my_msg[m - m0] = hm;
      run |= 1u << (m - m0);
    }
  }
#pragma unroll 1
  for (int b = 62; b >= 0; --b) {
    if (b != 62) f = hex_sqr(f);
    const int steps = ((X_ABS >> b) & 1) ? 2 : 1;
#pragma unroll 1
    for (int s = 0; s < steps; ++s, ++idx) {
      if (s_quad) f = hex_line_folded(f, ls, idx);
      if (hoist) {
#pragma unroll 1
        for (uint32_t bits = run; bits; bits &= bits - 1) {
          const uint32_t j = __builtin_ctz(bits);
          f = hex_line_at_v(f, B.h_lines + (size_t)LINES_WORDS * my_msg[j], idx, hex_line_operand(B.l0m_q[m0 + j]));
        }
        continue;
      }
#pragma unroll 1
      for (uint32_t m = m0; m < m1; ++m) {
        if (B.l0m_state[m] != L0M_SUMMED) continue;
        uint32_t hm = m;
        L0M_OPAQUE(hm);
        if (B.h_status[hm] != 0) continue;
        f = hex_line_at_v(f, B.h_lines + (size_t)LINES_WORDS * hm, idx, hex_line_operand(B.l0m_q[m]));
      }
    }
  }
  hex_store(dst, f);
}

// One hexad per group of message slots: the product of its chunks' values
// into grp_f (the product tree's input); a summed message whose H(m) is
// unusable makes level 0 fail, the rule k_l0_fold applies per duty.
__global__ void TBG_LAUNCH_N(TBG_HEX_WAVES) k_l0m_fold(DevBatch B) {
  TBG_URGENT();
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t G = B.rlc_group, C = B.rlc_chunk;
  const uint32_t n_groups = (B.n_msgs + G - 1) / G, nch = (G + C - 1) / C, nq = nch + 1;
  const uint32_t g = hex_slot(t);
  if (g >= n_groups || B.counters[CNT_L0_BAD]) return;
  const uint32_t m0 = g * G, m1 = min(m0 + G, B.n_msgs);
  for (uint32_t m = m0; m < m1; ++m) {
    if (B.l0m_state[m] == L0M_SUMMED && B.h_status[m] != 0) {
      if (hex_lead()) B.counters[CNT_L0_BAD] = 1;
      return;
    }
  }
  const uint32_t* base = B.chunk_f + (size_t)3 * L0M_QUAD_WORDS * nq * g;
  Fp4h f = hex_load(base);
  for (uint32_t c = 1; c < nch; ++c) f = hex_mul(f, hex_load(base + (size_t)3 * L0M_QUAD_WORDS * c));
  hex_store(B.grp_f + (size_t)3 * L0M_QUAD_WORDS * g, f);
}

void launch_l0m_sums(const DevBatch& B, hipStream_t st) {
  if (B.l0m_n_chunks) {
    TBG_KLAUNCH(k_l0m_chunks, grid_for(B.l0m_n_chunks), dim3(kBlock), st, B);
    const uint32_t passes = l0m_passes(B.l0m_max_chunks);
    for (uint32_t p = 0; p < passes; ++p)
      TBG_KLAUNCH(k_l0m_msgs, dim3((B.l0m_n_chunks + BINV_BLOCK - 1) / BINV_BLOCK), dim3(BINV_BLOCK), st, B,
                  (uint32_t)l0m_stride(p), 0u);
  }
  TBG_KLAUNCH(k_l0m_msgs, dim3((B.n_msgs + BINV_BLOCK - 1) / BINV_BLOCK), dim3(BINV_BLOCK), st, B,
              (uint32_t)l0m_stride(l0m_passes(B.l0m_max_chunks)), 1u);
}

void launch_l0m_miller(const DevBatch& B, hipStream_t st) {
  const uint32_t n_groups = l0m_groups(B);
  const uint32_t nch = (B.rlc_group + B.rlc_chunk - 1) / B.rlc_chunk;
  TBG_KLAUNCH(k_l0m_miller, grid_for(hex_threads(n_groups * nch + 1)), dim3(kBlock), st, B);
  TBG_KLAUNCH(k_l0m_fold, grid_for(hex_threads(n_groups)), dim3(kBlock), st, B);
}

}  // namespace tbg
