// Level 0 by message: the segmented G1 sums behind
//
//   prod_(d: m_d = m) e(P_d, H(m)) = e(Q_m, H(m)),   Q_m = sum_(d: m_d = m) P_d,
//
// which lets a fused level 0 (tbls_launch.h l0_by_msg) evaluate the 68 stored
// lines of H(m) once per distinct MESSAGE instead of once per duty.  Every DV
// of a cluster signs the same root for its randao, sync-message and selection
// duties (reference core/types.go:41-54) and a committee's attesters share
// their attestation data, so a launch holds far fewer messages than duties.
//
// Written per lane over a plain view of the arrays, so that the kernels
// (k_l0msg.hip) and the host twin (tests/l0msg) run the same code:
//
//   plan (host, l0m_sort_batch / l0m_chunk_plan): the launch's duties sorted
//     by message (CSR: msg_first, msg_duty; duties ascending inside a
//     message), every message cut into chunks of L0M_CHUNK duties;
//   l0m_chunk_lane: one lane per chunk, the mixed additions of its combined
//     duties' P_d;
//   l0m_fold_lane: pass p folds L0M_FAN chunk sums at stride L0M_FAN^p into
//     the first of them -- no lane's chain grows with the largest message;
//     the host knows the pass count from that message's chunks (l0m_passes);
//   l0m_msg_lane: one lane per message, the <= L0M_FAN sums the passes left;
//     the kernel then makes Q_m affine with one batched inversion.
//
// Operands: dv_p[d] holds P_d as (-x, y), the Miller steps' operand form; x
// is negated back before adding and Q_m is stored as (-x, y) again.  Only
// duties with dv_state == RLC_COMBINED are members, as in the Miller kernel.
// Group law: the cheap additions (bls_pair.h jac_add_aff_x / jac_add_x: no
// doubling branch; P == -Q and an infinite accumulator handled) and, when one
// of them met two equal operands, the same sum again with the complete
// formulas -- two duties that share a key set and draw equal scalars are
// unlikely, a replayed duty list makes equal chunk sums certain.
#pragma once
#include "bls_pair.h"

namespace tbg {

#ifndef TBG_L0M_CHUNK
#define TBG_L0M_CHUNK 16
#endif
#ifndef TBG_L0M_FAN
#define TBG_L0M_FAN 8
#endif
constexpr uint32_t L0M_CHUNK = TBG_L0M_CHUNK;  // duties per chunk lane (mixed additions)
constexpr uint32_t L0M_FAN = TBG_L0M_FAN;      // chunk sums per lane of a fold pass (Jacobian additions)
constexpr int32_t L0M_COMBINED = 1;            // RLC_COMBINED (tbls_launch.h; asserted in k_l0msg.hip)

// Per-message state of a launch's message sums.
enum L0mState : int32_t {
  L0M_EMPTY = 0,       // no combined duty names the message: its slot is skipped
  L0M_SUMMED = 1,      // Q_m stored
  L0M_DEGENERATE = 2,  // the combined duties' P_d sum to infinity: level 0 is void
};

TBG_HD uint32_t l0m_chunks_of(uint32_t n_duties) { return (n_duties + L0M_CHUNK - 1) / L0M_CHUNK; }
// Fold passes before the per-message lane, which takes <= L0M_FAN sums at
// stride L0M_FAN^passes.
TBG_HD uint32_t l0m_passes(uint32_t max_chunks) {
  uint32_t p = 0;
  for (uint64_t s = 1; s * L0M_FAN < max_chunks; s *= L0M_FAN) ++p;
  return p;
}
TBG_HD uint64_t l0m_stride(uint32_t pass) {
  uint64_t s = 1;
  for (uint32_t k = 0; k < pass; ++k) s *= L0M_FAN;
  return s;
}
// Chunks a launch of n_msgs messages over n_duties duties can have at most.
TBG_HD uint64_t l0m_chunk_bound(uint64_t n_msgs, uint64_t n_duties) { return n_msgs + n_duties / L0M_CHUNK; }

struct L0mView {
  uint32_t n_msgs;
  const uint32_t* msg_first;    // [n_msgs + 1] CSR offsets into msg_duty
  const uint32_t* msg_duty;     // [n_duties] duties by message, ascending inside a message
  const uint32_t* chunk_first;  // [n_msgs + 1] first chunk of each message
  const uint32_t* chunk_msg;    // [n_chunks] message of each chunk
  const G1A* dv_p;              // [n_duties] P_d as (-x, y)
  const int32_t* dv_state;      // [n_duties]
  G1J* part;                    // [n_chunks] chunk sums, folded in place
  uint32_t* cnt;                // [n_chunks] combined duties in the sum, folded with it
};

// ---- host plan ------------------------------------------------------------
// Counting sort of ONE caller batch's duties [d0, d0 + nd) by message; its
// messages are [m0, m0 + nm) and duty_msg holds launch-wide indices.  Writes
// msg_first[m0 + 1 .. m0 + nm] and msg_duty[d0 .. d0 + nd): disjoint from
// every other batch's, so the batches sort in parallel.  (msg_first[m0] = d0
// is the previous batch's last entry; msg_first[0] = 0 is the caller's.)
inline void l0m_sort_batch(const uint32_t* duty_msg, uint32_t d0, uint32_t nd, uint32_t m0, uint32_t nm,
                           uint32_t* msg_first, uint32_t* msg_duty, uint32_t* cursor /* [nm] scratch */) {
  for (uint32_t m = 0; m < nm; ++m) cursor[m] = 0;
  for (uint32_t d = 0; d < nd; ++d) ++cursor[duty_msg[d0 + d] - m0];
  uint32_t run = d0;
  for (uint32_t m = 0; m < nm; ++m) {
    const uint32_t c = cursor[m];
    cursor[m] = run;
    run += c;
    msg_first[m0 + m + 1] = run;
  }
  for (uint32_t d = 0; d < nd; ++d) msg_duty[cursor[duty_msg[d0 + d] - m0]++] = d0 + d;
}
// The chunk plan of messages [m0, m0 + nm), continuing at chunk *n_chunks
// (chunk_first[m0] is written here too); returns the largest message's chunks.
inline uint32_t l0m_chunk_plan(const uint32_t* msg_first, uint32_t m0, uint32_t nm, uint32_t* chunk_first,
                               uint32_t* chunk_msg, uint32_t* n_chunks) {
  uint32_t nc = *n_chunks, largest = 0;
  for (uint32_t m = m0; m < m0 + nm; ++m) {
    chunk_first[m] = nc;
    const uint32_t k = l0m_chunks_of(msg_first[m + 1] - msg_first[m]);
    for (uint32_t j = 0; j < k; ++j) chunk_msg[nc++] = m;
    if (k > largest) largest = k;
  }
  chunk_first[m0 + nm] = nc;
  *n_chunks = nc;
  return largest;
}

// ---- lanes ----------------------------------------------------------------
template <bool FAST>
TBG_HD G1J l0m_chunk_sum(const L0mView& V, uint32_t j0, uint32_t j1, uint32_t& n, bool& exc) {
  G1J acc = jac_inf<Fp>();
  n = 0;
#pragma unroll 1
  for (uint32_t j = j0; j < j1; ++j) {
    const uint32_t d = V.msg_duty[j];
    if (V.dv_state[d] != L0M_COMBINED) continue;
    G1A p = V.dv_p[d];
    p.x = fp_reduce(fp_neg(p.x));
    if constexpr (FAST) acc = jac_add_aff_x(acc, p, exc);
    else acc = jac_add_aff(acc, p);  // (complete; out of line on the device)
    ++n;
  }
  return acc;
}
// Chunk c: the sum of its combined duties' P_d.  redo = false is the tests'
// control (the cheap formula's result kept); *met says whether an addition
// met two equal operands.
TBG_HD void l0m_chunk_lane(const L0mView& V, uint32_t c, bool redo = true, bool* met = nullptr) {
  const uint32_t m = V.chunk_msg[c];
  const uint32_t j0 = V.msg_first[m] + (c - V.chunk_first[m]) * L0M_CHUNK;
  const uint32_t j1 = j0 + L0M_CHUNK < V.msg_first[m + 1] ? j0 + L0M_CHUNK : V.msg_first[m + 1];
  uint32_t n = 0;
  bool exc = false;
  G1J acc = l0m_chunk_sum<true>(V, j0, j1, n, exc);
  if (exc) {
    if (met) *met = true;
    if (redo) acc = l0m_chunk_sum<false>(V, j0, j1, n, exc);
  }
  V.part[c] = acc;
  V.cnt[c] = n;
}

template <bool FAST>
TBG_HD G1J l0m_part_sum(const L0mView& V, uint32_t c0, uint32_t c1, uint64_t stride, uint32_t& n, bool& exc) {
  G1J acc = V.part[c0];
  n = V.cnt[c0];
#pragma unroll 1
  for (uint64_t c = c0 + stride; c < c1; c += stride) {
    if constexpr (FAST) acc = jac_add_x(acc, V.part[c], exc);
    else acc = jac_add(acc, V.part[c]);
    n += V.cnt[c];
  }
  return acc;
}
// Fold pass at `stride` (L0M_FAN^pass), one lane per chunk: the chunk whose
// index in its message is a multiple of stride * L0M_FAN takes the sums at
// stride behind it (inside the message) into its own slot; the others idle.
// A pass reads only slots that no lane of the same pass writes.
TBG_HD void l0m_fold_lane(const L0mView& V, uint32_t c, uint64_t stride, bool redo = true, bool* met = nullptr) {
  const uint32_t m = V.chunk_msg[c];
  const uint32_t l = c - V.chunk_first[m], k = V.chunk_first[m + 1] - V.chunk_first[m];
  if (l % (stride * L0M_FAN) != 0 || l + stride >= k) return;
  const uint64_t e = l + stride * L0M_FAN;
  const uint32_t c1 = V.chunk_first[m] + (uint32_t)(e < k ? e : k);
  uint32_t n = 0;
  bool exc = false;
  G1J acc = l0m_part_sum<true>(V, c, c1, stride, n, exc);
  if (exc) {
    if (met) *met = true;
    if (redo) acc = l0m_part_sum<false>(V, c, c1, stride, n, exc);
  }
  V.part[c] = acc;
  V.cnt[c] = n;
}
// Message m after the fold passes: the sum of its <= L0M_FAN remaining sums
// (Jacobian; the caller converts) and its state.
TBG_HD int32_t l0m_msg_lane(const L0mView& V, uint32_t m, uint64_t stride, G1J& sum, bool redo = true,
                            bool* met = nullptr) {
  const uint32_t c0 = V.chunk_first[m], c1 = V.chunk_first[m + 1];
  sum = jac_inf<Fp>();
  if (c0 == c1) return L0M_EMPTY;  // no duty names the message
  uint32_t n = 0;
  bool exc = false;
  sum = l0m_part_sum<true>(V, c0, c1, stride, n, exc);
  if (exc) {
    if (met) *met = true;
    if (redo) sum = l0m_part_sum<false>(V, c0, c1, stride, n, exc);
  }
  if (n == 0) return L0M_EMPTY;
  return jac_is_inf(sum) ? L0M_DEGENERATE : L0M_SUMMED;
}
// Q_m in the Miller steps' operand form from the Jacobian sum and 1 / Z.
TBG_HD G1A l0m_operand(const G1J& sum, const Fp& zinv) {
  const Fp zi2 = fp_sqr(zinv);
  return G1A{fp_reduce(fp_neg(fp_mul(sum.X, zi2))), fp_mul(sum.Y, fp_mul(zi2, zinv))};
}

}  // namespace tbg
