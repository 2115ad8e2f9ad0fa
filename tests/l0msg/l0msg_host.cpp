// TEST TOOLING ONLY: host (CPU) twin of level 0's message sums
// (charon_amd/csrc/bls_l0msg.h: the plan the engine packs, and the lanes that
// k_l0m_chunks / k_l0m_msgs run) for tests/test_l0msg_host.py, with the value
// bound checks (TBG_BOUNDS_CHECK) switched on.  Modelled on tests/l0straus.
// Built with -DL0MSG_MAIN it is a stand-alone program (its own main) for the
// host sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../charon_amd/csrc/bls_pairing.h"
#include "../../charon_amd/csrc/bls_batchinv.h"
#include "../../charon_amd/csrc/bls_l0msg.h"

extern "C" unsigned long long tbg_mad_count = 0;

using namespace tbg;

extern "C" {

// [L0M_CHUNK, L0M_FAN, L0M_EMPTY, L0M_SUMMED, L0M_DEGENERATE]
void lm_consts(uint32_t* out5) {
  out5[0] = L0M_CHUNK;
  out5[1] = L0M_FAN;
  out5[2] = (uint32_t)L0M_EMPTY;
  out5[3] = (uint32_t)L0M_SUMMED;
  out5[4] = (uint32_t)L0M_DEGENERATE;
}
uint32_t lm_passes(uint32_t max_chunks) { return l0m_passes(max_chunks); }

// The plan of a grouped pack as tbg_submit_group builds it: n_batches caller
// batches, batch k with nd[k] duties over nm[k] messages of its own,
// duty_msg[k-th batch's duties] LOCAL message indices (rebased here as the
// engine's pack does).  Outputs: msg_first [M + 1], msg_duty [D], chunk_first
// [M + 1], chunk_msg [>= l0m_chunk_bound(M, D)], per batch ch1 / maxch (the
// prefix's chunk count and largest message).  Returns the chunk count.
int lm_plan(const uint32_t* duty_msg_local, const uint32_t* nd, const uint32_t* nm, uint32_t n_batches,
            uint32_t* msg_first, uint32_t* msg_duty, uint32_t* chunk_first, uint32_t* chunk_msg, uint32_t* ch1,
            uint32_t* maxch) {
  uint32_t D = 0, M = 0;
  for (uint32_t k = 0; k < n_batches; ++k) {
    D += nd[k];
    M += nm[k];
  }
  std::vector<uint32_t> dm(D);
  uint32_t d0 = 0, m0 = 0;
  for (uint32_t k = 0; k < n_batches; ++k) {
    for (uint32_t d = 0; d < nd[k]; ++d) {
      if (duty_msg_local[d0 + d] >= nm[k]) return -1;
      dm[d0 + d] = m0 + duty_msg_local[d0 + d];
    }
    d0 += nd[k];
    m0 += nm[k];
  }
  msg_first[0] = 0;
  // (backwards: the batches' sections are disjoint, so their order is free)
  for (uint32_t k = n_batches; k-- > 0;) {
    d0 = m0 = 0;
    for (uint32_t j = 0; j < k; ++j) {
      d0 += nd[j];
      m0 += nm[j];
    }
    std::vector<uint32_t> cursor(nm[k]);
    l0m_sort_batch(dm.data(), d0, nd[k], m0, nm[k], msg_first, msg_duty, cursor.data());
  }
  uint32_t nc = 0, largest = 0;
  m0 = 0;
  for (uint32_t k = 0; k < n_batches; ++k) {
    const uint32_t big = l0m_chunk_plan(msg_first, m0, nm[k], chunk_first, chunk_msg, &nc);
    if (big > largest) largest = big;
    ch1[k] = nc;
    maxch[k] = largest;
    m0 += nm[k];
  }
  if (nc > l0m_chunk_bound(M, D)) return -2;
  return (int)nc;
}

// The message sums of one launch: n_duties duties with P_d (48-byte
// compressed; stored as the engine stores it, (-x, y)), dv_state and
// duty_msg over n_msgs messages.  Every lane of k_l0m_chunks, of the fold
// passes and of the final pass of k_l0m_msgs runs in turn, the final pass's
// inversion batched in workgroups of 64 (batch_inv_emulate).  redo = 0 is
// the control: the cheap formulas' results are kept; *met says whether an
// addition met two equal operands.  Outputs per message: Q_m compressed
// (x negated back; the identity when not summed) and its state.  Returns the
// fold passes run, or a negative error.
int lm_run(const uint8_t* pd48, const int32_t* dv_state, uint32_t n_duties, const uint32_t* duty_msg, uint32_t n_msgs,
           int redo, uint8_t* q48, int32_t* state, int* met) {
  if (!n_duties || !n_msgs) return -1;
  std::vector<G1A> dv_p(n_duties);
  for (uint32_t d = 0; d < n_duties; ++d) {
    if (duty_msg[d] >= n_msgs) return -1;
    G1A p;
    const int32_t rc = g1_decompress(pd48 + 48ull * d, p);
    if (rc == DEC_IDENTITY) {  // (only behind a non-combined state: the engine never stores infinity)
      if (dv_state[d] == L0M_COMBINED) return -3;
      p = G1A{fp_zero(), fp_zero()};
    } else if (rc != DEC_OK) {
      return -2;
    }
    dv_p[d] = G1A{fp_reduce(fp_neg(p.x)), p.y};
  }
  std::vector<uint32_t> msg_first(n_msgs + 1), msg_duty(n_duties), chunk_first(n_msgs + 1),
      chunk_msg((size_t)l0m_chunk_bound(n_msgs, n_duties) + 1), cursor(n_msgs);
  msg_first[0] = 0;
  l0m_sort_batch(duty_msg, 0, n_duties, 0, n_msgs, msg_first.data(), msg_duty.data(), cursor.data());
  uint32_t nc = 0;
  const uint32_t largest = l0m_chunk_plan(msg_first.data(), 0, n_msgs, chunk_first.data(), chunk_msg.data(), &nc);
  std::vector<G1J> part(nc + 1);
  std::vector<uint32_t> cnt(nc + 1);
  const L0mView V{n_msgs,      msg_first.data(), msg_duty.data(), chunk_first.data(), chunk_msg.data(),
                  dv_p.data(), dv_state,         part.data(),     cnt.data()};
  bool any = false;
  for (uint32_t c = 0; c < nc; ++c) l0m_chunk_lane(V, c, redo != 0, &any);
  const uint32_t passes = l0m_passes(largest);
  for (uint32_t p = 0; p < passes; ++p)
    for (uint32_t c = 0; c < nc; ++c) l0m_fold_lane(V, c, l0m_stride(p), redo != 0, &any);
  std::vector<G1J> sum(n_msgs);
  std::vector<Fp> z(n_msgs), zi(n_msgs);
  std::vector<uint8_t> present(n_msgs);
  for (uint32_t m = 0; m < n_msgs; ++m) {
    state[m] = l0m_msg_lane(V, m, l0m_stride(passes), sum[m], redo != 0, &any);
    present[m] = state[m] == L0M_SUMMED;
    z[m] = sum[m].Z;
  }
  batch_inv_emulate(z.data(), (const bool*)present.data(), zi.data(), (int)n_msgs, 1);
  for (uint32_t m = 0; m < n_msgs; ++m) {
    G1A q{fp_zero(), fp_zero()};
    if (present[m]) {
      q = l0m_operand(sum[m], zi[m]);
      q.x = fp_reduce(fp_neg(q.x));
    }
    g1_compress(q, !present[m], q48 + 48ull * m);
  }
  if (met) *met = any ? 1 : 0;
  return (int)passes;
}

}  // extern "C"

#ifdef L0MSG_MAIN
// Stand-alone run for the host sanitizers: multiples of the generator spread
// over a few messages (interleaved, one message unused, one all non-combined,
// a duplicate pair and an opposite pair), the plan of a two-batch pack.
int main() {
  const uint32_t n = 3 * L0M_CHUNK * L0M_FAN + 5, nm = 6;
  std::vector<uint8_t> pd(48ull * n);
  std::vector<int32_t> st(n, L0M_COMBINED);
  std::vector<uint32_t> dm(n);
  const G1A g{fp_from_const(G1_X), fp_reduce(fp_neg(fp_from_const(G1_NEG_Y)))};
  G1J acc = jac_from_aff(g);
  for (uint32_t d = 0; d < n; ++d) {
    G1A a;
    if (!jac_to_aff(acc, a)) return 2;
    if (d == 7) a.y = fp_reduce(fp_neg(a.y));  // -[8]g next to ...
    g1_compress(a, false, pd.data() + 48ull * d);
    if (d != 3 && d != 6) acc = jac_add_aff(acc, g);  // (duties 3, 4 and 6, 7 hold equal multiples)
    dm[d] = d < 40 ? d % 2 : (d % 16 == 0 ? 4 : 2);   // message 3 unused, 5 below
  }
  dm[n - 1] = dm[n - 2] = 5;
  st[n - 1] = st[n - 2] = 0;
  std::vector<uint8_t> q(48ull * nm);
  std::vector<int32_t> ms(nm);
  int met = 0;
  const int passes = lm_run(pd.data(), st.data(), n, dm.data(), nm, 1, q.data(), ms.data(), &met);
  std::printf("passes %d met %d states", passes, met);
  for (uint32_t m = 0; m < nm; ++m) std::printf(" %d", ms[m]);
  std::printf("\n");
  if (passes < 1 || ms[3] != L0M_EMPTY || ms[5] != L0M_EMPTY || ms[0] != L0M_SUMMED) return 1;
  const uint32_t nd2[2] = {n / 2, n - n / 2}, nm2[2] = {nm, nm};
  std::vector<uint32_t> mf(2 * nm + 1), md(n), cf(2 * nm + 1), cm((size_t)l0m_chunk_bound(2 * nm, n) + 1);
  uint32_t ch1[2], maxch[2];
  const int nc = lm_plan(dm.data(), nd2, nm2, 2, mf.data(), md.data(), cf.data(), cm.data(), ch1, maxch);
  std::printf("plan chunks %d prefix %u\n", nc, ch1[0]);
  return nc > 0 && (uint32_t)nc == ch1[1] ? 0 : 1;
}
#endif
