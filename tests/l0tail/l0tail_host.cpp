// TEST TOOLING ONLY: host (CPU) build of the fused level 0's S role
// (charon_amd/csrc/bls_l0tail.h l0t_block, the body the first workgroups of
// k_rlc_g1_l0's grid run) for tests/test_l0_tail_host.py: the same block
// function over a host environment -- the 32 lane pairs of a block in a loop
// (Fp2p), the tree's schedule as the device runs it, the hand-off counters as
// plain words -- with the value bound checks (TBG_BOUNDS_CHECK) switched on.
// The caller chooses the order in which the blocks run.  Modelled on
// tests/l0fused.
#include <array>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../charon_amd/csrc/bls_pairing.h"
#include "../../charon_amd/csrc/bls_h2c.h"
#include "../../charon_amd/csrc/bls_l0tail.h"

extern "C" unsigned long long tbg_mad_count = 0;

using namespace tbg;

namespace {

Jac<Fp2p> from_g2j(const G2J& p) { return {pp_from(p.X), pp_from(p.Y), pp_from(p.Z)}; }
G2J to_g2j(const Jac<Fp2p>& p) { return {pp_to(p.X), pp_to(p.Y), pp_to(p.Z)}; }

struct HostEnv {
  using F = Fp2p;
  using V = std::array<Jac<Fp2p>, L0T_PAIRS>;
  const G2J* q;        // [n_sg][L0T_QCOLS] Q_k of each group
  const G2J* t;        // [n_sg * n_t] slices of T
  G2J* sum;            // [l0t_sum_entries]
  uint32_t* counters;  // [L0T_COLS] per column, then columns done
  G2A* out;            // S
  uint32_t* bad;       // the S = 0 flag
  uint32_t* finishes;  // blocks that reached finish()
  uint32_t acquires = 0;
  bool acquired = false;  // since this block's last arrival

  template <class Fn>
  V per_pair(uint32_t n, Fn&& f) {
    V v;
    for (uint32_t pr = 0; pr < L0T_PAIRS; ++pr) v[pr] = pr < n ? f(pr) : jac_inf<Fp2p>();
    return v;
  }
  Jac<Fp2p> tree(V v, uint32_t n) {
    for (uint32_t s = 1; s < n; s <<= 1) {
      const V snap = v;  // (the device's LDS image of the level)
      for (uint32_t pr = 0; pr < L0T_PAIRS; ++pr)
        if ((pr & (2 * s - 1)) == 0 && pr + s < n) v[pr] = jac_add(v[pr], snap[pr + s]);
    }
    return v[0];
  }
  Jac<Fp2p> load_q(uint32_t g, uint32_t col) { return from_g2j(q[(size_t)L0T_QCOLS * g + col]); }
  Jac<Fp2p> load_t(uint32_t a) { return from_g2j(t[a]); }
  // (another block's sums may only be loaded behind an acquire)
  Jac<Fp2p> load_sum(uint32_t i) {
    if (!acquired) abort();
    return from_g2j(sum[i]);
  }
  void store_sum(uint32_t i, const Jac<Fp2p>& p) { sum[i] = to_g2j(p); }
  uint32_t arrive_col(uint32_t col) {
    acquired = false;
    return counters[col]++;
  }
  uint32_t arrive_done() {
    acquired = false;
    return counters[L0T_COLS]++;
  }
  void acquire() {
    acquired = true;
    ++acquires;
  }
  void finish(const Jac<Fp2p>& S) {
    ++*finishes;
    if (jac_is_inf(S)) {
      *bad = 1;
      return;
    }
    const Fp2p zi = f_inv(S.Z), zi2 = f_sqr(zi);
    *out = G2A{pp_to(f_mul(S.X, zi2)), pp_to(f_mul(S.Y, f_mul(zi2, zi)))};
  }
};

// [k] base by double-and-add (k = 0: the point at infinity)
Jac<Fp2p> small_mul(const Aff<Fp2p>& base, uint32_t k) {
  Jac<Fp2p> acc = jac_inf<Fp2p>();
  for (int bit = 31; bit >= 0; --bit) {
    acc = jac_dbl(acc);
    if ((k >> bit) & 1u) acc = jac_add_aff_in(acc, base);
  }
  return acc;
}

int compress(const Jac<Fp2p>& S, uint8_t* out96) {
  G2A a{};
  const bool fin = !jac_is_inf(S);
  if (fin) {
    const Fp2p zi = f_inv(S.Z), zi2 = f_sqr(zi);
    a = G2A{pp_to(f_mul(S.X, zi2)), pp_to(f_mul(S.Y, f_mul(zi2, zi)))};
  }
  g2_compress(a, !fin, out96);
  return fin ? 0 : 1;
}

}  // namespace

extern "C" {

uint32_t l0t_hc_blocks(uint32_t n_sg, uint32_t n_t) { return l0t_blocks(l0t_shape(n_sg, n_t)); }
uint32_t l0t_hc_chunks(uint32_t n_sg, uint32_t n_t, uint32_t col) {
  const L0tShape sh = l0t_shape(n_sg, n_t);
  return col < L0T_QCOLS ? sh.wq : sh.wt;
}

// The role on n_sg groups with n_t slices of T each.  Inputs as multiples of
// `base96` (a compressed G2 point): qk[n_sg][18] and tk[n_sg * n_t].  The
// blocks run in the order `order[0 .. blocks)` (a permutation).
//   out_role96   S as the role leaves it (compressed; infinity when it set the flag)
//   out_ref96    S = sum_j psi^j(2 A_j + T) with every column summed point by
//                point and the Horner steps as tests/l0fused forms them
//   stats[4]     finishes, the flag, acquires, the position in `order` of the block that finished
//   counters20   the hand-off counters afterwards
// 0, or a negative error.
int l0t_hc_run(const uint8_t* base96, uint32_t n_sg, uint32_t n_t, const uint32_t* qk, const uint32_t* tk,
               const uint32_t* order, uint8_t* out_role96, uint8_t* out_ref96, uint32_t* stats, uint32_t* counters20) {
  G2A b;
  if (g2_decompress(base96, b) != DEC_OK) return -1;
  const Aff<Fp2p> base{pp_from(b.x), f_reduce(pp_from(b.y))};
  const L0tShape sh = l0t_shape(n_sg, n_t);
  std::vector<G2J> q((size_t)n_sg * L0T_QCOLS), t((size_t)n_sg * n_t), sum(l0t_sum_entries(sh));
  for (size_t i = 0; i < q.size(); ++i) q[i] = to_g2j(small_mul(base, qk[i]));
  for (size_t i = 0; i < t.size(); ++i) t[i] = to_g2j(small_mul(base, tk[i]));
  // (poison: a point that belongs to no sum, so a slot read before it was stored changes S)
  for (auto& s : sum) s = to_g2j(small_mul(base, 0x7FFFFFFFu));

  uint32_t counters[L0T_COLS + 1] = {}, bad = 0, finishes = 0, acquires = 0, who = 0xFFFFFFFFu;
  G2A S{};
  const uint32_t blocks = l0t_blocks(sh);
  std::vector<uint8_t> seen(blocks, 0);
  for (uint32_t k = 0; k < blocks; ++k) {
    const uint32_t blk = order[k];
    if (blk >= blocks || seen[blk]) return -2;
    seen[blk] = 1;
    HostEnv env{q.data(), t.data(), sum.data(), counters, &S, &bad, &finishes};
    const uint32_t before = finishes;
    l0t_block(env, sh, blk);
    acquires += env.acquires;
    if (finishes != before) who = k;
  }
  g2_compress(S, bad != 0 || finishes == 0, out_role96);
  stats[0] = finishes;
  stats[1] = bad;
  stats[2] = acquires;
  stats[3] = who;
  for (uint32_t c = 0; c <= L0T_COLS; ++c) counters20[c] = counters[c];

  // the reference: columns point by point, then the Horner form
  std::vector<Jac<Fp2p>> col(L0T_COLS, jac_inf<Fp2p>());
  for (uint32_t g = 0; g < n_sg; ++g)
    for (uint32_t k = 0; k < L0T_QCOLS; ++k)
      col[k] = jac_add_in<Fp2p, true>(col[k], from_g2j(q[(size_t)L0T_QCOLS * g + k]));
  for (size_t i = 0; i < t.size(); ++i) col[L0T_QCOLS] = jac_add_in<Fp2p, true>(col[L0T_QCOLS], from_g2j(t[i]));
  Jac<Fp2p> R = jac_inf<Fp2p>();
  for (int j = 0; j < 4; ++j) {
    const int e0 = l0f_first(j), e1 = l0f_first(j + 1);
    Jac<Fp2p> acc = col[e1 - 1];
    for (int e = e1 - 2; e >= e0; --e) acc = l0f_mul13_add(acc, col[e]);
    R = jac_add_in<Fp2p, true>(R, l0f_term(acc, col[L0T_QCOLS], j));
  }
  compress(R, out_ref96);
  return 0;
}

}  // extern "C"
