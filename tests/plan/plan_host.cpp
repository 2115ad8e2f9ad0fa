// TEST TOOLING ONLY: C entry points over charon_amd/csrc/tbls_plan.h -- the
// launch plan, the section layout, bind over fake base addresses and the
// replay fit rule -- and over tbls_work.h, the workspaces of the one-shot
// calls, for tests/test_plan_host.py; and over the fallback lists' pass
// schedule and grid-stride loops (tbls_launch.h fb_passes / fb_pass_loop, the
// slot geometry of bls_hex.h), for tests/test_fb_passes_host.py.  Plain host
// C++: the headers make no HIP runtime call.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../charon_amd/csrc/bls_hex.h"
#include "../../charon_amd/csrc/tbls_plan.h"
#include "../../charon_amd/csrc/tbls_work.h"

using namespace tbg;

namespace {

// cfg16: PlanConfig's fields in their order
PlanConfig config(const double* v) {
  PlanConfig c;
  c.rlc_group = (uint32_t)v[0];
  c.rlc_chunk = (uint32_t)v[1];
  c.chunk_auto = v[2] != 0;
  c.rlc_auto = v[3] != 0;
  c.rlc_batch = (uint32_t)v[4];
  c.invalid_ema = v[5];
  c.nonsub_ema = v[6];
  c.gident = (uint32_t)v[7];
  c.fb_window = (uint32_t)v[8];
  c.sgb_mode = (uint32_t)v[9];
  c.l0_duty_partials = (uint32_t)v[10];
  c.l0_tail_partials = (uint32_t)v[11];
  c.l0_msg_share = (uint32_t)v[12];
  c.sgb_tri_partials = (uint32_t)v[13];
  c.sgb_tri_m = (uint32_t)v[14];
  c.n_simd = (uint32_t)v[15];
  return c;
}

// batches: [n][3] duties, partials, messages of each caller batch
bool plan_of(const PlanConfig& c, uint32_t op, uint64_t msg_bytes, const uint32_t* batches, uint32_t n_batches,
             const uint32_t* set_first, uint32_t n_sets, LaunchLayout& L) {
  LaunchDims d;
  d.op = op;
  d.msg_bytes = (size_t)msg_bytes;
  d.sets = set_first != nullptr;
  d.n_sets = n_sets;
  std::vector<uint32_t> dm(2 * (size_t)n_batches);
  for (uint32_t k = 0; k < n_batches; ++k) {
    d.n_duties += batches[3 * k];
    d.n_partials += batches[3 * k + 1];
    d.n_msgs += batches[3 * k + 2];
    dm[2 * k] = batches[3 * k];
    dm[2 * k + 1] = batches[3 * k + 2];
  }
  const LaunchPlan p = plan_launch(c, d, set_first, dm.data(), n_batches);
  if (!p.ok) return false;
  L = layout(p, d);
  return true;
}

// A slot sized for nd0 duties of three partials, one message each, at a configured (G0, C0), level 0 on.
LaunchLayout slot_of(uint32_t nd0, uint32_t G0, uint32_t C0) {
  PlanConfig c;
  c.rlc_group = G0;
  c.rlc_chunk = C0;
  c.chunk_auto = false;
  c.rlc_batch = TBG_RLC_L0_ON;
  const uint32_t b[3] = {nd0, 3 * nd0, nd0};
  LaunchLayout L;
  plan_of(c, TBG_OP_VERIFY_AGGREGATE, 32ull * nd0, b, 1, nullptr, 0, L);
  return L;
}

}  // namespace

extern "C" {

uint32_t pl_max_sections() { return kMaxSections; }

// plan_out[20]: n_duties, rlc_group_cfg, G, C, l0, vp, fb_w, fb_full, sgb, sgb_m, sgb_m_small, sgb_split, fused, msm,
// l0m_in, l0m, l0m_chunks, gident, aggver, l0_msg_share; totals[4]: in_bytes, work_bytes, w_out, out_bytes;
// secs[n][3]: arena, offset, bytes; names[n].  Returns the section count, -1 for a refused plan.
int pl_layout(const double* cfg16, uint32_t op, uint64_t msg_bytes, const uint32_t* batches, uint32_t n_batches,
              const uint32_t* set_first, uint32_t n_sets, uint64_t* plan_out, uint64_t* totals, uint64_t* secs,
              const char** names) {
  LaunchLayout L;
  if (!plan_of(config(cfg16), op, msg_bytes, batches, n_batches, set_first, n_sets, L)) return -1;
  const LaunchPlan& p = L.plan;
  const uint64_t po[20] = {L.dims.n_duties, p.rlc_group_cfg, p.G, p.C, p.l0, p.vp, p.fb_w, p.fb_full, p.sgb, p.sgb_m,
                           p.sgb_m_small, p.sgb_split, p.fused, p.msm, p.l0m_in, p.l0m, p.l0m_chunks, p.gident, p.aggver,
                           p.l0_msg_share};
  memcpy(plan_out, po, sizeof(po));
  totals[0] = L.in_bytes;
  totals[1] = L.work_bytes;
  totals[2] = L.w_out;
  totals[3] = L.out_bytes;
  for (uint32_t i = 0; i < L.n; ++i) {
    secs[3 * i] = L.sec[i].arena;
    secs[3 * i + 1] = L.sec[i].off;
    secs[3 * i + 2] = L.sec[i].bytes;
    names[i] = L.sec[i].name;
  }
  return (int)L.n;
}

// bind over fake bases (0: that arena is not bound; out_base: the output image apart from the work
// arena, 0 for its tail): ptrs[n] the members' values in table order, alias[5] sig_lines and its four
// aliases, scalars[12]: op, n_duties, n_partials, n_msgs, rlc_group, rlc_chunk, rlc_batch, fb_window, sgb, sgb_m,
// sets, n_sets
int pl_bind(const double* cfg16, uint32_t op, uint64_t msg_bytes, const uint32_t* batches, uint32_t n_batches,
            const uint32_t* set_first, uint32_t n_sets, uint64_t in_base, uint64_t work_base, uint64_t out_base, uint64_t* ptrs,
            uint64_t* alias, uint32_t* scalars) {
  LaunchLayout L;
  if (!plan_of(config(cfg16), op, msg_bytes, batches, n_batches, set_first, n_sets, L)) return -1;
  DevBatch B;
  memset(&B, 0, sizeof(B));
  bind(B, L, (uint8_t*)(uintptr_t)in_base, (uint8_t*)(uintptr_t)work_base, (uint8_t*)(uintptr_t)out_base);
  uint32_t i = 0;
  for_each_section(L.plan, L.dims,
                   [&](const char*, auto member, ArenaId, size_t, bool) { ptrs[i++] = (uint64_t)(uintptr_t)(B.*member); });
  const void* al[5] = {B.sig_lines, B.chunk_lines, B.cid_lines, B.gid_lines, B.id_lines};
  for (int k = 0; k < 5; ++k) alias[k] = (uint64_t)(uintptr_t)al[k];
  const uint32_t sc[12] = {B.op, B.n_duties, B.n_partials, B.n_msgs, B.rlc_group, B.rlc_chunk, B.rlc_batch, B.fb_window,
                           B.sgb, B.sgb_m, B.sets, B.n_sets};
  memcpy(scalars, sc, sizeof(sc));
  return (int)L.n;
}

// The fit rule derived from the table: nd duties at (G, C) in a slot laid out for nd0 duties at (G0, C0).
int pl_shape_fits(uint32_t nd0, uint32_t G0, uint32_t C0, uint32_t nd, uint32_t G, uint32_t C) {
  return shape_fits(slot_of(nd0, G0, C0), nd, 3 * nd, nd, G, C) ? 1 : 0;
}

// l0_shape; with n_prefix > 0 under the filter "every prefix_nd[k] fits a slot of (nd0, G0, C0)"
void pl_l0_shape(uint64_t nd, uint32_t n_simd, int g_free, uint32_t G, uint32_t nd0, uint32_t G0, uint32_t C0,
                 const uint32_t* prefix_nd, uint32_t n_prefix, uint32_t* out_gc) {
  uint32_t C = 0;
  if (n_prefix) {
    const LaunchLayout slot = slot_of(nd0, G0, C0);
    l0_shape(nd, n_simd, g_free != 0, G, C, [&](uint32_t g, uint32_t ch) {
      for (uint32_t k = 0; k < n_prefix; ++k)
        if (!shape_fits(slot, prefix_nd[k], 3 * prefix_nd[k], prefix_nd[k], g, ch)) return false;
      return true;
    });
  } else {
    l0_shape(nd, n_simd, g_free != 0, G, C, l0_fits_any);
  }
  out_gc[0] = G;
  out_gc[1] = C;
}

int pl_sgb_plan(double rho, uint32_t* m) { return sgb_plan(rho, *m) ? 1 : 0; }

uint32_t pl_fb_small() { return FB_SMALL; }
uint32_t pl_lines_words() { return LINES_WORDS; }

// The passes fb_passes makes over a fallback list of `count` entries (max_entries: what the launcher sizes the
// passes by), each with the grid its launcher starts and every walker of that grid run through fb_pass_loop:
//   kind 0, the hexad kernels (k_verify_list, k_rlc_ident_check): grid_for(hex_threads(n)) blocks of kBlock, a
//           walker per hex_slot of its threads, stride hex_slots_of(threads);
//   kind 1, the pair kernels (k_lines_sig_list, k_lines_fold): grid_for(2 n), a walker per t >> 1, stride
//           pair_slots_of(threads).
// passes[p][6]: base, n as the body received it, the stride, the walkers (distinct slots of the grid's threads), the
// offset of the pass in trips, the largest fb_slot a walker formed; trips[]: the body's runs per walker, in slot
// order; hits[max_entries]: visits per list position (the caller zeroes it); hit_pass[max_entries]: the pass of the
// last one.  Returns the number of passes; -1: passes or trips would not fit; -2: the threads' slots are not 0, 1, ...
// with 6 (2) threads each; -3: a visit outside [0, count).
int pl_fb_cover(uint32_t fb_w, uint32_t fb_full, uint32_t count, uint32_t max_entries, int may_shrink, int kind,
                uint64_t* passes, uint32_t max_passes, uint32_t* trips, uint64_t max_trips, uint32_t* hits,
                uint32_t* hit_pass) {
  DevBatch B;
  memset(&B, 0, sizeof(B));
  B.fb_window = fb_w;
  B.fb_full = fb_full;
  int n_passes = 0, err = 0;
  uint64_t used = 0;
  std::vector<uint32_t> seen;
  fb_passes(B, max_entries, [&](const DevBatch& P, uint32_t n) {
    if (err) return;
    const uint32_t blocks = (kind == 0 ? grid_for(hex_threads(n)) : grid_for(2 * n)).x, threads = blocks * (uint32_t)kBlock;
    // (as hex_grid_slots forms it on the device: per block)
    const uint32_t stride = kind == 0 ? blocks * hex_slots_of((uint32_t)kBlock) : pair_slots_of(threads);
    const uint32_t lanes = kind == 0 ? 6u : 2u;
    if ((uint32_t)n_passes >= max_passes || used + threads > max_trips) {
      err = -1;
      return;
    }
    uint64_t max_slot = 0;
    uint32_t walkers = 0;
    seen.assign(threads, 0u);
    for (uint32_t t = 0; t < threads; ++t) {
      const uint32_t s = kind == 0 ? hex_slot(t) : t >> 1;
      if (s == 0xFFFFFFFFu) continue;  // (lane 15 of a row: no hexad)
      if (s >= threads) {
        err = -2;
        return;
      }
      if (seen[s]++) continue;  // one walker per slot: its lanes walk together
      ++walkers;
      uint32_t runs = 0;
      fb_pass_loop(P, s, stride, count, [&](uint32_t k) {
        ++runs;
        if (k >= count || k >= max_entries) {
          err = -3;
          return;
        }
        ++hits[k];
        hit_pass[k] = (uint32_t)n_passes;
        max_slot = std::max<uint64_t>(max_slot, fb_slot(P, k));
      });
      trips[used + s] = runs;
    }
    for (uint32_t s = 0; s < threads; ++s)
      if (seen[s] != (s < walkers ? lanes : 0u)) err = -2;
    const uint64_t row[6] = {P.fb_base, n, stride, walkers, used, max_slot};
    memcpy(passes + 6 * (size_t)n_passes, row, sizeof(row));
    used += walkers;
    ++n_passes;
  }, may_shrink != 0);
  return err ? err : n_passes;
}

uint32_t pl_max_work_sections() { return kMaxWorkSections; }

// The workspace of one-shot call `call` (0 tbg_sk_to_pk, 1 tbg_sk_to_pk_ct, 2 tbg_sign, 3 tbg_sign_ct, 4
// tbg_sum_pubkeys, 5 tbg_sum_sigs, 6 tbg_fast_aggregate_verify) as the engine makes it: work_size, then
// work_bind over `base` (0: the sizing walk alone).  dims[4]: the signers' n, n_msgs, msg_bytes, tab_words; the
// sums' n_sets, n_chunks, n_items / n_keys, msg_bytes.  secs[n][2]: offset, bytes of the sizing walk; ptrs[n]:
// the description's pointers after the binding walk, in section order; *total: the allocation's bytes.
// Returns the section count, -1 for an unknown call.
int pl_work(uint32_t call, const uint64_t* dims, uint64_t base, uint64_t* total, uint64_t* secs, uint64_t* ptrs,
            const char** names) {
  auto run = [&](auto& w) {
    const WorkWalk sized = work_size(w);
    *total = sized.bytes();
    for (uint32_t i = 0; i < sized.n; ++i) {
      secs[2 * i] = sized.sec[i].off;
      secs[2 * i + 1] = sized.sec[i].bytes;
      names[i] = sized.sec[i].name;
    }
    if (base) work_bind(w, sized, (uint8_t*)(uintptr_t)base);
    uint32_t i = 0;
    auto read = [&](const char*, auto*& p, size_t, size_t = 0) { ptrs[i++] = (uint64_t)(uintptr_t)p; };
    w.sections(read);
    return (int)sized.n;
  };
  auto sum_dims = [&](SumWork& w, size_t part_elem) {
    w.n_sets = dims[0];
    w.n_chunks = dims[1];
    w.part_elem = part_elem;
  };
  switch (call) {
    case 0: {
      SkToPkWork w;
      w.n = dims[0];
      return run(w);
    }
    case 1: {
      SkToPkCtWork w;
      w.n = dims[0];
      w.tab_words = dims[3];
      return run(w);
    }
    case 2: {
      SignWork w;
      w.n = dims[0];
      w.n_msgs = dims[1];
      w.msg_bytes = dims[2];
      return run(w);
    }
    case 3: {
      SignCtWork w;
      w.n = dims[0];
      w.n_msgs = dims[1];
      w.msg_bytes = dims[2];
      w.tab_words = dims[3];
      return run(w);
    }
    case 4: {
      SumPubkeysWork w;
      sum_dims(w, sizeof(G1J));
      w.n_items = dims[2];
      return run(w);
    }
    case 5: {
      SumSigsWork w;
      sum_dims(w, sizeof(G2J));
      w.n_items = dims[2];
      return run(w);
    }
    case 6: {
      FastAggVerifyWork w;
      sum_dims(w, sizeof(G1J));
      w.n_keys = dims[2];
      w.msg_bytes = dims[3];
      return run(w);
    }
  }
  return -1;
}

}  // extern "C"
