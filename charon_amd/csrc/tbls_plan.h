// What a launch decides before it touches the device, as plain host
// arithmetic: the plan (group size, launch shape, level 0, the subgroup test's
// schedule, ...), and ONE table of the arena sections from which the sizes,
// the DevBatch pointers and a replay's fit rule are all derived.  No HIP
// runtime call in here: tests/plan builds it with a host compiler and
// tests/test_plan_host.py checks it on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <type_traits>
#include "tbls_launch.h"
#include "bls_l0msg.h"

namespace tbg {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The bump allocator of every arena in the engine: sections start 16-byte aligned.
struct Arena {
  size_t o = 0;
  size_t take(size_t bytes) {
    const size_t at = o;
    o = align_up(o + bytes, 16);
    return at;
  }
};

// The fields of a context that planning reads (tbg_ctx is one).
struct PlanConfig {
  // Defaults measured on MI355X (tools/sweep_rlc.sh, config 2): 16 duties per
  // level-1 group, 4 per Miller quad beat 8 / 2 by ~8 %: half the final
  // exponentiations and Fp12 squarings per duty.
  uint32_t rlc_group = 16;  // 0 = per-partial checks (TBG_VERIFY_EACH)
  uint32_t rlc_chunk = 4;
  bool chunk_auto = true;    // rlc_chunk not configured: level-0 launches of many duties take 8
  bool rlc_auto = false;     // rlc_group follows the observed invalid share (tbg_config.rlc_group = 0)
  uint32_t rlc_batch = TBG_RLC_L0_AUTO;  // level 0 (the whole device batch as one check)
  double invalid_ema = 0.0;  // exponential average of the invalid share of collected verified partials
  double nonsub_ema = 0.0;   // exponential average of the non-subgroup share of collected partials
  uint32_t gident = TBG_GIDENT_OFF;  // level 1g routing (tbg_config.gident)
  uint32_t fb_window = TBG_FB_WINDOW;  // fallback line buffer positions per pass (tbg_config.fb_window)
  uint32_t sgb_mode = TBG_SGB_AUTO;    // batched subgroup test (tbg_config.subgroup_batch)
  uint32_t l0_duty_partials = TBG_L0_DUTY_PARTIALS;  // fused level 0: P_d per duty from this many partials (tbg_config.l0_duty_partials)
  uint32_t l0_tail_partials = TBG_L0_TAIL_PARTIALS;  // fused level 0: S inside the key-side grid from this many partials (tbg_config.l0_tail_partials)
  uint32_t l0_msg_share = TBG_L0_MSG_SHARE;  // fused level 0: per message from this many duties per message (tbg_config.l0_msg_share)
  uint32_t sgb_tri_partials = TBG_SGB_TRI_PARTIALS;  // batched subgroup test: triple schedule from this many partials (tbg_config.sgb_tri_partials)
  uint32_t sgb_tri_m = SGB_TRI_M;                    // its group size (tbg_config.sgb_tri_m)
  uint32_t n_simd = 1024;  // SIMDs of the device (CUs x 4): the level-0 shape rule's unit (l0_shape)
};

// The counts of one device batch.  plan_launch pads n_duties for a set launch.
struct LaunchDims {
  uint32_t op = 0, n_duties = 0, n_partials = 0, n_msgs = 0;
  size_t msg_bytes = 0;
  bool sets = false;
  uint32_t n_sets = 0;
};

// Everything a submit decides before it sizes its arenas.
struct LaunchPlan {
  bool ok = true;          // false: a set launch's padded duties pass the engine's limit
  uint32_t rlc_group_cfg;  // the context's rlc_group from here on (the adaptive size under rlc_auto)
  uint32_t G, C;           // duties per level-1 group (0: per-partial checks) and per Miller chunk
  bool aggver;             // TBG_OP_AGGREGATE_VERIFY: the checks run on the batch's view (aggver_view), one
                           // candidate per duty, so every array of the check levels is sized by duties
  uint32_t vp;             // candidates of the check levels
  bool l0;                 // level 0 runs
  uint32_t fb_w, fb_full;  // DevBatch::fb_window, ::fb_full
  bool sgb;                // the batched subgroup test runs
  uint32_t sgb_m, sgb_m_small, sgb_split;  // its group size; a prefix's below sgb_tri_partials; slices per bucket
  bool fused, msm;         // level 0's S from the subgroup test's sums / from the bucket MSM
  bool l0m_in, l0m;        // level 0 by message: the plan is packed with the inputs / the work arrays exist
  size_t l0m_chunks;       // the chunk plan's bound
  uint32_t gident;         // DevBatch::gident
  uint32_t l0_duty_partials, l0_tail_partials, l0_msg_share;  // DevBatch's (l0_msg_share: never, without a plan)
};

// Level-0 launch shape.  The level-0 Miller kernel's
// waves are long -- one hexad = the whole 68-step loop over C duties -- and
// issue-bound at ONE wave per SIMD: a lone wave runs its loop in 3.6 ms at
// C = 4, two sharing a SIMD take 6.8 ms each (profiles/r05/waves), so the
// kernel's time is ~ceil(waves / SIMDs) hexad lengths, and a launch whose
// waves spill just past a multiple of the SIMD count pays a whole hexad
// length for the remainder: config 4's 125k-duty shard at (G, C) = (16, 4)
// is 3,126 waves on 1,024 SIMDs.  A hexad of C duties costs 62 squarings +
// 68 C line products, w(C) = 0.95 M + 1.39 M C u32 mul-adds
// (profiles/work_model.json, l0_chunk_*), so fewer, longer hexads win where
// they save a unit: (16, 8) halves the squarings, (14, 7) runs 125k duties
// in 2 units instead of 4.  The rule picks the cheapest of (16, 4), (16, 8),
// (14, 7) by ceil(waves / SIMDs) x w(C) -- 100k duties keep (16, 4), 125k
// take (14, 7), 160k (16, 8), as the A/B runs of profiles/r05/chunk8_ab,
// shape_ab and sqrt_x2_ab measured best.  A configured group size G keeps G
// (C = 4 or 8 only).  tbg_replay_plan applies it to the duties of the
// launches it runs together (their Miller kernels share the SIMDs).
inline double l0_shape_cost(uint64_t nd, uint32_t n_simd, uint32_t g, uint32_t ch) {
  const uint64_t hexads = (uint64_t)((nd + g - 1) / g) * ((g + ch - 1) / ch);
  const uint64_t waves = (hexads + 9) / 10;
  return (0.948 + 1.395 * ch) * (double)((waves + n_simd - 1) / n_simd);
}
// Round 6: with the group size free, every chunk C of
// 5 .. 10 duties is a candidate too, as (G, C) = (C, C) -- one chunk per
// group -- so the hexads can fill whole wave-slot rounds: the 20-step plan's
// 200k duties take (10, 10) (2,000 waves: 2 rounds) instead of (14, 7) (2,858
// waves: 3 rounds; +2.6 % at the driver shape, profiles/r06/shape), config
// 3's 100k (10, 10) instead of (16, 4) (Miller 8.0 vs 9.4 ms).  Chunks of 13
// and 16 duties were measured far off the model (a round of ~1,000 lone
// waves: (16, 16) 20.4 ms vs (16, 8) 12.2 ms at 160k duties, (13, 13) 16.8
// vs (14, 7) 11.0 ms at 125k: the C line loads of a step are not hidden by a
// second wave), so C stops at L0_SHAPE_MAX_C.
// `fits` (a replay's arenas, shape_fits below) drops the candidates a launch cannot hold.
inline bool l0_fits_any(uint32_t, uint32_t) { return true; }
inline void l0_shape(uint64_t nd, uint32_t n_simd, bool g_free, uint32_t& G, uint32_t& C,
                     const std::function<bool(uint32_t, uint32_t)>& fits) {
  C = 4;
  if (G < 8) return;
  constexpr uint32_t L0_SHAPE_MAX_C = 10;
  uint32_t cand[3 + L0_SHAPE_MAX_C][2] = {{g_free ? 16u : G, 4}, {g_free ? 16u : G, 8}, {14, 7}};
  uint32_t n_cand = g_free ? 3u : 2u;
  for (uint32_t c = 5; g_free && c <= L0_SHAPE_MAX_C; ++c) {
    cand[n_cand][0] = c;
    cand[n_cand][1] = c;
    ++n_cand;
  }
  double best = 1e300;
  const uint32_t G0 = G;
  for (uint32_t k = 0; k < n_cand; ++k) {
    if (!fits(cand[k][0], cand[k][1])) continue;
    const double cost = l0_shape_cost(nd, n_simd, cand[k][0], cand[k][1]);
    if (cost < best - 1e-9) {
      best = cost;
      G = cand[k][0];
      C = cand[k][1];
    }
  }
  if (best == 1e300) G = G0;  // (nothing fits: the caller keeps its shapes)
}

// Batched subgroup test plan from the non-subgroup share `rho` of the
// collected partials.  Per signature, in units of one
// per-signature test (psi(s) == [x] s: 63 doublings + 5 additions): the 16.6
// bucket additions with the sort and running sums 0.55 (measured: k_sgb_*
// 0.47-0.57 of k_subgroup_sigs' time per signature, profiles/r06/sgb), the
// group's 18 tests 1.1 x 18 / m (each on a lone lane pair), and the failed
// groups' members tested alone 1 - (1 - rho)^m.  The group size m is the
// cheapest power of two in [SGB_M_MIN, SGB_M]; the test runs while that
// costs under 0.95 of testing every signature alone -- up to rho ~ 2.5e-3
// (TBG_SGB_AUTO_MAX).  Clean traffic keeps m = 1,024; config 5's 1.25e-3
// takes m = 128 (at 1,024, 72 % of its groups would fail).  The 0.55 is the
// classic schedule's; the paired schedule of groups >= SGB_PAIR_M
// (tbls_launch.h) is cheaper, which only widens the test's margin, and the
// sizes this plan picks are left as they were.
inline bool sgb_plan(double rho, uint32_t& m) {
  double best = 1e9;
  m = SGB_M;
  for (uint32_t k = SGB_M; k >= SGB_M_MIN; k >>= 1) {
    const double cost = 0.55 + 1.1 * (double)SGB_K / k + (1.0 - std::pow(1.0 - std::min(rho, 1.0), (double)k));
    if (cost < best - 1e-12) {
      best = cost;
      m = k;
    }
  }
  return best < 0.95;
}

// The triple schedule (tbls_launch.h sgb_triple) in the same units.  Whether
// its arithmetic pays at a launch's size is the threshold's business
// (tbg_config.sgb_tri_partials, set from an A/B like l0_duty_partials): the
// count model (tools/sgb_pair_model.py) has bucket
// additions, ranked slots and reductions at 7.30 per member in groups of
// 16,384 against the paired 11.66 at 1,024, so 0.55 x (1 - 7.30 / 11.66) =
// 0.21 less per signature.  What the plan weighs is the term that grows with
// the group: a failed group's members are tested alone, 1 - (1 - rho)^m of
// them, against the same term at the size `m_small` that sgb_plan picked.
// The triple schedule runs while that difference stays under the modelled
// saving -- rho up to ~1.4e-5 at 16,384, the clean regime; any measurable
// non-subgroup share falls back to the paired sizes exactly as before.
inline bool sgb_plan_triple(double rho, uint32_t m_small, uint32_t m_tri) {
  const double r = std::min(rho, 1.0);
  const double extra = std::pow(1.0 - r, (double)m_small) - std::pow(1.0 - r, (double)m_tri) +
                       1.1 * (double)SGB_K * (1.0 / m_tri - 1.0 / m_small);
  return extra < 0.55 * (1.0 - 7.30 / 11.66);
}
// The launch's group size: sgb_plan's, or the triple schedule's in a clean
// launch of at least sgb_tri_partials partials.  (A replayed prefix asks
// again with its own partial count.)
inline uint32_t sgb_group_size(const PlanConfig& c, uint32_t np, uint32_t m_small, bool clean_tri) {
  return clean_tri && np >= c.sgb_tri_partials ? c.sgb_tri_m : m_small;
}

// Device duties of a set launch at group size G: every non-empty set starts on
// a multiple of G (the duties between are empty padding), so no level-1 group
// holds duties of two sets.
inline uint64_t sets_padded(const uint32_t* set_first, uint32_t n_sets, uint32_t G) {
  uint64_t e = 0;
  for (uint32_t k = 0; k < n_sets; ++k) {
    const uint32_t n = set_first[k + 1] - set_first[k];
    if (n) e = (e + G - 1) / G * G + n;
  }
  return e;
}

// The plan of a launch of n_batches caller batches, batch k bringing
// batch_dm[2 k] duties and batch_dm[2 k + 1] messages; d holds their totals (a set launch: the
// one batch's counts, set_first its sets) and leaves with the device duties.
inline LaunchPlan plan_launch(const PlanConfig& c, LaunchDims& d, const uint32_t* set_first,
                              const uint32_t* batch_dm, uint32_t n_batches) {
  LaunchPlan p{};
  const bool verify = d.op != TBG_OP_AGGREGATE;
  const uint32_t np = d.n_partials, nm = d.n_msgs;
  p.aggver = d.op == TBG_OP_AGGREGATE_VERIFY;
  p.rlc_group_cfg = !c.rlc_auto                        ? c.rlc_group
                    : c.invalid_ema < TBG_RLC_AUTO_TO8 ? 16
                    : c.invalid_ema < TBG_RLC_AUTO_TO4 ? 8
                                                       : 4;
  uint32_t G = verify ? p.rlc_group_cfg : 0;
  if (d.sets) {
    // An unconfigured group size shrinks (to 8, then 4) while the sets'
    // padding would pass 1/8 of the duties: a launch of small sets keeps its
    // groups full instead of checking mostly padding.
    const uint64_t nd64 = d.n_duties;
    while (c.rlc_auto && G > 4 && sets_padded(set_first, d.n_sets, G) > nd64 + nd64 / 8) G /= 2;
    const uint64_t padded = sets_padded(set_first, d.n_sets, G ? G : 1);  // (>= the caller's duties: validate() wants one at least)
    if (padded > 0x7FFFFFFFull) {
      p.ok = false;
      return p;
    }
    d.n_duties = (uint32_t)padded;
  }
  const uint32_t nd = d.n_duties;
  const uint32_t vp = p.vp = p.aggver ? nd : np;
  // Level 0 by message (bls_l0msg.h): the duties sorted by message and the
  // chunk plan, packed with the inputs.  Reserved whenever a fused level 0
  // may run with the knob on, whatever the launch's own duties per message:
  // a replayed prefix decides from its own (l0_by_msg).  The work arena's
  // sections exist once `fused` is known; the input side is sized by the
  // same conditions except the subgroup test's, which only shrink it.
  // Nothing is reserved or sorted when no prefix of the caller batches
  // reaches the share (one message per duty: the headline workload).
  if (verify && !p.aggver && p.rlc_group_cfg != 0 && c.rlc_batch != TBG_RLC_L0_OFF && c.sgb_mode != TBG_SGB_OFF &&
      c.l0_msg_share != TBG_L0_MSG_NEVER && np >= SGB_MIN_PARTIALS) {
    uint64_t cd = 0, cm = 0;
    for (uint32_t k = 0; k < n_batches; ++k) {
      cd = d.sets ? nd : cd + batch_dm[2 * k];
      cm += batch_dm[2 * k + 1];
      p.l0m_in = p.l0m_in || cm * c.l0_msg_share <= cd;
    }
  }
  p.l0m_chunks = p.l0m_in ? (size_t)l0m_chunk_bound(nm, nd) : 0;
  // The fallback levels' lines share one buffer of fb_w list positions,
  // consumed in passes (DevBatch::fb_window): a slot no longer holds 22.8 KB
  // per partial for lists that a clean batch leaves empty.
  p.fb_w = verify ? std::max<uint32_t>(1u, std::min<uint32_t>(c.fb_window, vp)) : 0u;
  // Level 0 while the collected batches are clean (or as configured): one
  // failed level-0 check costs its own work on top of the group levels.
  p.l0 = G != 0 && vp < (1u << 28) &&
         (c.rlc_batch == TBG_RLC_L0_ON || (c.rlc_batch == TBG_RLC_L0_AUTO && c.invalid_ema < TBG_RLC_AUTO_L0));
  uint32_t C = c.rlc_chunk;
  // (a set launch keeps its G: the sets are padded to it)
  if (p.l0 && c.chunk_auto) l0_shape(nd, c.n_simd, !d.sets && c.rlc_auto && G == 16, G, C, l0_fits_any);
  if (C > G) C = G ? G : 1;
  p.G = G;
  p.C = C;
  // Batched subgroup test while the collected batches carry (almost) no
  // non-subgroup signature: groups of 1,024 partials, a failed group's members
  // tested alone (k_sgb.hip); small batches test every signature alone.
  uint32_t sgb_m = SGB_M;
  p.sgb = np >= SGB_MIN_PARTIALS && c.sgb_mode != TBG_SGB_OFF && (sgb_plan(c.nonsub_ema, sgb_m) || c.sgb_mode == TBG_SGB_ON);
  // A clean launch of at least sgb_tri_partials partials takes the triple
  // schedule's large groups.  A replayed prefix below the threshold goes back
  // to sgb_m_small, so such a launch's sections hold either layout.
  p.sgb_m_small = sgb_m;
  const bool sgb_tri_ok = p.sgb && sgb_plan_triple(c.nonsub_ema, p.sgb_m_small, c.sgb_tri_m);
  p.sgb_m = sgb_group_size(c, np, p.sgb_m_small, sgb_tri_ok);
  p.sgb_split = sgb_triple(p.sgb_m) ? 1u : sgb_split_for(p.sgb_m);
  // Level 0's signature side: with the batched test on, S comes from the
  // test's sums (l0_fused, tbls_launch.h; a replayed prefix of the launch
  // keeps both flags, so it takes the same path) and the bucket MSM's
  // arrays are not needed; otherwise the bucket MSM of k_msm.hip.
  // (TBG_OP_AGGREGATE_VERIFY: the subgroup test is the partials', the level 0 the view's,
  // which has no digits to take S from -- always the bucket MSM, over the duties)
  p.fused = p.l0 && p.sgb && !p.aggver;
  p.msm = p.l0 && !p.fused;
  p.l0m = p.fused && p.l0m_in;
  p.l0_duty_partials = c.l0_duty_partials;
  p.l0_tail_partials = c.l0_tail_partials;
  p.l0_msg_share = p.l0m ? c.l0_msg_share : TBG_L0_MSG_NEVER;  // (no plan: never by message)
  // Level 1g is opt-in (tbg_config.gident).  Measured
  // (profiles/r03/gident/): +7 % at 1 % invalid in 20-step runs, whose three
  // launches reach their latency-bound fallback levels together, but -3 % at
  // 48 steps and -11 % on config 5, where launches overlap and the
  // narrowing's shorter lists matter more than its extra levels.
  // (level 1g's lines kernel runs a lane per duty of a group; a set launch's failed group is not narrowed)
  p.gident = G > 1 && G <= 64 && !d.sets ? c.gident : 0u;
  // full-grid passes of the duty / partial lists: those the collected
  // batches' invalid share makes likely (10x margin), every pass for the
  // per-partial schedule
  const double share = std::min(1.0, 10.0 * c.invalid_ema);
  const uint64_t expect = (uint64_t)((double)vp * share);
  p.fb_full = (G == 0 || p.fb_w == 0) ? 0xFFFFFFFFu
                                      : (uint32_t)std::min<uint64_t>(0xFFFFFFFFull, (expect / p.fb_w + 1) * (uint64_t)p.fb_w);
  return p;
}

// ---- the section table -------------------------------------------------------
// IN: the input arena (one H2D copy of the pinned image).  WORK: the work
// arena.  OUT: the outputs, the work arena's tail, contiguous so that one D2H
// copy brings them back.
enum ArenaId : uint8_t { ARENA_IN = 0, ARENA_WORK = 1, ARENA_OUT = 2 };

// Every section of a launch's arenas, each named once, in arena order:
//   visit(name, &DevBatch::member, arena, bytes, null_when_empty)
// bytes is the unaligned size, 0 when the section's condition is off.  An
// empty section's member points at where it would start (never dereferenced);
// the members that exist only in a set or TBG_OP_AGGREGATE_VERIFY launch stay
// null in every other one (k_aggregate.hip tests agg_aff).
template <class V>
void for_each_section(const LaunchPlan& p, const LaunchDims& d, V&& visit) {
  const size_t nd = d.n_duties, np = d.n_partials, nm = d.n_msgs, vp = p.vp;
  const size_t G = p.G, C = p.C;
  const size_t ng = G ? (nd + G - 1) / G : 0, nch = G ? (G + C - 1) / C : 0;
  const bool verify = d.op != TBG_OP_AGGREGATE, agg = d.op != TBG_OP_VERIFY;
  const bool lv = G > 1;                        // the levels between the groups and the partials
  const size_t FE = 4ull * 3 * 4 * NL;          // one Fp12 value in the quad layout
  const size_t LINES = 4ull * LINES_WORDS;      // one point's Miller lines
  const bool tri = sgb_triple(p.sgb_m);
  const size_t n_sg = p.sgb ? sgb_groups(d.n_partials, p.sgb_m) : 0;
  const size_t n_sg_small = p.sgb ? sgb_groups(d.n_partials, p.sgb_m_small) : 0;  // (the most groups a prefix can have)
  // a section of per_group(m) units per group, in either layout of a triple launch (plan_launch)
  auto sgsec = [&](auto&& per_group) {
    return std::max<size_t>(per_group(p.sgb_m) * n_sg, tri ? per_group(p.sgb_m_small) * n_sg_small : 0);
  };
#define TBG_SEC(member, arena, bytes) visit(#member, &DevBatch::member, arena, (size_t)(bytes), false)
#define TBG_SEC_OPT(member, arena, bytes) visit(#member, &DevBatch::member, arena, (size_t)(bytes), true)
  TBG_SEC(msgs, ARENA_IN, d.msg_bytes);
  TBG_SEC(msg_off, ARENA_IN, 4 * (nm + 1));
  TBG_SEC(duty_msg, ARENA_IN, 4 * nd);
  TBG_SEC(duty_first, ARENA_IN, 4 * (nd + 1));
  TBG_SEC(duty_threshold, ARENA_IN, 4 * nd);
  TBG_SEC(partial_duty, ARENA_IN, 4 * np);
  TBG_SEC(sigs, ARENA_IN, 96 * np);
  TBG_SEC(identifiers, ARENA_IN, np);
  TBG_SEC(pubkey_ids, ARENA_IN, 4 * vp);
  TBG_SEC_OPT(duty_set, ARENA_IN, d.sets ? 4 * nd : 0);
  TBG_SEC_OPT(av_iota, ARENA_IN, p.aggver ? 4 * (nd + 1) : 0);
  // level 0 by message: the duties by message and the chunk plan
  TBG_SEC(msg_first, ARENA_IN, p.l0m_in ? 4 * (nm + 1) : 0);
  TBG_SEC(msg_duty, ARENA_IN, p.l0m_in ? 4 * nd : 0);
  TBG_SEC(l0m_chunk_first, ARENA_IN, p.l0m_in ? 4 * (nm + 1) : 0);
  TBG_SEC(l0m_chunk_msg, ARENA_IN, p.l0m_in ? 4 * p.l0m_chunks : 0);

  TBG_SEC(sig_aff, ARENA_WORK, sizeof(G2A) * np);
  TBG_SEC(h_aff, ARENA_WORK, sizeof(G2A) * nm);
  TBG_SEC(h_status, ARENA_WORK, 4 * nm);
  TBG_SEC(h_jac, ARENA_WORK, 3 * sizeof(G2J) * nm);  // H(m) + the cofactor clearing's two temporaries
  TBG_SEC(lam, ARENA_WORK, 32 * np);
  TBG_SEC(sig_lines, ARENA_WORK, LINES * p.fb_w);  // the fallback levels' one line buffer (plan_launch fb_w)
  TBG_SEC(h_lines, ARENA_WORK, LINES * nm);
  TBG_SEC(part_p, ARENA_WORK, G ? sizeof(G1J) * vp : 0);
  TBG_SEC(part_s, ARENA_WORK, G ? sizeof(G2J) * vp : 0);
  TBG_SEC(chunk_f, ARENA_WORK, G ? FE * ng * (nch + 1) : 0);
  TBG_SEC(chunk_list, ARENA_WORK, lv ? 4 * ng * nch : 0);
  TBG_SEC(dv_p, ARENA_WORK, G ? sizeof(G1A) * nd : 0);
  TBG_SEC(dv_s, ARENA_WORK, G ? sizeof(G2J) * nd : 0);
  TBG_SEC(dv_state, ARENA_WORK, G ? 4 * nd : 0);
  TBG_SEC(grp_state, ARENA_WORK, 4 * ng);
  TBG_SEC(grp_lines, ARENA_WORK, LINES * ng);
  TBG_SEC(counters, ARENA_WORK, 4 * CNT_WORDS);
  TBG_SEC(part_list, ARENA_WORK, verify ? 4 * vp : 0);
  TBG_SEC(id_fe, ARENA_WORK, lv ? FE * nd : 0);
  TBG_SEC(pend_pts, ARENA_WORK, G ? sizeof(G2A) * std::max(std::max(ng, ng * nch), nd) : 0);
  TBG_SEC(chunk_fe, ARENA_WORK, lv ? FE * ng * nch : 0);
  TBG_SEC(cid_list, ARENA_WORK, lv ? 4 * ng * nch : 0);
  TBG_SEC(cid_p, ARENA_WORK, lv ? sizeof(G1A) * ng * nch * C : 0);
  TBG_SEC(grp_fe, ARENA_WORK, lv ? FE * ng : 0);
  TBG_SEC(gid_list, ARENA_WORK, lv ? 4 * ng : 0);
  TBG_SEC(gid_p, ARENA_WORK, lv ? sizeof(G1A) * ng * G : 0);
  TBG_SEC(gid_f, ARENA_WORK, lv ? FE * ng * (nch + 1) : 0);
  TBG_SEC(id_list, ARENA_WORK, lv ? 4 * nd : 0);
  TBG_SEC(id_p, ARENA_WORK, lv ? sizeof(G1A) * nd : 0);
  TBG_SEC(batch_pt, ARENA_WORK, p.l0 ? sizeof(G2A) : 0);
  TBG_SEC(batch_lines, ARENA_WORK, p.l0 ? LINES : 0);
  TBG_SEC(batch_f, ARENA_WORK, p.l0 ? FE : 0);
  TBG_SEC(grp_f, ARENA_WORK, p.l0 ? FE * grp_f_entries((uint32_t)ng) : 0);
  // level 1's group MSM (k_gmsm.hip): entries, offsets, bucket sums, leads, the failed groups' candidates
  TBG_SEC(gm_off, ARENA_WORK, G ? 4 * (GM_BUCKETS + 1) * ng : 0);
  TBG_SEC(gm_ent, ARENA_WORK, G ? 64 * vp : 0);
  TBG_SEC(gm_part, ARENA_WORK, G ? sizeof(G2J) * GM_BUCKETS * ng : 0);
  TBG_SEC(gm_lead, ARENA_WORK, G ? 4 * ng : 0);
  TBG_SEC(gm_list, ARENA_WORK, G ? 4 * vp : 0);
  TBG_SEC(gm_hist, ARENA_WORK, G ? 4 * 256 : 0);
  TBG_SEC(gm_order, ARENA_WORK, G ? 4 * GM_BUCKETS * ng : 0);
  // the batched subgroup test (k_sgb.hip)
  TBG_SEC(sgb_off, ARENA_WORK, 4 * sgsec([](uint32_t m) { return (size_t)sgb_off_stride(m); }));
  TBG_SEC(sgb_ent, ARENA_WORK, 4 * sgsec([](uint32_t m) { return (size_t)sgb_ent_stride(m); }));
  TBG_SEC(sgb_part, ARENA_WORK, sizeof(G2J) * sgsec([](uint32_t m) { return (size_t)sgb_part_stride(m); }));
  TBG_SEC(sgb_rank, ARENA_WORK, 4 * sgsec([](uint32_t m) { return (size_t)sgb_rank_stride(m); }));
  TBG_SEC(sgb_code, ARENA_WORK, tri ? 4 * SGB_TRIPLES * np : 0);
  TBG_SEC(sgb_bad, ARENA_WORK, 4 * std::max(n_sg, tri ? n_sg_small : 0));
  // level 0's S: the bucket MSM's arrays, or the fused path's
  TBG_SEC(msm_r, ARENA_WORK, p.msm ? 8 * vp : 0);
  TBG_SEC(msm_off, ARENA_WORK, p.msm ? 4 * (MSM_BUCKETS + 1) : 0);
  TBG_SEC(msm_cur, ARENA_WORK, p.msm ? 4 * MSM_BUCKETS : 0);
  TBG_SEC(msm_ent, ARENA_WORK, p.msm ? 16 * vp : 0);
  TBG_SEC(msm_bkt, ARENA_WORK, p.msm ? sizeof(G2J) * MSM_BUCKETS : 0);
  TBG_SEC(msm_part, ARENA_WORK, p.msm ? sizeof(G2J) * MSM_BUCKETS * MSM_SPLIT : 0);
  TBG_SEC(msm_sum, ARENA_WORK, p.msm ? sizeof(G2J) * MSM_SUM_ENTRIES : 0);
  TBG_SEC(sgb_t, ARENA_WORK, p.fused ? sizeof(G2J) * sgsec([](uint32_t m) { return (size_t)sgb_t_slices(m); }) : 0);
  TBG_SEC(l0f_sum, ARENA_WORK,
          p.fused ? sizeof(G2J) * std::max<size_t>(l0f_sum_entries((uint32_t)n_sg, p.sgb_m),
                                                   tri ? l0f_sum_entries((uint32_t)n_sg_small, p.sgb_m_small) : 0)
                  : 0);
  TBG_SEC(l0f_u, ARENA_WORK, p.fused ? 16 * np : 0);
  // level 0 by message: chunk sums and their member counts, Q_m, the messages' states
  TBG_SEC(l0m_part, ARENA_WORK, p.l0m ? sizeof(G1J) * p.l0m_chunks : 0);
  TBG_SEC(l0m_cnt, ARENA_WORK, p.l0m ? 4 * p.l0m_chunks : 0);
  TBG_SEC(l0m_q, ARENA_WORK, p.l0m ? sizeof(G1A) * nm : 0);
  TBG_SEC(l0m_state, ARENA_WORK, p.l0m ? 4 * nm : 0);
  TBG_SEC(agg_acc, ARENA_WORK, agg ? sizeof(G2J) * nd : 0);
  TBG_SEC(agg_list, ARENA_WORK, agg ? 4 * nd : 0);
  TBG_SEC_OPT(agg_aff, ARENA_WORK, p.aggver ? sizeof(G2A) * nd : 0);
  TBG_SEC_OPT(av_status, ARENA_WORK, p.aggver ? 4 * nd : 0);
  TBG_SEC_OPT(av_counters, ARENA_WORK, p.aggver ? 4 * CNT_WORDS : 0);

  TBG_SEC(partial_status, ARENA_OUT, 4 * np);
  TBG_SEC(duty_status, ARENA_OUT, 4 * nd);
  TBG_SEC(agg, ARENA_OUT, 96 * nd);
  TBG_SEC_OPT(set_status, ARENA_OUT, d.sets ? 4 * ((size_t)d.n_sets + SET_TAIL) : 0);
#undef TBG_SEC
#undef TBG_SEC_OPT
}

constexpr uint32_t kMaxSections = 96;
// A table that outgrew kMaxSections, or two walks of it that disagree, stop the process.
inline void plan_check(bool ok, const char* what) {
  if (ok) return;
  fprintf(stderr, "tbls_plan.h: %s\n", what);
  abort();
}
struct Section {
  const char* name;
  ArenaId arena;
  size_t off, bytes;  // off: from its arena's base (OUT: the work arena's); bytes: unaligned
};
// Where every section of a launch lies, with the plan and counts it was made from.
struct LaunchLayout {
  LaunchPlan plan{};
  LaunchDims dims{};
  uint32_t n = 0;
  Section sec[kMaxSections] = {};
  size_t in_bytes = 0, work_bytes = 0;
  size_t w_out = 0, out_bytes = 0;  // the output image inside the work arena
};

inline LaunchLayout layout(const LaunchPlan& p, const LaunchDims& d) {
  LaunchLayout L;
  L.plan = p;
  L.dims = d;
  Arena in, work;
  bool out = false;
  for_each_section(p, d, [&](const char* name, auto, ArenaId a, size_t bytes, bool) {
    if (a == ARENA_OUT && !out) {
      L.w_out = work.o;
      out = true;
    }
    plan_check(L.n < kMaxSections, "more sections than kMaxSections");
    L.sec[L.n++] = Section{name, a, (a == ARENA_IN ? in : work).take(bytes), bytes};
  });
  L.in_bytes = in.o;
  L.work_bytes = work.o;
  L.out_bytes = L.work_bytes - L.w_out;
  return L;
}

// The pointers of a launch's sections over the given arena bases (an arena
// whose base is null is left alone), and its scalar fields from the plan.
// `out`: the base of the output image when that is not the work arena's tail
// (the pinned copy of it).  Device, host input image and host output image
// are all views made here.
inline void bind(DevBatch& B, const LaunchLayout& L, uint8_t* in, uint8_t* work, uint8_t* out = nullptr) {
  const LaunchPlan& p = L.plan;
  if (work && !out) out = work + L.w_out;
  uint32_t i = 0;
  for_each_section(p, L.dims, [&](const char*, auto member, ArenaId a, size_t, bool null_when_empty) {
    plan_check(i < L.n, "bind walks more sections than the layout holds");
    const Section& s = L.sec[i++];
    uint8_t* base = a == ARENA_IN ? in : a == ARENA_WORK ? work : out;
    if (!base || (null_when_empty && !s.bytes)) return;
    using T = std::remove_reference_t<decltype(B.*member)>;
    B.*member = (T)(base + (a == ARENA_OUT ? s.off - L.w_out : s.off));
  });
  plan_check(i == L.n, "bind walks fewer sections than the layout holds");
  // one fallback line buffer (sig_lines), used level after level (DevBatch::fb_window)
  B.chunk_lines = B.cid_lines = B.gid_lines = B.id_lines = B.sig_lines;
  B.op = L.dims.op;
  B.n_duties = L.dims.n_duties;
  B.n_partials = L.dims.n_partials;
  B.n_msgs = L.dims.n_msgs;
  B.sets = L.dims.sets ? 1u : 0u;
  B.n_sets = L.dims.sets ? L.dims.n_sets : 0u;
  B.rlc_group = p.aggver ? 0u : p.G;  // (an aggver batch itself runs no check: its view does, av_group)
  B.rlc_chunk = p.C;
  B.rlc_batch = p.l0 && !p.aggver ? 1u : 0u;
  if (p.aggver) {
    B.av_group = p.G;
    B.av_chunk = p.C;
    B.av_batch = p.l0 ? 1u : 0u;
  }
  B.gident = p.gident;
  B.fb_window = p.fb_w;
  B.fb_full = p.fb_full;
  B.fb_base = 0;
  B.sgb = p.sgb ? 1u : 0u;
  B.sgb_m = p.sgb_m;
  B.sgb_split = p.sgb_split;
  B.l0_duty_partials = p.l0_duty_partials;
  B.l0_tail_partials = p.l0_tail_partials;
  B.l0_msg_share = p.l0_msg_share;
}

// A launch of d' duties / partials / messages (a prefix of the slot's device
// batch) under plan p' -- the slot's own but for (G, C) -- fits the arenas
// laid out as `slot`: every section's bytes stay within the slot's section of
// the same name, so a section added to the table is covered from then on.
// (G <= 64 on both sides or neither: level 1g's lines kernel runs a lane per
// duty of a group, and the slot's gident was decided for its own G.)
inline bool shape_fits(const LaunchLayout& slot, const LaunchPlan& p, const LaunchDims& d) {
  bool ok = (p.G <= 64) == (slot.plan.G <= 64);
  uint32_t i = 0;
  for_each_section(p, d, [&](const char*, auto, ArenaId, size_t bytes, bool) {
    plan_check(i < slot.n, "shape_fits walks more sections than the layout holds");
    ok = bytes <= slot.sec[i++].bytes && ok;
  });
  plan_check(i == slot.n, "shape_fits walks fewer sections than the layout holds");
  return ok;
}
// The same for the prefix of nd duties, np partials and nm messages at (G, C).
inline bool shape_fits(const LaunchLayout& slot, uint32_t nd, uint32_t np, uint32_t nm, uint32_t G, uint32_t C) {
  LaunchPlan p = slot.plan;
  LaunchDims d = slot.dims;
  p.G = G;
  p.C = C;
  d.n_duties = nd;
  d.n_partials = np;
  d.n_msgs = nm;
  return shape_fits(slot, p, d);
}

}  // namespace tbg
