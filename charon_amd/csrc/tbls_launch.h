// Host-side view of the engine's kernels: the device batch layout and one
// launcher per kernel (each defined next to its kernel in a k_*.hip
// translation unit, so the units compile in parallel and no relocatable
// device code is needed).
#pragma once
#include <hip/hip_runtime.h>
#include "bls_curve.h"
#include "bls_lines.h"
#include "../../include/tbls_gpu.h"

namespace tbg {

constexpr int kBlock = 64;
// Per-key G1 tables for the RLC products [r_i] pk_i: the 8-entry window
// table (bls_rlc.h rlc_mul_key_w2: 14 doublings + 16 additions)
constexpr uint32_t PK_TAB = 8;  // G1A entries per key in the resident table
// Default list positions per pass of the fallback levels' shared line buffer
// (22.8 KB each: 0.75 GB per slot; tbg_config.fb_window overrides it).
#ifndef TBG_FB_WINDOW
#define TBG_FB_WINDOW 32768u
#endif

// Minimum waves per SIMD requested from the register allocator (1 lets a
// kernel use all 512 / 2 = 256 VGPRs at two waves per SIMD; 3 caps it at
// 168).  A tuning knob: tools/ab_variants.py builds -DTBG_MIN_WAVES=N.
#ifndef TBG_MIN_WAVES
#define TBG_MIN_WAVES 1
#endif
#define TBG_LAUNCH __launch_bounds__(64, TBG_MIN_WAVES)
// Kernels split by phase ask for the occupancy their footprint allows: at
// least two waves per SIMD (<= 256 VGPRs), because a lone wave issues the
// multiply-adds at ~58 % of the two-wave rate (profiles/r02/valu_rates.txt).
#ifndef TBG_PAIR_WAVES
#define TBG_PAIR_WAVES 2    // lane-pair G2 kernels (bls_pair.h)
#endif
#ifndef TBG_DECODE_WAVES
#define TBG_DECODE_WAVES 2  // k_decode_sigs (square roots only)
#endif
#define TBG_LAUNCH_N(w) __launch_bounds__(64, w)
// Latency-critical kernels of a launch's serial tail (the level-0 bucket
// reduction, S's lines, the product tree, the one final exponentiation) run
// a few waves each, often on SIMDs that also host other launches' long
// Miller / decode waves, which halve their issue rate (k_l0_final 3.4 ms
// alone, 6.8 ms beside a Miller kernel, profiles/r04/base/timeline_s20.txt).
// s_setprio 3 makes their waves win the SIMD's instruction arbitration;
// the throughput kernels lose nothing but the slots these few waves use.
#if defined(__HIP_DEVICE_COMPILE__)
#define TBG_URGENT() __builtin_amdgcn_s_setprio(3)
#else
#define TBG_URGENT() ((void)0)
#endif
inline dim3 grid_for(uint32_t n) { return dim3((n + kBlock - 1) / kBlock); }

// Device-side layout of one batch (all pointers into device memory).
struct DevBatch {
  uint32_t op, n_duties, n_partials, n_msgs;
  const uint8_t* msgs;
  const uint32_t* msg_off;
  const uint32_t* duty_msg;
  const uint32_t* duty_first;
  const uint32_t* duty_threshold;
  const uint32_t* partial_duty;
  const uint8_t* sigs;
  const uint8_t* identifiers;
  const uint32_t* pubkey_ids;
  // work buffers
  G2A* sig_aff;
  G2A* h_aff;
  int32_t* h_status;
  G2J* h_jac;          // [3 n_msgs] H(m) before affine conversion (k_hash_map / _clear / _affine), then
                       // the cofactor clearing's temporaries [x]P and [x]P + psi(P) (k_hash_clear.hip)
  uint32_t* lam;       // [n_partials][8] scalar words
  uint32_t* sig_lines;  // [fb window][LINES_WORDS] Miller lines of listed signatures (-g1 folded in)
  uint32_t* h_lines;    // [n_msgs][LINES_WORDS] Miller lines of each H(m) (G1 factor left out)
  // random-linear-combination verification (k_rlc.hip)
  uint32_t rlc_seed[8];   // secret per-batch key of the scalars r_i
  uint32_t rlc_group;     // duties per level-1 group; 0 = per-partial checks only
  G1J* part_p;            // [n_partials] r_i pk_i
  G2J* part_s;            // [n_partials] r_i sig_i
  uint32_t rlc_chunk;     // duties per level-1 Miller chunk (quads per group = ceil(G / chunk))
  uint32_t* chunk_f;      // [n_groups * (chunks + 1)][3][4 NL] Miller products of the chunks (quad layout);
                          // chunk index `chunks` of a group is its S pair alone
  uint32_t* chunk_list;   // [n_groups * chunks] level-1.5 chunks of failed groups (group * chunks + c)
  uint32_t* chunk_lines;  // [fb window][LINES_WORDS] lines of S_c, by chunk-list position - fb_base
  G1A* dv_p;              // [n_duties] sum r_i pk_i (affine), stored as (-x, y)
  G2J* dv_s;              // [n_duties] sum r_i sig_i
  int32_t* dv_state;      // [n_duties] RLC_*
  int32_t* grp_state;     // [n_groups] GRP_*
  uint32_t* grp_lines;    // [n_groups][LINES_WORDS] lines of the group's S (-g1 folded in)
  uint32_t* counters;     // [CNT_*] work-list lengths
  uint32_t* part_list;    // [n_partials] level-3 partials (sig_lines by list position)
  G2A* pend_pts;          // [max(n_groups, n_groups * chunks, n_duties)] affine points whose folded Miller
                          // lines k_lines_fold computes next (group S, then the fallback lists' sums)
  uint32_t* chunk_fe;     // [n_groups * chunks][3][4 NL] final-exponentiated value of failed chunks (by list position)
  uint32_t* cid_list;     // [n_groups * chunks] level-1.5b entries: chunk-list positions
  G1A* cid_p;             // [n_groups * chunks][rlc_chunk] w_d P_d as (-x, y), by level-1.5b position
  uint32_t* cid_lines;    // [fb window][LINES_WORDS] lines of sum w_d S_d, by level-1.5b position - fb_base
  // level 1g: the exponent test over a failed GROUP's partials, right after
  // level 1 (most failed groups hold exactly one bad partial)
  uint32_t gident;        // 1: failed groups go to level 1g first, its unresolved ones to level 3
                          // (2: to level 1.5; 0: no level 1g)
  uint32_t* grp_fe;       // [n_groups][3][4 NL] final-exponentiated value A_g of a level-1g group (by list position)
  uint32_t* gid_list;     // [n_groups] level-1g entries: group index (| ID_DEGENERATE)
  G1A* gid_p;             // [n_groups][rlc_group] sum_(i in d) w_i r_i pk_i as (-x, y): level-1g position, duty in group
  uint32_t* gid_lines;    // lines of sum w_i r_i sig_i by level-1g position - fb_base (the fallback line buffer)
  uint32_t* gid_f;        // [n_groups][chunks + 1][3][4 NL] Miller products of a level-1g entry (chunks, then S')
  uint32_t* id_fe;        // [n_duties][3][4 NL] value A_d of each level-2b duty (by list position)
  uint32_t* id_list;      // [n_duties] level-2b entries: failed duties with several candidates
  G1A* id_p;              // [n_duties] sum w_i r_i pk_i (affine), by level-2b position
  // The fallback levels' line buffers (chunk_lines, cid_lines, id_lines,
  // sig_lines) are ONE buffer of fb_window entries (0: unbounded), used in
  // stream order: each level's lines are written and consumed in passes of
  // fb_window list positions [fb_base, fb_base + fb_window) before the next
  // level writes (launch_rlc_check) -- a slot's HBM no longer scales with the
  // worst-case list length (22.8 KB per partial of every batch).
  uint32_t fb_window, fb_base;
  // Passes of the duty (level 2b) and partial (level 3) lists start full grids
  // only below fb_full list positions (the list lengths the collected batches'
  // invalid share makes likely); later passes launch a few waves that loop
  // over the pass (k_verify_list, k_lines_sig_list, k_rlc_ident_check,
  // k_lines_fold), so a clean batch does not dispatch ~80k empty waves of 20
  // partial passes per 16-batch launch (round 6).  UINT32_MAX: every pass full.
  uint32_t fb_full;
  uint32_t* id_lines;     // lines of sum w_i r_i sig_i by level-2b position: aliases sig_lines,
                          // which level 3 only fills after level 2b has consumed them
  // level 0 (k_msm.hip, k_rlc.hip): the whole device batch as ONE RLC check,
  //   prod_d e(P_d, H(m_d)) * e(-g1, S) == 1,  S = sum_i r_i s_i,
  // S as a bucket MSM over the signatures and their psi images (no per-partial
  // G2 scalar multiplication) -- or, while the batched subgroup test runs, from
  // that test's sums (l0_fused below; the msm_* arrays are then not allocated);
  // a failure falls through to the group levels
  uint32_t rlc_batch;     // 1: level 0 runs first (every candidate's r_i random, no group lead)
  uint32_t l0_tail_partials;  // fused launches of at least this many partials form S inside the key-side
                              // kernel's grid (l0_tail below; only the launchers read it)
  uint64_t* msm_r;        // [n_partials] r_i of the candidates
  uint32_t* msm_off;      // [MSM_BUCKETS + 1] bucket sizes, then their offsets
  uint32_t* msm_cur;      // [MSM_BUCKETS] scatter cursors
  uint32_t* msm_ent;      // [4 n_partials] bucket entries: partial << 3 | k << 1 | negative
  G2J* msm_part;          // [MSM_BUCKETS * MSM_SPLIT] sums of the bucket slices
  G2J* msm_bkt;           // [MSM_BUCKETS] (2j + 1) * (bucket j's sum)
  G2J* msm_sum;           // [MSM_SUM_ENTRIES] tree sums of msm_bkt
  G2A* batch_pt;          // [1] S in affine form
  uint32_t* batch_lines;  // [LINES_WORDS] Miller lines of S (-g1 folded in)
  uint32_t* batch_f;      // [3][4 NL] Miller product of the S pair (quad layout)
  uint32_t* grp_f;        // [GRP_F_ENTRIES(n_groups)][3][4 NL] each group's P-chunk product, then the product tree
  // level 1's group sums S_g = sum_i r_i s_i as one bucket MSM per group
  // (k_gmsm.hip): 4-bit windows of the four psi digits,
  // no per-partial G2 scalar multiplication; the per-partial products r_i s_i
  // are formed afterwards for the failed groups' candidates only
  uint32_t* gm_off;       // [n_groups][GM_BUCKETS + 1] bucket offsets into the group's entries
  uint32_t* gm_ent;       // [16 n_partials] entries (partial << 3 | k << 1 | negative); group g's
                          // start at 16 * (its first partial)
  G2J* gm_part;           // [n_groups][GM_BUCKETS] bucket sums, then the window sums T_w at w * GM_V
  uint32_t* gm_lead;      // [n_groups] the group's r = 1 partial (UINT32_MAX: none / level 0's scalars)
  uint32_t* gm_list;      // [n_partials] candidates of failed groups, whose r_i s_i are formed afterwards
  uint32_t* gm_hist;      // [256] bucket-size histogram, then the size-order cursors
  uint32_t* gm_order;     // [n_groups * GM_BUCKETS] buckets by decreasing size (k_gm_bucket's order)
  // batched subgroup test of the decoded signatures (k_sgb.hip): per group
  // of SGB_M consecutive partials, SGB_K random combinations sum c_i s_i with
  // c_i uniform mod 13 are tested psi(Q) == [x] Q; only the members of a
  // failed group take the per-signature test (k_subgroup_sigs)
  uint32_t sgb;           // 1: the batched test runs (0: every signature is tested alone)
  uint32_t sgb_m;         // consecutive partials per group (a power of two, SGB_M_MIN..SGB_M; larger: the
                          // triple schedule, sgb_triple below)
  uint32_t sgb_split;     // slices per bucket (k_sgb_bucket / k_sgb_fold)
  uint32_t sgb_seed[8];   // secret per-batch key of the combinations' digits: always fresh OS
                          // entropy, even under a fixed rlc_seed (a predictable key would let a
                          // submitter craft torsion components that cancel across combinations)
  uint32_t* sgb_off;      // [n_sg][sgb_off_stride] bucket offsets into the group's entries
  uint32_t* sgb_ent;      // [n_sg][sgb_ent_stride] entries: member << 1 | negative
  G2J* sgb_part;          // [n_sg][sgb_part_stride] bucket (slice) sums; Q_k at sgb_q_slot
  uint32_t* sgb_rank;     // [n_sg][SGB_PBUCKETS / SGB_TBUCKETS] paired and triple schedules: the group's
                          // buckets by decreasing entry count
  uint32_t* sgb_code;     // [n_partials][SGB_TRIPLES] triple schedule: bucket | negative << 11 | place in
                          // its bucket << 12 (k_sgb_tri_count -> k_sgb_tri_scatter), SGBT_NONE: no entry
  uint32_t* sgb_bad;      // [n_sg] 1: some combination is outside G2 (members tested alone)
  // fused level 0 (l0_fused below): S from the subgroup test's sums
  G2J* sgb_t;             // [n_sg][sgb_t_slices(sgb_m)] slice sums of the group's unweighted candidates
  G2J* l0f_sum;           // [l0f_sum_entries] chunk sums of the Q_k columns and of T, then the L0F_COLS
                          // column totals (the S role of k_rlc_g1_l0, bls_l0tail.h; in launches below
                          // l0_tail_partials k_l0f_reduce, then k_l0f_fold, with 512-point chunks)
  uint32_t* l0f_u;        // [n_partials][4] the digits u_j of the fused r_i (k_sgb_sort -> k_rlc_g1_l0)
  uint32_t l0_duty_partials;   // fused launches of at least this many partials form P_d per duty (l0_per_duty below)
  // level 0 by message (l0_by_msg below; bls_l0msg.h, k_l0msg.hip): one G1 sum
  // Q_m per distinct message, so the Miller kernel evaluates H(m)'s lines once
  // per message.  The plan is packed by the host with the launch's inputs.
  uint32_t l0_msg_share;       // fused launches with at least this many duties per message pair per message
  uint32_t l0m_n_chunks;       // chunks of this launch's messages (a replayed prefix: its own count)
  uint32_t l0m_max_chunks;     // chunks of its largest message (the fold's pass count, l0m_passes)
  const uint32_t* msg_first;   // [n_msgs + 1] CSR offsets into msg_duty
  const uint32_t* msg_duty;    // [n_duties] duties by message, ascending inside a message
  const uint32_t* l0m_chunk_first;  // [n_msgs + 1] first chunk of each message
  const uint32_t* l0m_chunk_msg;    // [l0m_chunk_bound] message of each chunk
  G1J* l0m_part;               // [l0m_chunk_bound] chunk sums, folded in place
  uint32_t* l0m_cnt;           // [l0m_chunk_bound] combined duties in each sum
  G1A* l0m_q;                  // [n_msgs] Q_m = sum of the message's P_d (affine), stored as (-x, y)
  int32_t* l0m_state;          // [n_msgs] L0M_* (bls_l0msg.h)
  // recombination (k_aggregate.hip)
  G2J* agg_acc;           // [n_duties] integer-coefficient sums awaiting [1/D] (listed duties only)
  uint32_t* agg_list;     // [n_duties] duties whose Lagrange denominator D > 1
  // outputs
  int32_t* partial_status;
  int32_t* duty_status;
  uint8_t* agg;        // [n_duties][96]
  // set launch (tbg_submit_sets, k_sets.hip): per set, whether every member
  // verifies; a failed group fails its set with no narrowing.  Every set
  // starts on a multiple of rlc_group (empty padding duties, packed by the
  // host), so a level-1 group lies inside one set.
  uint32_t sets;              // 1: a set launch
  uint32_t n_sets;
  const uint32_t* duty_set;   // [n_duties] the duty's set
  int32_t* set_status;        // [n_sets + SET_TAIL] TBG_SS_* per set (outputs), then SET_BAD, SET_ANY
  // aggregate, then verify the aggregate (TBG_OP_AGGREGATE_VERIFY, k_aggver.hip): the batch
  // itself decodes and recombines as TBG_OP_AGGREGATE does (rlc_group = rlc_batch = 0: no
  // check of the partials); the checks run on a second VIEW of it, aggver_view below, in
  // which every duty is one candidate -- its affine aggregate, handed over in agg_aff.
  // The view's shape and the arrays only it owns are kept here, so that a replayed prefix
  // derives its view from its own fields.  All null / 0 for every other op.
  G2A* agg_aff;               // [n_duties] the affine aggregates (written beside the compressed bytes)
  int32_t* av_status;         // [n_duties] the view's partial_status
  uint32_t* av_counters;      // [CNT_WORDS] the view's counters
  const uint32_t* av_iota;    // [n_duties + 1] 0, 1, 2, ...: the view's duty_first and partial_duty
  uint32_t av_group, av_chunk, av_batch;  // the view's rlc_group, rlc_chunk, rlc_batch
};
static_assert(offsetof(DevBatch, msm_r) == offsetof(DevBatch, rlc_batch) + 8, "l0_tail_partials fills rlc_batch's padding");
// set_status's tail words: SET_BAD counts the partials left invalid or
// unverified (every candidate of a failed group: the adaptive policies' upper
// bound), SET_ANY the partials whose code is not VALID (0: nothing to rewrite)
enum SetTail : int { SET_BAD = 0, SET_ANY = 1, SET_TAIL = 2 };

enum RlcState : int32_t { RLC_NONE = 0, RLC_COMBINED = 1, RLC_EACH = 2 };
enum GroupState : int32_t { GRP_EMPTY = 0, GRP_LINES = 1, GRP_OK = 2, GRP_FAIL = 3, GRP_GID = 4,  // GRP_GID: at level 1g
                            GRP_BAD = 5 };  // a set launch's group whose check failed (GRP_FAIL: its sum was degenerate)
// CNT_DUTIES: level-2b duties (id_list), CNT_PARTIALS: level-3 partials, CNT_AGG: [1/D] duties,
// CNT_CHUNKS: level-1.5 chunks, CNT_CID: level-1.5b chunks, CNT_L0_BAD: level 0 cannot
// hold (a degenerate sum, a duty checked per partial, an unusable H(m)), CNT_L0_OK: level 0 passed
// CNT_L0F_COL + col: the chunk sums of column col stored so far, CNT_L0F_DONE: the column totals
// stored so far (the fused level 0's S role, bls_l0tail.h: the last arriver goes on).  Like every
// counter they are zeroed by k_decode_sigs at the head of each chain, replays included.
enum Counter : int { CNT_DUTIES = 0, CNT_PARTIALS = 1, CNT_AGG = 2, CNT_CHUNKS = 3, CNT_CID = 4, CNT_L0_BAD = 5,
                     CNT_L0_OK = 6, CNT_GID = 7, CNT_LAZY = 8,  // CNT_GID: level-1g groups, CNT_LAZY: gm_list entries
                     CNT_L0F_COL = 9, CNT_L0F_DONE = CNT_L0F_COL + 19, CNT_WORDS = CNT_L0F_DONE + 1 };

// Level-0 MSM: a digit a (odd, |a| < 2^16) of r_i puts psi^k(s_i) into bucket
// (|a| - 1) / 2; the tree sums (k_msm_tree) leave one point per workgroup in
// msm_sum.
constexpr uint32_t MSM_BUCKETS = 32768;
constexpr uint32_t MSM_SPLIT = 4;  // slices per bucket (k_msm_bucket_part)
constexpr uint32_t MSM_SUM_ENTRIES = 128;
// Batched subgroup test (k_sgb.hip).  A point of E2(Fp2) outside G2 has a
// component of order divisible by a prime factor of the G2 cofactor, the
// smallest of which is 13: with c_i uniform mod 13 (signed digits -6..6) a
// combination hides such a component with probability <= 1/13, so SGB_K =
// 18 independent combinations leave 13^-18 < 2^-66.
#ifndef TBG_SGB_M
#define TBG_SGB_M 1024
#endif
#ifndef TBG_SGB_SPLIT
#define TBG_SGB_SPLIT 4
#endif
// The group size follows the non-subgroup share of the collected batches
// (sgb_plan, tbls_plan.h): SGB_M while clean, down to SGB_M_MIN when a
// few signatures per thousand are outside G2 (a failed group costs its
// members' per-signature tests).
constexpr uint32_t SGB_M = TBG_SGB_M;  // largest group: consecutive partials (LDS of k_sgb_sort)
constexpr uint32_t SGB_M_MIN = 64;
constexpr uint32_t SGB_K = 18;         // combinations per group
constexpr uint32_t SGB_V = 6;          // buckets per combination (|c| = 1..6)
constexpr uint32_t SGB_BUCKETS = SGB_K * SGB_V;
constexpr uint32_t SGB_SPLIT = TBG_SGB_SPLIT;  // slices per bucket at SGB_M (~40 additions each)
constexpr uint32_t SGB_MIN_PARTIALS = 2 * SGB_M;  // smaller batches test each signature alone
TBG_HD uint32_t sgb_groups(uint32_t n_partials, uint32_t m) { return (n_partials + m - 1) / m; }
// slices per bucket for groups of m: ~40 entries per slice, at least one
TBG_HD uint32_t sgb_split_for(uint32_t m) {
  const uint32_t s = SGB_SPLIT * m / SGB_M;
  return s ? s : 1u;
}
// Paired schedule (k_sgb.hip) for groups of at least SGB_PAIR_M: a member is
// sorted by two of its digits at once, (c_2p, c_2p+1) for the SGB_PAIRS pairs
// of combinations, into one of SGB_PB two-dimensional buckets per pair -- one
// addition per pair instead of one per combination; no slices.  Smaller
// groups keep the classic one-dimensional buckets: the paired reductions
// (~1,500 additions per group whatever its size) and its many short buckets
// cost more than the halved bucket additions save.
constexpr uint32_t SGB_PAIR_M = 256;
constexpr uint32_t SGB_PAIRS = SGB_K / 2;
constexpr uint32_t SGB_PB = SGB_V + SGB_V * (2 * SGB_V + 1);  // 84: a = 0 has b = 1..6, a = 1..6 has b = -6..6
constexpr uint32_t SGB_PBUCKETS = SGB_PAIRS * SGB_PB;         // 756 per group
constexpr uint32_t SGB_PRANK = (SGB_PBUCKETS + 31) / 32 * 32;  // k_sgb_bucket's lane pairs per group: whole waves
// Triple schedule (k_sgb.hip) for groups LARGER than SGB_M: the same step
// again, a member sorted by three digits at once, (c_3t, c_3t+1, c_3t+2) for
// the SGB_TRIPLES triples of combinations, into one of SGB_TB = (13^3 - 1) / 2
// buckets per triple -- 6 x 2196/2197 = 6.0 additions per member instead of
// 8.9.  Its reductions cost ~2,400 additions per triple whatever the group's
// size, so it pays only in groups of many thousands, which no longer fit the
// sort's LDS: the sort runs in global memory (k_sgb_tri_*).  Only large clean
// launches take it (sgb_plan, tbls_plan.h; tbg_config.sgb_tri_partials,
// sgb_tri_m); every group of at most SGB_M keeps the schedules above.
#ifndef TBG_SGB_TRI_M
#define TBG_SGB_TRI_M 16384
#endif
constexpr uint32_t SGB_TRI_M = TBG_SGB_TRI_M;    // default group size of the triple schedule
constexpr uint32_t SGB_TRI_M_MAX = 32768;        // (entries hold member << 1 in 16 bits, codes a place < 2^20)
constexpr uint32_t SGB_TRIPLES = SGB_K / 3;
constexpr uint32_t SGB_TB = SGB_PB + SGB_V * (2 * SGB_V + 1) * (2 * SGB_V + 1);  // 1,098: a = 0 is a pair's 84
constexpr uint32_t SGB_TBUCKETS = SGB_TRIPLES * SGB_TB;                          // 6,588 per group
constexpr uint32_t SGB_TRANK = (SGB_TBUCKETS + 31) / 32 * 32;  // k_sgb_bucket's lane pairs per group: whole waves
// k_sgb_fold's first pass per triple: the 84 sums P(a, b) over c, then the 84
// partial sums E(v, a, sign) of the third combination (bls_sgb.h)
constexpr uint32_t SGB_TF1 = 2 * SGB_PB;
static_assert(SGB_TRI_M > SGB_M && SGB_TRI_M <= SGB_TRI_M_MAX && (SGB_TRI_M & (SGB_TRI_M - 1)) == 0, "SGB_TRI_M");
TBG_HD bool sgb_triple(uint32_t m) { return m > SGB_M; }
TBG_HD bool sgb_paired(uint32_t m) { return m >= SGB_PAIR_M && !sgb_triple(m); }
// per-group strides of sgb_off, sgb_ent and sgb_part in each schedule
// (paired: the SGB_PBUCKETS bucket sums, then the SGB_BUCKETS sums of
// k_sgb_fold laid out as the classic schedule's folded buckets; triple: the
// SGB_TBUCKETS bucket sums, the first pass's SGB_TRIPLES x SGB_TF1 sums, then
// the same SGB_BUCKETS folded sums)
TBG_HD uint32_t sgb_off_stride(uint32_t m) {
  return (sgb_triple(m) ? SGB_TBUCKETS : sgb_paired(m) ? SGB_PBUCKETS : SGB_BUCKETS) + 1;
}
TBG_HD uint32_t sgb_ent_stride(uint32_t m) {
  return m * (sgb_triple(m) ? SGB_TRIPLES : sgb_paired(m) ? SGB_PAIRS : SGB_K);
}
TBG_HD uint32_t sgb_rank_stride(uint32_t m) { return sgb_triple(m) ? SGB_TBUCKETS : sgb_paired(m) ? SGB_PBUCKETS : 0u; }
constexpr uint32_t SGB_TFOLD = SGB_TBUCKETS + SGB_TRIPLES * SGB_TF1;  // the triple schedule's folded sums in a group
TBG_HD uint32_t sgb_part_stride(uint32_t m) {
  return sgb_triple(m)   ? SGB_TFOLD + SGB_BUCKETS
         : sgb_paired(m) ? SGB_PBUCKETS + SGB_BUCKETS
                         : SGB_BUCKETS * sgb_split_for(m);
}
// Q_k of group g (k_sgb_combine's output; k_sgb_test and the fused level 0 read it)
TBG_HD size_t sgb_q_slot(const DevBatch& B, uint32_t g, uint32_t k) {
  return (size_t)sgb_part_stride(B.sgb_m) * g + (sgb_triple(B.sgb_m)   ? SGB_TFOLD + SGB_V * k
                                                 : sgb_paired(B.sgb_m) ? SGB_PBUCKETS + SGB_V * k
                                                                       : SGB_V * k * B.sgb_split);
}
// (the same from the two fields alone: the S role of k_rlc_g1_l0 is an out-of-line body that is
// handed the launch's fields it needs, not the DevBatch)
TBG_HD size_t sgb_q_slot(uint32_t m, uint32_t split, uint32_t g, uint32_t k) {
  return (size_t)sgb_part_stride(m) * g + (sgb_triple(m)   ? SGB_TFOLD + SGB_V * k
                                           : sgb_paired(m) ? SGB_PBUCKETS + SGB_V * k
                                                           : SGB_V * k * split);
}
// Fused level 0 (bls_rlc.h, k_msm.hip): while the batched subgroup test runs,
// r_i is a fixed linear form of the partial's 18 subgroup digits, so S is a
// fixed linear form of the test's sums Q_k (summed over the groups) and of the
// unweighted sum T of the candidates -- no bucket MSM.  The host and every
// kernel decide the path from the launch's own fields.
TBG_HD bool l0_fused(const DevBatch& B) {
  return B.rlc_batch && B.rlc_group && B.sgb && B.n_partials;
}
// The fused level 0's key side (k_rlc_g1_l0, k_msm.hip) runs one lane per
// DUTY -- P_d in Straus' joint form, the 18 doublings once per duty
// (bls_rlc.h rlc_duty_keys_l0f), affine P_d written by the same kernel -- in
// launches of at least l0_duty_partials partials.  Smaller launches keep one lane per
// partial and k_rlc_duty_sum<DSUM_L0_P>: with few waves the kernel's time is
// one lane's chain, and the duty's chain is about three times the partial's
// (tbg_config.l0_duty_partials, default TBG_L0_DUTY_PARTIALS).
// The saving grows with the candidates of the launch and the cost with its
// few, long waves, so the rule counts partials (config 3: 100k duties of ten).
// A replayed prefix decides from its own partials.
TBG_HD bool l0_per_duty(const DevBatch& B) { return l0_fused(B) && B.n_partials >= B.l0_duty_partials; }
// Level 0 by message (bls_l0msg.h, k_l0msg.hip).  By bilinearity
//   prod_(d: m_d = m) e(P_d, H(m)) = e(sum_d P_d, H(m)),
// so a fused launch in which messages are shared pairs ONE key sum Q_m per
// distinct message: the 68 line evaluations of H(m) run once per message
// instead of once per duty, against one mixed G1 addition per merged duty.
// Fused launches only: a failed or void fused level 0 keeps nothing (the P
// chunks are formed again with the classic scalars, launch_rlc_check), so no
// fallback level sees the merged products.  l0_msg_share is the least number
// of duties per distinct message at which a launch merges
// (tbg_config.l0_msg_share, default TBG_L0_MSG_SHARE).  Decided from the
// launch's own fields: a replayed prefix from its own duties and messages, a
// set launch from its padded duties, a tbg_multi shard per shard.
TBG_HD bool l0_by_msg(const DevBatch& B) {
  return l0_fused(B) && B.l0_msg_share != TBG_L0_MSG_NEVER && (uint64_t)B.n_msgs * B.l0_msg_share <= B.n_duties;
}
constexpr uint32_t SGB_T_PER = 32;  // candidates per slice of T (no longer a chain than a bucket slice's ~40)
TBG_HD uint32_t sgb_t_slices(uint32_t m) { return m / SGB_T_PER; }  // (m: a power of two >= SGB_M_MIN = 64)
constexpr uint32_t L0F_COLS = SGB_K + 1;        // the 18 sums over the groups of Q_k, then T
// The S role of k_rlc_g1_l0 (bls_l0tail.h, whose L0T_* constants k_msm.hip checks against
// these): one wave per chunk -- kBlock / 2 lane pairs, 4 points per pair.  l0f_sum is sized for
// these chunks; the 512-point chunks of k_l0f_reduce (L0FK_*, smaller launches) need fewer entries.
constexpr uint32_t L0F_PAIRS = kBlock / 2, L0F_PER = 4;
constexpr uint32_t L0F_CHUNK = L0F_PAIRS * L0F_PER;
constexpr uint32_t L0FK_PAIRS = 128, L0FK_PER = 4;  // k_l0f_reduce: lane pairs per workgroup, points per pair
constexpr uint32_t L0FK_CHUNK = L0FK_PAIRS * L0FK_PER;
static_assert(L0FK_CHUNK >= L0F_CHUNK, "l0f_sum holds either chunking");
TBG_HD uint32_t l0fk_q_chunks(uint32_t n_sg) { return (n_sg + L0FK_CHUNK - 1) / L0FK_CHUNK; }
TBG_HD uint32_t l0fk_t_chunks(uint32_t n_sg, uint32_t m) { return (n_sg * sgb_t_slices(m) + L0FK_CHUNK - 1) / L0FK_CHUNK; }
static_assert(CNT_L0F_DONE - CNT_L0F_COL == (int)L0F_COLS, "one counter per column");
TBG_HD uint32_t l0f_q_chunks(uint32_t n_sg) { return (n_sg + L0F_CHUNK - 1) / L0F_CHUNK; }
TBG_HD uint32_t l0f_t_chunks(uint32_t n_sg, uint32_t m) { return (n_sg * sgb_t_slices(m) + L0F_CHUNK - 1) / L0F_CHUNK; }
TBG_HD uint32_t l0f_sum_entries(uint32_t n_sg, uint32_t m) {
  return SGB_K * l0f_q_chunks(n_sg) + l0f_t_chunks(n_sg, m) + L0F_COLS;
}
// S inside the key-side kernel's grid (bls_l0tail.h) in fused launches of at least
// l0_tail_partials partials (tbg_config.l0_tail_partials, default TBG_L0_TAIL_PARTIALS = 131,072:
// 2,048 wave slots x 64 lanes, from where the key side fills every wave slot of the machine and
// lasts longer than the S chain it hides).  Below it the key side is one wave's chain, shorter
// than the S chain, which as a role runs out-of-line point operations: nothing would be hidden,
// and the launch keeps k_l0f_reduce, k_l0f_fold and k_l0f_horner after the aggregation.  A
// replayed prefix decides from its own partials.  Same S either way.
TBG_HD bool l0_tail(const DevBatch& B) { return l0_fused(B) && B.n_partials >= B.l0_tail_partials; }
// the S role's workgroups in such a launch's key-side grid (the lowest block indices)
TBG_HD uint32_t l0f_s_blocks(const DevBatch& B) {
  const uint32_t n_sg = sgb_groups(B.n_partials, B.sgb_m);
  return SGB_K * l0f_q_chunks(n_sg) + l0f_t_chunks(n_sg, B.sgb_m);
}
// Level-0 product tree over the groups' P-chunk products.  Each pass is a
// chain of F - 1 Fp12 products on one lane group (~24 us each at one wave per
// SIMD), so the tree's latency ~ log_F(n) * F is smallest near F = 4 (16: 1.3
// ms for 10k groups; 4: ~0.7 ms) -- it sits on every launch's critical path.
constexpr uint32_t L0_TREE_FAN = 4;
// (sum over the passes of ceil(n / F^k) <= n / (F - 1) + one per pass)
TBG_HD uint32_t grp_f_entries(uint32_t n_groups) { return n_groups + n_groups / (L0_TREE_FAN - 1) + 40; }
// k_miller_hex modes
enum MillerMode : int { MILLER_GROUPS = 0, MILLER_L0 = 1, MILLER_GROUP_S = 2 };
// k_rlc_duty_sum phases
//   DSUM_P: P_d only (level 1's S comes from the group MSM, k_gmsm.hip);
//   DSUM_FALLBACK_S: S_d of the failed groups' duties, from the r_i s_i formed
//   for them after the group checks
enum DutySumPhase : int { DSUM_L0_P = 1, DSUM_FALLBACK_S = 2, DSUM_P = 3 };
// Level 1's group MSM (k_gmsm.hip): each 16-bit digit a_k of r_i (bls_rlc.h)
// read as four 4-bit windows of signed binary digits, v = 2 nibble - 15 (odd,
// |v| <= 15): 16 entries per partial into GM_BUCKETS = 4 windows x 8 buckets
// (|v| = 2b + 1) per group.
constexpr uint32_t GM_W = 4, GM_V = 8, GM_BUCKETS = GM_W * GM_V;

// Flags in the fallback lists (k_rlc.hip): the entry's sum is the point at
// infinity -- no lines, its members go to an exact level.
constexpr uint32_t CHUNK_DEGENERATE = 0x80000000u;
constexpr uint32_t ID_DEGENERATE = 0x80000000u;
// k_lines_fold<KIND>: which pending points get lines, and where they go.
enum FoldKind : int { FOLD_GROUPS = 0, FOLD_CHUNKS = 1, FOLD_CID = 2, FOLD_IDENT = 3, FOLD_GID = 5 };

// Fallback list position k in the current pass, and its slot in the line buffer.
TBG_HD bool fb_in_pass(const DevBatch& B, uint32_t k) { return B.fb_window == 0 || k - B.fb_base < B.fb_window; }
TBG_HD size_t fb_slot(const DevBatch& B, uint32_t k) { return (size_t)LINES_WORDS * (k - B.fb_base); }
// The list positions of the current pass, from `first` in steps of `stride`
// (a grid smaller than the pass loops): stops at the list's end or the pass's.
template <class F>
TBG_HD void fb_pass_loop(const DevBatch& B, uint32_t first, uint32_t stride, uint32_t count, F&& body) {
  const uint32_t w = B.fb_window ? B.fb_window : 0xFFFFFFFFu;
  for (uint32_t s = first; s < w; s += stride) {
    const uint32_t k = B.fb_base + s;
    if (k >= count) break;
    body(k);
  }
}
// The list positions a grid of `threads` holds at one lane pair each: the
// stride of a pair kernel that loops (the hexad kernels': hex_slots_of, bls_hex.h).
TBG_HD uint32_t pair_slots_of(uint32_t threads) { return threads >> 1; }
// The fallback levels' list positions [0, max_entries) in passes of
// B.fb_window (the line buffer's capacity; 0: one pass), in stream order.
// body(P, n): n = the list positions the pass's grids cover -- all of the
// pass below B.fb_full, else FB_SMALL (the pass kernels that may run small
// loop over the rest: fb_pass_loop; the others take n = the pass).
constexpr uint32_t FB_SMALL = 640;  // 64 hexad waves, 20 pair waves
template <class F>
inline void fb_passes(const DevBatch& B, uint32_t max_entries, F&& body, bool may_shrink = false) {
  const uint32_t W = B.fb_window ? B.fb_window : max_entries;
  for (uint32_t base = 0; base < max_entries; base += W) {
    DevBatch P = B;
    P.fb_base = base;
    const uint32_t n = max_entries - base < W ? max_entries - base : W;
    body(P, may_shrink && base > 0 && base >= B.fb_full && n > FB_SMALL ? FB_SMALL : n);  // (pass 0 always full)
  }
}

// Participation of a partial in its duty's aggregate.  SPEC: the
// speculative aggregation that runs BEFORE verification while level 0 is on
// (launch_chain): every candidate counts as valid, which is what a level-0
// pass concludes; after a failed level 0 the aggregation runs again.
template <bool SPEC = false>
TBG_HD bool participates(uint32_t op, int32_t st) {
  return op == TBG_OP_VERIFY_AGGREGATE ? (st == TBG_PS_VALID || (SPEC && st == TBG_PS_NOT_VERIFIED))
                                       : (st == TBG_PS_NOT_VERIFIED);
}

// The check side of a TBG_OP_AGGREGATE_VERIFY batch: a TBG_OP_VERIFY batch of its own in
// which duty d is the one candidate d -- the affine aggregate under the duty's group key
// and message.  The aggregates are sums of points that passed the subgroup test and are
// never the identity (TBG_DS_AGG_IDENTITY is decided in the recombination), so the view
// runs no decode and no subgroup test: sgb = 0, hence the classic level 0 (bucket MSM) and
// no by-message merge, which both need the subgroup test's digits.  It shares the batch's
// messages, H(m) and RLC work arrays (sized by duties in tbls_plan.h's section table: the batch itself runs
// no check) and owns partial_status and counters.  Derived from the batch's own fields
// alone: a replayed prefix's view is the prefix's.
inline DevBatch aggver_view(const DevBatch& B) {
  DevBatch V = B;
  V.op = TBG_OP_VERIFY;
  V.n_partials = B.n_duties;
  V.duty_first = V.partial_duty = B.av_iota;
  V.sig_aff = B.agg_aff;
  V.partial_status = B.av_status;
  V.counters = B.av_counters;
  V.rlc_group = B.av_group;
  V.rlc_chunk = B.av_chunk;
  V.rlc_batch = B.av_batch;
  V.sgb = 0;
  V.l0_msg_share = TBG_L0_MSG_NEVER;
  V.agg_aff = nullptr;
  return V;
}
// What a launch's check levels ran on: the view for TBG_OP_AGGREGATE_VERIFY, else the batch.
inline DevBatch checked_batch(const DevBatch& B) { return B.op == TBG_OP_AGGREGATE_VERIFY ? aggver_view(B) : B; }

// Debug aid: with TBG_DEBUG_SYNC=1 in the environment every launch is
// followed by a stream synchronisation and a line on stderr (kernel, ms,
// status), so a faulting or runaway kernel names itself.  Off by default.
void debug_after_launch(const char* kernel, hipStream_t st);
// Per-kernel timing (tbg_replay_profile): while a recorder is active on the
// launching thread every launch is bracketed by a HIP event pair on its own
// stream; otherwise these are a thread-local pointer test.
void kprof_pre(const char* kernel, hipStream_t st);
void kprof_post(hipStream_t st);
#define TBG_KLAUNCH(kernel, grid, block, st, ...)                      \
  do {                                                                \
    kprof_pre(#kernel, st);                                           \
    hipLaunchKernelGGL(kernel, grid, block, 0, st, __VA_ARGS__);      \
    kprof_post(st);                                                   \
    debug_after_launch(#kernel, st);                                  \
  } while (0)

// launchers (asynchronous on `st`)
// Device arrays of one plain-sum call (k_sum.hip): n_sets sets of items,
// summed in chunks of sum_chunk_size() items.
struct SumPlan {
  uint32_t n_sets, n_chunks;
  const uint32_t* off;          // [n_sets + 1] item offsets of the sets
  const uint32_t* chunk_first;  // [n_sets + 1] first chunk of each set
  const uint32_t* chunk_set;    // [n_chunks] set of each chunk
  void* part;                   // [n_chunks] G1J / G2J chunk sums
  int32_t* set_bad;             // [n_sets] zeroed before the launch
};
uint32_t sum_chunk_size();
void launch_sum_g1(const G1A* table, const int32_t* pk_status, uint32_t n_pk, const uint32_t* ids, const SumPlan& p,
                   uint8_t* out48, int32_t* status, hipStream_t st);
void launch_sum_g2(const uint8_t* sigs96, const SumPlan& p, uint8_t* out96, int32_t* status, int32_t* sig_status,
                   hipStream_t st);
void launch_decode_pubkeys(const uint8_t* pk48, uint32_t n, G1A* out, G1A* out_x, int32_t* status, hipStream_t st);
void launch_decode_sigs(const DevBatch& B, hipStream_t st);
// the batched subgroup test (B.sgb): sort, bucket sums, combination checks
void launch_subgroup_batch(const DevBatch& B, hipStream_t st);
void launch_hash_msgs(const DevBatch& B, hipStream_t st);
void launch_hash_clear(const DevBatch& B, hipStream_t st);
void launch_h_lines(const DevBatch& B, hipStream_t st);
// after_keys (optional) is enqueued once the candidates are final (the
// ERR_PUBKEY marks made), before the level-0 bucket MSM: the chain's
// speculative aggregation goes there, off the Miller kernel's critical path
void launch_rlc_prepare(const DevBatch& B, const G1A* pk_aff, const G1A* pk_tab, const int32_t* pk_status,
                        uint32_t n_pk, hipStream_t st, void (*after_keys)(const DevBatch&, hipStream_t) = nullptr);
// pk_tab: for the group levels' G1 products after a void or failed fused level 0
void launch_rlc_check(const DevBatch& B, const G1A* pk_aff, const G1A* pk_tab, const int32_t* pk_status, uint32_t n_pk,
                      hipStream_t st);
void launch_lines_fold(const DevBatch& B, int kind, uint32_t max_entries, hipStream_t st);
// set launches (k_sets.hip): set_status to VALID before the checks; after
// level 1, k_set_resolve in place of k_rlc_resolve_groups; after level 3, the
// sets' statuses and the partial statuses of the failed sets
void launch_set_init(const DevBatch& B, hipStream_t st);
void launch_set_resolve(const DevBatch& B, hipStream_t st);
void launch_set_status(const DevBatch& B, hipStream_t st);
// level 0 (k_msm.hip); with l0_tail(B) a fused launch's key side forms S too (its grid's S role)
void launch_pubkey_tables(const G1A* pk, const G1A* xpk, const int32_t* status, uint32_t n, G1A* tab, hipStream_t st);
void launch_l0_keys(const DevBatch& B, const G1A* pk_tab, const int32_t* pk_status, uint32_t n_pk, hipStream_t st);
void launch_l0_msm(const DevBatch& B, hipStream_t st);
// fused level 0 below l0_tail_partials: S from the subgroup test's sums (k_l0f_reduce, k_l0f_fold, k_l0f_horner)
void launch_l0_fused_s(const DevBatch& B, hipStream_t st);
void launch_l0_check(const DevBatch& B, hipStream_t st);
// level 0's P-chunk and S Miller products on hexads (k_miller_hex.hip)
void launch_l0_miller_hex(const DevBatch& B, hipStream_t st);
// level 0 by message (k_l0msg.hip): the message sums Q_m (after P_d, in
// launch_rlc_prepare), then one hexad per chunk of message slots, the S
// hexad and the fold over the message groups into grp_f (launch_rlc_check);
// l0m_groups: the values the product tree then takes
void launch_l0m_sums(const DevBatch& B, hipStream_t st);
void launch_l0m_miller(const DevBatch& B, hipStream_t st);
inline uint32_t l0m_groups(const DevBatch& B) { return (B.n_msgs + B.rlc_group - 1) / B.rlc_group; }
// level 1's P-chunk and group-S Miller products on hexads (k_miller_hex.hip)
void launch_groups_miller_hex(const DevBatch& B, hipStream_t st);
// after a level-0 failure: the groups' S Miller products only (k_miller_hex.hip)
void launch_group_s_miller_hex(const DevBatch& B, hipStream_t st);
// level 1 by group MSMs (k_gmsm.hip): the G1 products and key marks (no
// level 0), the groups' S in affine form in pend_pts (grp_state GRP_LINES, or
// GRP_FAIL for a degenerate sum), and after the group checks the failed
// groups' r_i s_i (k_pair.hip, list mode) and S_d
void launch_rlc_g1(const DevBatch& B, const G1A* pk_tab, const G1A* pk_aff, const int32_t* pk_status, uint32_t n_pk,
                   hipStream_t st);
void launch_gm_group_s(const DevBatch& B, hipStream_t st);
void launch_gm_failed_partials(const DevBatch& B, const G1A* pk_aff, hipStream_t st);
void launch_rlc_partials_list(const DevBatch& B, const G1A* pk_aff, hipStream_t st);
// spec: the speculative pass (level 0 on, before verification; skipped when
// level 0 already cannot pass); the regular pass then returns at once if
// level 0 passed
void launch_lagrange(const DevBatch& B, hipStream_t st, bool spec = false);
void launch_aggregate(const DevBatch& B, hipStream_t st, bool spec = false);
void launch_aggregate_finish(const DevBatch& B, hipStream_t st, bool spec = false);
// TBG_OP_AGGREGATE_VERIFY (k_aggver.hip; B the batch, V = aggver_view(B)): after the
// recombination, the duties that combined become V's candidates (and V's counters and
// level-0 bucket sizes are zeroed, as k_decode_sigs does at the head of a verify chain);
// after V's checks, their verdicts go into B.duty_status and a failed duty's agg96 is zeroed
void launch_aggver_candidates(const DevBatch& B, const DevBatch& V, hipStream_t st);
void launch_aggver_status(const DevBatch& B, const DevBatch& V, hipStream_t st);
void launch_sk_to_pk(const uint8_t* sk32, uint32_t n, uint8_t* pk48, hipStream_t st);
void launch_sign(const uint8_t* sk32, const uint32_t* item_msg, uint32_t n, const G2A* h_aff, const int32_t* h_status,
                 uint8_t* sig96, hipStream_t st);
// the hardened signer (k_keyed.hip, bls_ctmul.h): the tables of the multiples 0..8 of the
// public base points -- the G1 generator (one table), H(m) of every message -- then the
// fixed-schedule products.  ct_tab_words: 32-bit words of such a table set.
size_t ct_tab_words_g1();
size_t ct_tab_words_g2(uint32_t n_msgs);
void launch_ct_table_g1(uint32_t* tab, hipStream_t st);
void launch_ct_table_g2(const G2A* h_aff, const int32_t* h_status, uint32_t n_msgs, uint32_t* tab, hipStream_t st);
void launch_sk_to_pk_ct(const uint8_t* sk32, uint32_t n, const uint32_t* tab, uint8_t* pk48, int32_t* status,
                        hipStream_t st);
void launch_sign_ct(const uint8_t* sk32, const uint32_t* item_msg, uint32_t n, uint32_t n_msgs, const uint32_t* tab,
                    const int32_t* h_status, uint8_t* sig96, int32_t* status, hipStream_t st);
// Feldman commitment polynomials (k_feldman.hip, bls_feldman.h): evaluation e is polynomial
// eval_poly[e] -- the decoded commitments [poly_first[p], poly_first[p + 1]) of tab[n_commits] -- at eval_id[e]
void launch_fv_eval(const G1A* tab, const int32_t* tab_status, uint32_t n_commits, const uint32_t* poly_first,
                    uint32_t n_polys, const uint32_t* eval_poly, const uint32_t* eval_id, uint32_t n_evals, uint8_t* out48,
                    int32_t* status, hipStream_t st);
// shares on a fixed schedule (k_shares.hip, bls_frct.h).  Split: one lane per (polynomial, identifier
// 1..n_shares) -- the share, the share with a zero replaced by 1 (the ladder's scalar) and a zero flag per
// lane.  Combine: one lane per set -- the interpolation at 0 over all its shares and a zero flag; a set with
// set_ok == 0 is not computed.
void launch_split_ct(const uint8_t* coef32, uint32_t n_coefs, const uint32_t* poly_first, uint32_t n_polys,
                     uint32_t n_shares, uint8_t* share32, uint8_t* ladder32, uint32_t* zero, hipStream_t st);
void launch_combine_ct(const uint8_t* value32, const uint8_t* share_id, uint32_t n_values, const uint32_t* set_first,
                       const uint32_t* set_ok, uint32_t n_sets, uint8_t* secret32, uint32_t* zero, hipStream_t st);

}  // namespace tbg
