// The workspace of every call that runs to completion inside itself --
// tbg_sk_to_pk, tbg_sign, their hardened forms, the plain sums,
// tbg_fast_aggregate_verify, tbg_eval_commitments and the two share calls: one struct per call whose
// sections() names every section of the call's single device allocation once, with its element type
// and count, in arena order.  A call that holds secrets names the sections that hold them once more,
// in secrets(): the call's scope zeroes exactly that list before the allocation is released.  The size comes from one walk of it with a null
// base and the pointers from a second walk over the allocation (work_size,
// work_bind), the way for_each_section serves layout and bind for a launch.
// No HIP runtime call in here: tests/plan walks the descriptions on the CPU.
#pragma once
#include "tbls_plan.h"

namespace tbg {

constexpr uint32_t kMaxWorkSections = 32;

// One walk of a description: a bump allocator over Arena whose base may be
// null.  Without a base it only advances the offset; with one it also hands
// out base + offset.  Either way it records where each section lies.
struct WorkWalk {
  uint8_t* base = nullptr;
  Arena arena;
  uint32_t n = 0;
  Section sec[kMaxWorkSections] = {};
  // `count` elements of T, then `pad` more bytes (the paddings that keep an empty section addressable)
  template <class T>
  void operator()(const char* name, T*& p, size_t count, size_t pad = 0) {
    plan_check(n < kMaxWorkSections, "more workspace sections than kMaxWorkSections");
    const size_t bytes = sizeof(T) * count + pad;
    sec[n] = Section{name, ARENA_WORK, arena.take(bytes), bytes};
    if (base) p = (T*)(base + sec[n].off);
    ++n;
  }
  size_t bytes() const { return arena.o; }
};

template <class W>
WorkWalk work_size(W& w) {
  WorkWalk s;
  w.sections(s);
  return s;
}
// The pointers of w over `base`, an allocation of sized.bytes(); the two walks must agree.
template <class W>
void work_bind(W& w, const WorkWalk& sized, uint8_t* base) {
  WorkWalk b;
  b.base = base;
  w.sections(b);
  plan_check(b.n == sized.n, "the binding walk of a workspace visits another number of sections than the sizing walk");
  for (uint32_t i = 0; i < b.n; ++i)
    plan_check(b.sec[i].off == sized.sec[i].off && b.sec[i].bytes == sized.sec[i].bytes,
               "the binding walk of a workspace places a section elsewhere than the sizing walk");
}

// ---- the descriptions: the counts first, then the sections' pointers --------

struct SkToPkWork {  // tbg_sk_to_pk
  size_t n = 0;
  uint8_t *sk = nullptr, *pk = nullptr;
  template <class V>
  void sections(V& v) {
    v("sk", sk, 32 * n);
    v("pk", pk, 48 * n);
  }
};

struct SkToPkCtWork {  // tbg_sk_to_pk_ct
  size_t n = 0, tab_words = 0;  // tab_words: ct_tab_words_g1()
  uint8_t* sk = nullptr;
  uint32_t* tab = nullptr;
  uint8_t* pk = nullptr;
  int32_t* status = nullptr;
  template <class V>
  void sections(V& v) {
    v("sk", sk, 32 * n);
    v("tab", tab, tab_words);
    v("pk", pk, 48 * n);
    v("status", status, n);
  }
  template <class V>
  void secrets(V& v) {
    v("sk", sk, 32 * n);
  }
};

struct SignWork {  // tbg_sign
  size_t n = 0, n_msgs = 0, msg_bytes = 0;
  uint8_t *sk = nullptr, *msgs = nullptr;
  uint32_t *msg_off = nullptr, *item_msg = nullptr;
  G2A* h_aff = nullptr;
  int32_t* h_status = nullptr;
  uint8_t* sig = nullptr;
  G2J* h_jac = nullptr;  // H(m) + the cofactor clearing's two temporaries
  template <class V>
  void sections(V& v) {
    v("sk", sk, 32 * n);
    v("msgs", msgs, msg_bytes + 1);
    v("msg_off", msg_off, n_msgs + 1);
    v("item_msg", item_msg, n);
    v("h_aff", h_aff, n_msgs);
    v("h_status", h_status, n_msgs);
    v("sig", sig, 96 * n);
    v("h_jac", h_jac, 3 * n_msgs);
  }
};

struct SignCtWork : SignWork {  // tbg_sign_ct: tbg_sign's, then the tables and the statuses
  size_t tab_words = 0;         // ct_tab_words_g2(n_msgs)
  uint32_t* tab = nullptr;
  int32_t* status = nullptr;
  template <class V>
  void sections(V& v) {
    SignWork::sections(v);
    v("tab", tab, tab_words);
    v("status", status, n);
  }
  template <class V>
  void secrets(V& v) {
    v("sk", sk, 32 * n);
  }
};

// The device half of a sum plan (SumPlan), the head of the three calls below.
struct SumWork {
  size_t n_sets = 0, n_chunks = 0, part_elem = 0;  // part_elem: sizeof(G1J) or sizeof(G2J)
  uint32_t *off = nullptr, *chunk_first = nullptr, *chunk_set = nullptr;
  uint8_t* part = nullptr;
  int32_t* set_bad = nullptr;
  template <class V>
  void sections(V& v) {
    v("off", off, n_sets + 1);
    v("chunk_first", chunk_first, n_sets + 1);
    v("chunk_set", chunk_set, n_chunks + 1);
    v("part", part, part_elem * n_chunks, 16);
    v("set_bad", set_bad, n_sets + 1);
  }
};

struct SumPubkeysWork : SumWork {  // tbg_sum_pubkeys
  size_t n_items = 0;
  uint32_t* ids = nullptr;
  uint8_t* out = nullptr;
  int32_t* status = nullptr;
  template <class V>
  void sections(V& v) {
    SumWork::sections(v);
    v("ids", ids, n_items + 1);
    v("out", out, 48 * n_sets);
    v("status", status, n_sets);
  }
};

struct SumSigsWork : SumWork {  // tbg_sum_sigs
  size_t n_items = 0;
  uint8_t* sigs = nullptr;
  int32_t* sig_status = nullptr;
  uint8_t* out = nullptr;
  int32_t* status = nullptr;
  template <class V>
  void sections(V& v) {
    SumWork::sections(v);
    v("sigs", sigs, 96 * n_items, 4);
    v("sig_status", sig_status, n_items + 1);
    v("out", out, 96 * n_sets);
    v("status", status, n_sets);
  }
};

// tbg_fast_aggregate_verify: the key sums (n_keys ids in n_sets sets), their
// decoded table, then a TBG_OP_VERIFY batch of one duty, partial and message per set.
struct FastAggVerifyWork : SumWork {
  size_t n_keys = 0, msg_bytes = 0;
  uint32_t* ids = nullptr;
  uint8_t* pk48 = nullptr;
  int32_t* key_status = nullptr;
  G1A *t_pk = nullptr, *t_xpk = nullptr;
  int32_t* t_pk_status = nullptr;
  uint8_t* msgs = nullptr;
  uint32_t *msg_off = nullptr, *iota = nullptr;
  uint8_t *sigs = nullptr, *identifiers = nullptr;
  G2A *sig_aff = nullptr, *h_aff = nullptr;
  int32_t* h_status = nullptr;
  G2J* h_jac = nullptr;
  uint32_t *sig_lines = nullptr, *h_lines = nullptr, *counters = nullptr, *part_list = nullptr;
  int32_t *partial_status = nullptr, *duty_status = nullptr;
  template <class V>
  void sections(V& v) {
    const size_t n = n_sets;
    SumWork::sections(v);
    v("ids", ids, n_keys + 1);
    v("pk48", pk48, 48 * n);
    v("key_status", key_status, n);
    v("t_pk", t_pk, n);
    v("t_xpk", t_xpk, n);
    v("t_pk_status", t_pk_status, n);
    v("msgs", msgs, msg_bytes + 1);
    v("msg_off", msg_off, n + 1);
    v("iota", iota, n + 1);
    v("sigs", sigs, 96 * n);
    v("identifiers", identifiers, n);
    v("sig_aff", sig_aff, n);
    v("h_aff", h_aff, n);
    v("h_status", h_status, n);
    v("h_jac", h_jac, 3 * n);
    v("sig_lines", sig_lines, (size_t)LINES_WORDS * n);
    v("h_lines", h_lines, (size_t)LINES_WORDS * n);
    v("counters", counters, CNT_WORDS);
    v("part_list", part_list, n);
    v("partial_status", partial_status, n);
    v("duty_status", duty_status, n);
  }
};

// tbg_eval_commitments: n_commits Feldman commitments in n_polys polynomials,
// their decoded table (t_xc: the decode kernel's second output, unused
// here), then n_evals evaluations.
struct EvalCommitWork {
  size_t n_commits = 0, n_polys = 0, n_evals = 0;
  uint8_t* commit48 = nullptr;
  uint32_t *poly_first = nullptr, *eval_poly = nullptr, *eval_id = nullptr;
  G1A *t_c = nullptr, *t_xc = nullptr;
  int32_t* commit_status = nullptr;
  uint8_t* out48 = nullptr;
  int32_t* eval_status = nullptr;
  template <class V>
  void sections(V& v) {
    v("commit48", commit48, 48 * n_commits);
    v("poly_first", poly_first, n_polys + 1);
    v("eval_poly", eval_poly, n_evals);
    v("eval_id", eval_id, n_evals);
    v("t_c", t_c, n_commits);
    v("t_xc", t_xc, n_commits);
    v("commit_status", commit_status, n_commits);
    v("out48", out48, 48 * n_evals);
    v("eval_status", eval_status, n_evals);
  }
};

// tbg_split_secret_ct: n_coefs coefficients in n_polys polynomials, n_evals = n_polys * n_shares
// shares.  ks_status: what the two ladder launches write (max(n_coefs, n_evals) words).
struct SplitSecretCtWork {
  size_t n_coefs = 0, n_polys = 0, n_evals = 0, tab_words = 0;  // tab_words: ct_tab_words_g1()
  uint8_t* coef = nullptr;
  uint32_t* poly_first = nullptr;
  uint32_t* tab = nullptr;
  uint8_t *share = nullptr, *ladder = nullptr;
  uint32_t* share_zero = nullptr;
  uint8_t *commit = nullptr, *pubshare = nullptr;
  int32_t* ks_status = nullptr;
  template <class V>
  void sections(V& v) {
    v("coef", coef, 32 * n_coefs);
    v("poly_first", poly_first, n_polys + 1);
    v("tab", tab, tab_words);
    v("share", share, 32 * n_evals);
    v("ladder", ladder, 32 * n_evals);
    v("share_zero", share_zero, n_evals);
    v("commit", commit, 48 * n_coefs);
    v("pubshare", pubshare, 48 * n_evals);
    v("ks_status", ks_status, n_coefs > n_evals ? n_coefs : n_evals);
  }
  template <class V>
  void secrets(V& v) {
    v("coef", coef, 32 * n_coefs);
    v("share", share, 32 * n_evals);
    v("ladder", ladder, 32 * n_evals);
  }
};

// tbg_combine_shares_ct: n_values share values in n_sets sets.
struct CombineSharesCtWork {
  size_t n_values = 0, n_sets = 0;
  uint8_t *value = nullptr, *share_id = nullptr;
  uint32_t *set_first = nullptr, *set_ok = nullptr;
  uint8_t* secret = nullptr;
  uint32_t* secret_zero = nullptr;
  template <class V>
  void sections(V& v) {
    v("value", value, 32 * n_values, 16);
    v("share_id", share_id, n_values, 16);
    v("set_first", set_first, n_sets + 1);
    v("set_ok", set_ok, n_sets);
    v("secret", secret, 32 * n_sets);
    v("secret_zero", secret_zero, n_sets);
  }
  template <class V>
  void secrets(V& v) {
    v("value", value, 32 * n_values);
    v("secret", secret, 32 * n_sets);
  }
};

}  // namespace tbg
