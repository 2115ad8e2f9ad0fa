// TEST TOOLING ONLY: the workspaces of tbg_split_secret_ct and
// tbg_combine_shares_ct (SplitSecretCtWork, CombineSharesCtWork,
// charon_amd/csrc/tbls_work.h) walked on the CPU for tests/test_shares_abi.py,
// the way tests/feldman walks tbg_eval_commitments' -- and their secrets()
// lists, the sections the call's scope zeroes.  Plain host C++: the headers
// make no HIP runtime call.
#include <cstdint>
#include "../../charon_amd/csrc/tbls_work.h"

using namespace tbg;

namespace {

template <class W>
int walk(W& w, uint64_t base, uint64_t* total, uint64_t* secs, uint64_t* ptrs, const char** names, uint64_t* secret,
         const char** secret_names, uint32_t* n_secret) {
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
  // the secret list as the engine's scope takes it: name, pointer, bytes
  uint32_t k = 0;
  auto take = [&](const char* name, uint8_t*& p, size_t count, size_t = 0) {
    secret_names[k] = name;
    secret[2 * k] = (uint64_t)(uintptr_t)p;
    secret[2 * k + 1] = count;
    ++k;
  };
  w.secrets(take);
  *n_secret = k;
  return (int)sized.n;
}

}  // namespace

extern "C" {

uint32_t shw_max_sections() { return kMaxWorkSections; }

// The description as the engine makes it: work_size, then work_bind over `base` (0: the sizing walk alone).
// secs[n][2]: offset, bytes of the sizing walk; ptrs[n]: the pointers after the binding walk; secret[k][2]:
// pointer, bytes of each section secrets() names.  Returns the section count.
int shw_split(uint64_t n_coefs, uint64_t n_polys, uint64_t n_evals, uint64_t tab_words, uint64_t base, uint64_t* total,
              uint64_t* secs, uint64_t* ptrs, const char** names, uint64_t* secret, const char** secret_names,
              uint32_t* n_secret) {
  SplitSecretCtWork w;
  w.n_coefs = n_coefs;
  w.n_polys = n_polys;
  w.n_evals = n_evals;
  w.tab_words = tab_words;
  return walk(w, base, total, secs, ptrs, names, secret, secret_names, n_secret);
}

int shw_combine(uint64_t n_values, uint64_t n_sets, uint64_t base, uint64_t* total, uint64_t* secs, uint64_t* ptrs,
                const char** names, uint64_t* secret, const char** secret_names, uint32_t* n_secret) {
  CombineSharesCtWork w;
  w.n_values = n_values;
  w.n_sets = n_sets;
  return walk(w, base, total, secs, ptrs, names, secret, secret_names, n_secret);
}

// the hardened signer's two descriptions name their keys the same way (KeyedScope wipes what secrets() names)
int shw_keyed_secret(int sign, uint64_t n, uint64_t base, uint64_t* secret, const char** secret_names) {
  uint64_t total, secs[2 * kMaxWorkSections], ptrs[kMaxWorkSections];
  const char* names[kMaxWorkSections];
  uint32_t k = 0;
  if (sign) {
    SignCtWork w;
    w.n = n;
    w.n_msgs = 1;
    walk(w, base, &total, secs, ptrs, names, secret, secret_names, &k);
  } else {
    SkToPkCtWork w;
    w.n = n;
    walk(w, base, &total, secs, ptrs, names, secret, secret_names, &k);
  }
  return (int)k;
}

}  // extern "C"
