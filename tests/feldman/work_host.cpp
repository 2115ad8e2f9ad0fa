// TEST TOOLING ONLY: the workspace of tbg_eval_commitments (EvalCommitWork,
// charon_amd/csrc/tbls_work.h) walked on the CPU for tests/test_feldman_abi.py,
// the way tests/plan walks the other one-shot calls' workspaces.  Plain host
// C++: the headers make no HIP runtime call.
#include <cstdint>
#include "../../charon_amd/csrc/tbls_work.h"

using namespace tbg;

extern "C" {

uint32_t fvw_max_sections() { return kMaxWorkSections; }

// EvalCommitWork as the engine makes it: work_size, then work_bind over `base` (0: the sizing walk alone).
// secs[n][2]: offset, bytes of the sizing walk; ptrs[n]: the description's pointers after the binding walk,
// in section order; *total: the allocation's bytes.  Returns the section count.
int fvw_work(uint64_t n_commits, uint64_t n_polys, uint64_t n_evals, uint64_t base, uint64_t* total, uint64_t* secs,
             uint64_t* ptrs, const char** names) {
  EvalCommitWork w;
  w.n_commits = n_commits;
  w.n_polys = n_polys;
  w.n_evals = n_evals;
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
}

}  // extern "C"
