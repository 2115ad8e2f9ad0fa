// All-or-nothing verification of SETS of duties (tbg_submit_sets): per set,
// whether every member verifies -- the meaning of parsigex's receive path,
// which drops a peer's whole set on its first failing partial (reference
// core/parsigex/parsigex.go:101-107; validatorapi's submitters abort a batch
// likewise, core/validatorapi/validatorapi.go:228-287).
//
// A set launch runs the chain of k_rlc.hip up to the group checks (level 0,
// then level 1 after a void or failed level 0) and stops narrowing there: a
// failed group fails its set.  The host packs every set onto a multiple of
// the group size (empty padding duties), so a group lies inside one set and
// a clean set beside a bad one stays VALID; the group lead's r = 1 stays one
// per group, so errors cannot cancel across groups or sets.  Only what the
// chain sends to the exact per-partial level for exactness still goes there
// (a duty whose combination is degenerate, a group whose sum is, every
// partial under TBG_VERIFY_EACH).
//
//   k_set_init     set_status = VALID, the tail counters 0
//   k_set_resolve  one lane per duty, after k_rlc_group_final (in place of
//                  k_rlc_resolve_groups): accept, fail the set, or level 3
//   k_set_status   one lane per partial, after level 3: the member's code
//                  reduced into its set's status (atomicMin: ERROR < INVALID
//                  < VALID)
//   k_set_finish   one lane per partial: the candidates of the sets that are
//                  not VALID back to NOT_VERIFIED
// These sit on every set launch's serial tail: a clean launch issues no
// atomic (VALID is the initial value) and k_set_finish returns at once.
#include "tbls_launch.h"

namespace tbg {

__global__ void TBG_LAUNCH k_set_init(DevBatch B) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < B.n_sets) B.set_status[k] = TBG_SS_VALID;
  else if (k < B.n_sets + SET_TAIL) B.set_status[k] = 0;
}

__device__ __forceinline__ void set_push_partials(const DevBatch& B, uint32_t d) {
  for (uint32_t i = B.duty_first[d]; i < B.duty_first[d + 1]; ++i)
    if (B.partial_status[i] == TBG_PS_NOT_VERIFIED) B.part_list[atomicAdd(&B.counters[CNT_PARTIALS], 1u)] = i;
}

// After level 1 (one lane per duty).  The candidates of a failed group, and of
// a duty whose H(m) is unusable, stay NOT_VERIFIED: k_set_status reads that as
// a false pairing check.
__global__ void TBG_LAUNCH k_set_resolve(DevBatch B) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= B.n_duties) return;
  const int32_t st = B.dv_state[d];
  if (st == RLC_NONE) return;  // (padding duties, duties without a candidate)
  if (st == RLC_EACH) { set_push_partials(B, d); return; }
  if (B.h_status[B.duty_msg[d]] != 0) { atomicMin(&B.set_status[B.duty_set[d]], (int32_t)TBG_SS_INVALID); return; }
  const int32_t gs = B.grp_state[d / B.rlc_group];
  if (gs == GRP_OK) {
    for (uint32_t i = B.duty_first[d]; i < B.duty_first[d + 1]; ++i)
      if (B.partial_status[i] == TBG_PS_NOT_VERIFIED) B.partial_status[i] = TBG_PS_VALID;
    return;
  }
  if (gs == GRP_FAIL) { set_push_partials(B, d); return; }  // a degenerate group sum: the exact check decides
  atomicMin(&B.set_status[B.duty_set[d]], (int32_t)TBG_SS_INVALID);  // GRP_BAD
}

// After level 3 (one lane per partial, one wave per workgroup).  A wave whose
// members are all VALID has nothing to do; a wave inside one set (the common
// case: a peer set is thousands of items) reduces over its lanes and issues
// one atomicMin, a wave across a boundary one per lane with a failing code.
__global__ void __launch_bounds__(kBlock) k_set_status(DevBatch B) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < B.n_partials;
  int32_t code = TBG_SS_VALID;
  uint32_t set = 0;
  bool bad = false;
  if (in) {
    const int32_t st = B.partial_status[i];
    bad = st == TBG_PS_INVALID || st == TBG_PS_NOT_VERIFIED;
    code = st < 0 ? TBG_SS_ERROR : bad ? TBG_SS_INVALID : TBG_SS_VALID;
    set = B.duty_set[B.partial_duty[i]];
  }
  const uint64_t any = __ballot(code != TBG_SS_VALID);
  if (any == 0) return;  // (wave-uniform)
  const uint64_t nb = __ballot(bad);
  const uint32_t lane = threadIdx.x & 63u;
  if (lane == 0) {
    atomicAdd((uint32_t*)&B.set_status[B.n_sets + SET_ANY], (uint32_t)__popcll(any));
    if (nb) atomicAdd((uint32_t*)&B.set_status[B.n_sets + SET_BAD], (uint32_t)__popcll(nb));
  }
  const uint32_t set0 = (uint32_t)__shfl((int)set, 0);  // (lane 0 is in range whenever a lane is)
  if (__all(!in || set == set0)) {
    for (int m = 32; m >= 1; m >>= 1) code = min(code, __shfl_xor(code, m));
    if (lane == 0) atomicMin(&B.set_status[set0], code);
  } else if (code != TBG_SS_VALID) {
    atomicMin(&B.set_status[set], code);
  }
}

// The second pass: in a set that is not VALID no candidate keeps a verdict.
__global__ void __launch_bounds__(kBlock) k_set_finish(DevBatch B) {
  if (B.set_status[B.n_sets + SET_ANY] == 0) return;  // every member VALID (grid-uniform)
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B.n_partials) return;
  const int32_t st = B.partial_status[i];
  if ((st == TBG_PS_VALID || st == TBG_PS_INVALID) && B.set_status[B.duty_set[B.partial_duty[i]]] != TBG_SS_VALID)
    B.partial_status[i] = TBG_PS_NOT_VERIFIED;
}

void launch_set_init(const DevBatch& B, hipStream_t st) {
  TBG_KLAUNCH(k_set_init, grid_for(B.n_sets + SET_TAIL), dim3(kBlock), st, B);
}

void launch_set_resolve(const DevBatch& B, hipStream_t st) {
  TBG_KLAUNCH(k_set_resolve, grid_for(B.n_duties), dim3(kBlock), st, B);
}

void launch_set_status(const DevBatch& B, hipStream_t st) {
  if (!B.n_partials) return;
  TBG_KLAUNCH(k_set_status, grid_for(B.n_partials), dim3(kBlock), st, B);
  TBG_KLAUNCH(k_set_finish, grid_for(B.n_partials), dim3(kBlock), st, B);
}

}  // namespace tbg
