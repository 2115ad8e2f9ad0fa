// TBG_OP_AGGREGATE_VERIFY: the two kernels between a batch's recombination
// (k_aggregate.hip) and the checks of its view (aggver_view, tbls_launch.h), in
// which every duty is one candidate: its affine aggregate under the duty's
// group key and message.  One lane per duty.
#include "tbls_launch.h"

namespace tbg {

// A duty that did not combine is no candidate of the view: its status there is
// none of the TBG_PS_* codes, so no kernel of the check levels lists it, sums it
// or marks it (they all test for TBG_PS_NOT_VERIFIED), and the recombination's
// code stays in duty_status.
constexpr int32_t AV_NOT_A_CANDIDATE = -100;
static_assert(2 * sizeof(DevBatch) <= 4096, "two batch views as kernel arguments");

// After the recombination: the view's candidates.  Also what k_decode_sigs
// does at the head of a chain for the verify side: the view's counters and,
// for the classic level 0, its bucket sizes are zeroed (replays included).
__global__ void TBG_LAUNCH k_aggver_candidates(DevBatch B, DevBatch V) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d < CNT_WORDS) V.counters[d] = 0;
  if (V.rlc_batch && d <= MSM_BUCKETS) V.msm_off[d] = 0;
  if (d >= B.n_duties) return;
  V.partial_status[d] = B.duty_status[d] == TBG_DS_OK ? TBG_PS_NOT_VERIFIED : AV_NOT_A_CANDIDATE;
}

// After the view's checks: their verdicts as duty codes.  A duty whose
// aggregate did not verify gives its 96 bytes back: agg96 is all zero, as for
// a failed combination (agg_status' writer), so that a caller who ignores the
// status finds no unverified aggregate.
__global__ void TBG_LAUNCH k_aggver_status(DevBatch B, DevBatch V) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= B.n_duties) return;
  const int32_t st = V.partial_status[d];
  if (st == AV_NOT_A_CANDIDATE || st == TBG_PS_VALID) return;  // the recombination's code / TBG_DS_OK stands
  // (TBG_PS_NOT_VERIFIED cannot remain after the checks; it fails closed)
  B.duty_status[d] = st == TBG_PS_ERR_PUBKEY ? TBG_DS_AGG_PUBKEY : TBG_DS_AGG_INVALID;
  uint32_t* out = (uint32_t*)(B.agg + 96ull * d);
#pragma unroll
  for (int w = 0; w < 24; ++w) out[w] = 0;
}

void launch_aggver_candidates(const DevBatch& B, const DevBatch& V, hipStream_t st) {
  // at least enough lanes to zero the view's counters (and level 0's bucket sizes)
  uint32_t lanes = B.n_duties > CNT_WORDS ? B.n_duties : CNT_WORDS;
  if (V.rlc_batch && lanes < MSM_BUCKETS + 1) lanes = MSM_BUCKETS + 1;
  TBG_KLAUNCH(k_aggver_candidates, grid_for(lanes), dim3(kBlock), st, B, V);
}
void launch_aggver_status(const DevBatch& B, const DevBatch& V, hipStream_t st) {
  if (B.n_duties) TBG_KLAUNCH(k_aggver_status, grid_for(B.n_duties), dim3(kBlock), st, B, V);
}

}  // namespace tbg
