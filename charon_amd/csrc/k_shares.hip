#include "tbls_launch.h"
#include "bls_frct.h"

namespace tbg {

// ---- shares on a fixed schedule (tbg_split_secret_ct / tbg_combine_shares_ct,
// include/tbls_gpu.h): tbls.SplitSecret, GenerateTSS and CombineShares
// (reference tbls/tss.go:256-290, :120-139, :220-253; their callers
// cmd/createcluster.go:250-270, dkg/keycast.go:164-186). ----
// Every secret value -- a polynomial's coefficients, a share, a combined
// secret -- goes through bls_frct.h alone: no branch, loop bound or address
// below depends on one.  What does vary from lane to lane is public: the
// lane's index, its polynomial's threshold, its identifier, a set's size and
// identifiers, and whether the host has refused the set.  The host has
// replaced every coefficient and share value outside (0, r) by 1
// (tbls_engine.hip), so frct_from_be32's precondition holds.
namespace {

using FrS = FrCt<uint32_t>;

TBG_HD void shares_load_be32(const uint8_t* p, uint32_t (&b)[32]) {
#pragma unroll
  for (int j = 0; j < 32; ++j) b[j] = p[j];
}
TBG_HD void shares_store_be32(uint8_t* p, const uint32_t (&b)[32]) {
#pragma unroll
  for (int j = 0; j < 32; ++j) p[j] = (uint8_t)b[j];
}
TBG_HD void shares_store_zero(uint8_t* p) {
#pragma unroll
  for (int j = 0; j < 32; ++j) p[j] = 0;
}

// One lane per (polynomial p, identifier i = 1..n_shares): lane e = p n_shares + i - 1.
//   share32[e]  f_p(i), 32 bytes big-endian
//   ladder32[e] the same with a zero replaced by 1 (what the fixed-schedule ladder may take)
//   zero[e]     1 iff f_p(i) == 0, a data word: the host decides TBG_SH_SHARE_ZERO from it
// Lanes of one wave may run different trip counts (t is public).
__global__ void __launch_bounds__(64) k_split_ct(const uint8_t* coef32, uint32_t n_coefs, const uint32_t* poly_first,
                                                  uint32_t n_polys, uint32_t n_shares, uint8_t* share32, uint8_t* ladder32,
                                                  uint32_t* zero) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (n_shares == 0 || e / n_shares >= n_polys) return;
  const uint32_t p = e / n_shares, id = e % n_shares + 1;
  const uint32_t first = poly_first[p], last = poly_first[p + 1];
  // (tbg_split_secret_ct has refused such arrays; checked again here so that no content of
  // poly_first can take a read outside coef32)
  if (first >= last || last > n_coefs || last - first > 255u) {
    shares_store_zero(share32 + 32ull * e);
    shares_store_zero(ladder32 + 32ull * e);
    zero[e] = 0;
    return;
  }
  const FrS s = frct_horner<uint32_t>(fr_from_u32(id), last - first, [&](uint32_t j, uint32_t (&b)[32]) {
    shares_load_be32(coef32 + 32ull * (first + j), b);
  });
  const uint32_t zm = frct_zero_mask(s);
  const FrS one = frct_pub<uint32_t>(fr_from_limbs(R_ONE_M));
  uint32_t b[32];
  frct_to_be32(s, b);
  shares_store_be32(share32 + 32ull * e, b);
  frct_to_be32(frct_select(zm, one, s), b);
  shares_store_be32(ladder32 + 32ull * e, b);
  zero[e] = zm & 1u;
}

// One lane per set k: secret = sum_i lambda_i(0) s_i mod r over ALL the set's shares.  The
// lambda_i are public (bls_fr.h); the products with s_i and the sum are bls_frct.h's.
//   secret32[k] the sum, 32 bytes big-endian
//   zero[k]     1 iff the sum is 0
// A set the host has refused (set_ok[k] == 0: public reasons, or a value it replaced) is not
// computed: zero bytes, zero[k] = 0.
__global__ void __launch_bounds__(64) k_combine_ct(const uint8_t* value32, const uint8_t* share_id, uint32_t n_values,
                                                    const uint32_t* set_first, const uint32_t* set_ok, uint32_t n_sets,
                                                    uint8_t* secret32, uint32_t* zero) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_sets) return;
  const uint32_t first = set_first[k], last = set_first[k + 1];
  // (an accepted set has 2..255 distinct identifiers; checked again so that no content of
  // set_first can take a read outside the arrays or a loop beyond 255^2 steps)
  if (!set_ok[k] || first >= last || last > n_values || last - first > 255u) {
    shares_store_zero(secret32 + 32ull * k);
    zero[k] = 0;
    return;
  }
  const FrS acc = frct_interpolate_at_zero<uint32_t>(share_id + first, last - first, [&](uint32_t i, uint32_t (&b)[32]) {
    shares_load_be32(value32 + 32ull * (first + i), b);
  });
  uint32_t b[32];
  frct_to_be32(acc, b);
  shares_store_be32(secret32 + 32ull * k, b);
  zero[k] = frct_zero_mask(acc) & 1u;
}

}  // namespace

void launch_split_ct(const uint8_t* coef32, uint32_t n_coefs, const uint32_t* poly_first, uint32_t n_polys,
                     uint32_t n_shares, uint8_t* share32, uint8_t* ladder32, uint32_t* zero, hipStream_t st) {
  const uint32_t n = n_polys * n_shares;
  if (n)
    TBG_KLAUNCH(k_split_ct, grid_for(n), dim3(kBlock), st, coef32, n_coefs, poly_first, n_polys, n_shares, share32,
                ladder32, zero);
}
void launch_combine_ct(const uint8_t* value32, const uint8_t* share_id, uint32_t n_values, const uint32_t* set_first,
                       const uint32_t* set_ok, uint32_t n_sets, uint8_t* secret32, uint32_t* zero, hipStream_t st) {
  if (n_sets)
    TBG_KLAUNCH(k_combine_ct, grid_for(n_sets), dim3(kBlock), st, value32, share_id, n_values, set_first, set_ok, n_sets,
                secret32, zero);
}

}  // namespace tbg
