// Feldman commitment polynomials evaluated in G1 (tbg_eval_commitments,
// bls_feldman.h): tbls.NewTSS's pubshares from the verifier alone, and the
// right-hand side of Feldman share verification.  Public data throughout.
#include "tbls_launch.h"
#include "bls_feldman.h"
#include "bls_batchinv.h"

namespace tbg {

static_assert(FV_OK == TBG_FV_OK && FV_ID == TBG_FV_ID && FV_COMMIT == TBG_FV_COMMIT &&
                  FV_KEY_IDENTITY == TBG_FV_KEY_IDENTITY && FV_IDENTITY == TBG_FV_IDENTITY,
              "bls_feldman.h restates the TBG_FV_* codes of include/tbls_gpu.h");

// One lane per evaluation.  The lanes of a wave run Horner chains of different
// lengths (t of their polynomial, the bits of their id); nothing inside
// fv_eval is workgroup-wide.  Every thread then meets the batched inversion's
// barriers -- a lane past the end or with a failed evaluation with
// want = false -- so there is no return before it.
__global__ void __launch_bounds__(BINV_BLOCK) k_fv_eval(const G1A* tab, const int32_t* tab_status,
                                                        uint32_t n_commits, const uint32_t* poly_first,
                                                        uint32_t n_polys, const uint32_t* eval_poly,
                                                        const uint32_t* eval_id, uint32_t n_evals, uint8_t* out48,
                                                        int32_t* status) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = e < n_evals;
  G1J acc = jac_inf<Fp>();
  int32_t st = FV_COMMIT;
  if (in) {
    // (tbg_eval_commitments has refused such arrays; checked again here so that no content
    // of theirs can take a read outside the table)
    const uint32_t p = eval_poly[e];
    if (p < n_polys) {
      const uint32_t first = poly_first[p], end = poly_first[p + 1];
      if (first < end && end <= n_commits) st = fv_eval(tab + first, tab_status + first, end - first, eval_id[e], acc);
    }
  }
  G1A a{fp_zero(), fp_zero()};
  const bool aff = block_jac_to_aff<BINV_WAVES>(acc, in && st == FV_OK, a);  // every thread of the workgroup
  if (!in) return;
  uint8_t enc[48];
  if (st == FV_OK || st == FV_IDENTITY) {
    g1_compress(a, !aff, enc);
  } else {
    for (int j = 0; j < 48; ++j) enc[j] = 0;
  }
  for (int j = 0; j < 48; ++j) out48[48ull * e + j] = enc[j];
  status[e] = st;
}

void launch_fv_eval(const G1A* tab, const int32_t* tab_status, uint32_t n_commits, const uint32_t* poly_first,
                    uint32_t n_polys, const uint32_t* eval_poly, const uint32_t* eval_id, uint32_t n_evals, uint8_t* out48,
                    int32_t* status, hipStream_t st) {
  if (n_evals)
    TBG_KLAUNCH(k_fv_eval, dim3((n_evals + BINV_BLOCK - 1) / BINV_BLOCK), dim3(BINV_BLOCK), st, tab, tab_status, n_commits,
                poly_first, n_polys, eval_poly, eval_id, n_evals, out48, status);
}

}  // namespace tbg
