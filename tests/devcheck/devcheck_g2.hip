// Device unit harness for the lane-pair G2 group law (bls_pair.h, bls_sgb.h):
// the second source of tests/devcheck, compiled as k_sgb.hip compiles that
// code (the two defines below, set before the includes).  TEST TOOLING ONLY.
//
// One lane pair per item, 64-thread blocks: the additions without a doubling
// branch, the complete ones, psi, [|x|] P, the subgroup test, cofactor
// clearing and the batched subgroup test's fold / running sums run on real
// lanes, where the DPP exchanges sit inside branches that neighbouring pairs
// of one wave take differently.  Values cross as raw limbs: an Fp2 is 2 x 14
// words, an affine point 4 x 14, a Jacobian point 6 x 14.
//
// As devcheck.hip: the entry allocates, copies in, launches ONE kernel,
// synchronises, copies out and frees; the HIP status is sticky; the output
// buffers are copied in as well, so a sentinel shows every unwritten word.
#define TBG_ADD_DBL_INLINE 1
#define TBG_SCHED_FENCE 1
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include "../../charon_amd/csrc/bls_sgb.h"

using namespace tbg;

namespace {

int g_err = 0;  // sticky HIP status (this source's own)

enum {
  G2_ADD_X, G2_ADD_AFF_X, G2_DBL_LO, G2_ADD_IN, G2_ADD_AFF_IN, G2_PSI, G2_MUL_XABS_X, G2_MUL_XABS_AFF_X,
  G2_IN_SUBGROUP_AFF, G2_CLEAR_COFACTOR, G2_SGB_SUMS, G2_SGB_SUMS_COMPLETE, G2_SGB_FOLD, G2_SGB_FOLD_COMPLETE, G2_NOPS
};
constexpr uint32_t FP2_W = 2 * NL, AFF_W = 4 * NL, JAC_W = 6 * NL;
constexpr uint32_t G2_SUM_V = 6;     // buckets of one combination (SGB_V)
constexpr uint32_t G2_FOLD_S = 4;    // slices of one bucket (SGB_SPLIT)

// words of operand a / b per item
__host__ __device__ constexpr uint32_t g2_a_words(int op) {
  return (op == G2_MUL_XABS_AFF_X || op == G2_IN_SUBGROUP_AFF) ? AFF_W
         : (op == G2_SGB_SUMS || op == G2_SGB_SUMS_COMPLETE)   ? G2_SUM_V * JAC_W
         : (op == G2_SGB_FOLD || op == G2_SGB_FOLD_COMPLETE)   ? G2_FOLD_S * JAC_W
                                                               : JAC_W;
}
__host__ __device__ constexpr uint32_t g2_b_words(int op) {
  return (op == G2_ADD_X || op == G2_ADD_IN) ? JAC_W : (op == G2_ADD_AFF_X || op == G2_ADD_AFF_IN) ? AFF_W : 0u;
}

// out: one Jacobian point per item (G2_IN_SUBGROUP_AFF writes none); flags:
// one word per LANE, bit 0 `exc`, bit 1 the subgroup test's verdict
template <int OP>
__global__ void __launch_bounds__(64) k_g2(const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* flags,
                                           uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, pr = t >> 1;
  if (pr >= n) return;
  const uint32_t* pa = a + (size_t)g2_a_words(OP) * pr;
  const uint32_t* pb = b + (size_t)g2_b_words(OP) * pr;
  bool exc = false, verdict = false;
  Jac<Fp2x> r = jac_inf<Fp2x>();
  if constexpr (OP == G2_ADD_X) r = jac_add_x(px_load(*(const G2J*)pa), px_load(*(const G2J*)pb), exc);
  else if constexpr (OP == G2_ADD_AFF_X) r = jac_add_aff_x(px_load(*(const G2J*)pa), px_load(*(const G2A*)pb), exc);
  else if constexpr (OP == G2_DBL_LO) r = jac_dbl_lo(px_load(*(const G2J*)pa));
  else if constexpr (OP == G2_ADD_IN) r = jac_add_in<Fp2x, true>(px_load(*(const G2J*)pa), px_load(*(const G2J*)pb));
  else if constexpr (OP == G2_ADD_AFF_IN) r = jac_add_aff_in(px_load(*(const G2J*)pa), px_load(*(const G2A*)pb));
  else if constexpr (OP == G2_PSI) r = g2_psi_g(px_load(*(const G2J*)pa));
  else if constexpr (OP == G2_MUL_XABS_X) r = jac_mul_xabs_x(px_load(*(const G2J*)pa), exc);
  else if constexpr (OP == G2_MUL_XABS_AFF_X) r = jac_mul_xabs_aff_x(px_load(*(const G2A*)pa), exc);
  else if constexpr (OP == G2_IN_SUBGROUP_AFF) verdict = g2_in_subgroup_aff_g(px_load(*(const G2A*)pa), exc);
  else if constexpr (OP == G2_CLEAR_COFACTOR) r = g2_clear_cofactor_g(px_load(*(const G2J*)pa), exc);
  else if constexpr (OP == G2_SGB_SUMS || OP == G2_SGB_SUMS_COMPLETE)
    r = sgb_running_sums_g<Fp2x, OP == G2_SGB_SUMS>([&](uint32_t v) { return px_load(((const G2J*)pa)[v]); },
                                                    G2_SUM_V, exc);
  else
    r = sgb_fold_g<Fp2x, OP == G2_SGB_FOLD>([&](uint32_t sl) { return px_load(((const G2J*)pa)[sl]); }, G2_FOLD_S,
                                            exc);
  flags[t] = (exc ? 1u : 0u) | (verdict ? 2u : 0u);
  if constexpr (OP != G2_IN_SUBGROUP_AFF) px_store(((G2J*)out)[pr], r);
}

}  // namespace

extern "C" {

int dc_sticky_error(void);  // devcheck.hip's status: after a failure there, nothing runs here either
int dc_g2_sticky_error(void) { return g_err; }
int dc_g2_a_words(int op) { return op < 0 || op >= G2_NOPS ? -1 : (int)g2_a_words(op); }
int dc_g2_b_words(int op) { return op < 0 || op >= G2_NOPS ? -1 : (int)g2_b_words(op); }

#define DC_G2_CASE(OP) \
  case OP: hipLaunchKernelGGL(k_g2<OP>, grid, block, 0, 0, da, db, dout, dflags, n); break;

// n items; out `cap` Jacobian points, flags 2 `cap` words (cap >= n: the words
// past item n must come back untouched)
int dc_g2(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* flags, uint32_t n, uint32_t cap) {
  if (op < 0 || op >= G2_NOPS || n == 0 || cap < n || !a || !out || !flags) return -1;
  if (g2_b_words(op) && !b) return -1;
  if (g_err) return g_err;
  if (dc_sticky_error()) return dc_sticky_error();
  const uint32_t *da = nullptr, *db = nullptr;
  uint32_t *dout = nullptr, *dflags = nullptr;
  const size_t wa = (size_t)n * g2_a_words(op) * 4, wb = (size_t)n * g2_b_words(op) * 4;
  const size_t wo = (size_t)cap * JAC_W * 4, wf = (size_t)cap * 2 * 4;
  int err = (int)hipMalloc((void**)&da, wa);
  if (!err) err = (int)hipMalloc((void**)&db, wb ? wb : 4);
  if (!err) err = (int)hipMalloc((void**)&dout, wo);
  if (!err) err = (int)hipMalloc((void**)&dflags, wf);
  if (!err) err = (int)hipMemcpy((void*)da, a, wa, hipMemcpyHostToDevice);
  if (!err && wb) err = (int)hipMemcpy((void*)db, b, wb, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(dout, out, wo, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(dflags, flags, wf, hipMemcpyHostToDevice);
  const dim3 grid((2 * n + 63) / 64), block(64);
  if (!err) switch (op) {
    DC_G2_CASE(G2_ADD_X) DC_G2_CASE(G2_ADD_AFF_X) DC_G2_CASE(G2_DBL_LO) DC_G2_CASE(G2_ADD_IN)
    DC_G2_CASE(G2_ADD_AFF_IN) DC_G2_CASE(G2_PSI) DC_G2_CASE(G2_MUL_XABS_X) DC_G2_CASE(G2_MUL_XABS_AFF_X)
    DC_G2_CASE(G2_IN_SUBGROUP_AFF) DC_G2_CASE(G2_CLEAR_COFACTOR) DC_G2_CASE(G2_SGB_SUMS)
    DC_G2_CASE(G2_SGB_SUMS_COMPLETE) DC_G2_CASE(G2_SGB_FOLD) DC_G2_CASE(G2_SGB_FOLD_COMPLETE)
  }
  if (!err) err = (int)hipGetLastError();
  if (!err) err = (int)hipDeviceSynchronize();
  if (!err) err = (int)hipMemcpy(out, dout, wo, hipMemcpyDeviceToHost);
  if (!err) err = (int)hipMemcpy(flags, dflags, wf, hipMemcpyDeviceToHost);
  if (!err) {
    (void)hipFree((void*)da);
    (void)hipFree((void*)db);
    (void)hipFree(dout);
    (void)hipFree(dflags);
  } else {
    g_err = err;  // (after a failure nothing more is asked of the device, frees included)
  }
  return err;
}

}  // extern "C"
