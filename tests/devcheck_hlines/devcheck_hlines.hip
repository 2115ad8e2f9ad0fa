// Device unit harness for the H(m)-lines kernel's body: ONE gfx950 kernel
// around px_h_lines (charon_amd/csrc/bls_pair.h), one lane pair per point,
// exported as plain C for tests/test_gpu_hlines.py.  TEST TOOLING ONLY, in the
// manner of tests/devcheck: never loaded by charon_amd, includes the product
// headers unchanged and is compiled as k_verify.hip compiles that code (the
// unit's flags, TBG_SCHED_FENCE and the launch bounds of the pair kernels).
// Values cross as raw limbs; all Montgomery conversion is Python's.
//
// The entry allocates, copies in (the output buffer too, so the caller's
// sentinel fill shows every word the kernel did not write), launches the
// kernel once, synchronises, copies out, frees and returns the HIP status.
// The status is sticky: after a non-zero one the entry returns it without
// touching the GPU.
#ifndef TBG_SCHED_FENCE
#define TBG_SCHED_FENCE 1
#endif
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include "../../charon_amd/csrc/tbls_launch.h"
#include "../../charon_amd/csrc/bls_lines.h"
#include "../../charon_amd/csrc/bls_pair.h"

using namespace tbg;

namespace {

int g_err = 0;  // sticky HIP status

// q: n affine points (x.c0, x.c1, y.c0, y.c1; NL Montgomery limbs each);
// out: LINES_WORDS words per point.  Lanes of pairs past n return at once.
__global__ void TBG_LAUNCH_N(TBG_PAIR_WAVES) k_hl_lines(const uint32_t* q, uint32_t* out, uint32_t n) {
  const uint32_t pr = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  if (pr >= n) return;
  px_h_lines(px_load(((const G2A*)q)[pr]), out + (size_t)LINES_WORDS * pr);
}

}  // namespace

extern "C" {

int dch_sticky_error(void) { return g_err; }

// the lines of n points into out[0 .. n * LINES_WORDS); out holds out_words >= n * LINES_WORDS words
int dch_lines(const uint32_t* q, uint32_t* out, uint32_t n, uint32_t out_words) {
  if (n == 0 || !q || !out || (size_t)out_words < (size_t)n * LINES_WORDS) return -1;
  if (g_err) return g_err;
  const size_t qb = (size_t)n * 4 * NL * sizeof(uint32_t), ob = (size_t)out_words * sizeof(uint32_t);
  uint32_t *dq = nullptr, *dout = nullptr;
  int err = (int)hipMalloc(&dq, qb);
  if (!err) err = (int)hipMalloc(&dout, ob);
  if (!err) err = (int)hipMemcpy(dq, q, qb, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(dout, out, ob, hipMemcpyHostToDevice);
  if (!err) {
    hipLaunchKernelGGL(k_hl_lines, dim3((2 * n + kBlock - 1) / kBlock), dim3(kBlock), 0, 0, dq, dout, n);
    err = (int)hipGetLastError();
  }
  if (!err) err = (int)hipDeviceSynchronize();
  if (!err) err = (int)hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
  if (!err) {
    (void)hipFree(dq);
    (void)hipFree(dout);
  }
  if (err) g_err = err;  // (after a failure nothing more is asked of the device, frees included)
  return err;
}

}  // extern "C"
