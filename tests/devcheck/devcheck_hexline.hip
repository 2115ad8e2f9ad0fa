// Device unit harness for the hexad's line steps: ONE gfx950 kernel around
// hex_line_at_v / hex_line_folded (charon_amd/csrc/bls_hex.h), one hexad per
// slot, exported as plain C for tests/test_gpu_hex_line_direct.py.  TEST
// TOOLING ONLY, in the manner of devcheck.hip: never loaded by charon_amd,
// includes the product headers unchanged and is compiled as k_miller_hex.hip
// compiles that code (the unit's flags, TBG_SCHED_FENCE and the launch bounds
// of the hexad kernels); built into a library of its own by
// tests/devcheck_hexline.  Values cross as raw limbs; all Montgomery
// conversion is Python's.
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
#include "../../charon_amd/csrc/bls_hex.h"

using namespace tbg;

namespace {

int g_err = 0;  // sticky HIP status

constexpr int HEX_WORDS = 12 * NL;  // quad layout: 3 trio lanes x [a.c0, a.c1, b.c0, b.c1]

// f: n elements (HEX_WORDS each); lines: one line per slot (LINE_WORDS: l0, l1,
// l4); pts: (-x, y) per slot (2 NL words), read by the unevaluated step only.
// Lane 15 of a row and the lanes of slots past n return at once.
template <bool FOLDED>
__global__ void __launch_bounds__(64, TBG_HEX_WAVES) k_hexline(const uint32_t* f, const uint32_t* lines,
                                                               const uint32_t* pts, uint32_t* out, uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t s = hex_slot(t);
  if (s == 0xFFFFFFFFu || s >= n) return;
  const Fp4h A = hex_load(f + (size_t)HEX_WORDS * s);
  Fp4h R;
  if constexpr (FOLDED) R = hex_line_folded(A, lines + (size_t)LINE_WORDS * s, 0);
  else R = hex_line_at_v(A, lines + (size_t)LINE_WORDS * s, 0, hex_line_operand(((const G1A*)pts)[s]));
  hex_store(out + (size_t)HEX_WORDS * s, R);
}

}  // namespace

extern "C" {

int dcx_sticky_error(void) { return g_err; }

// one line step per slot: out[s] = f[s] * line[s]; out holds cap >= n slots
int dcx_hex_line(int folded, const uint32_t* f, const uint32_t* lines, const uint32_t* pts, uint32_t* out, uint32_t n,
                 uint32_t cap) {
  if (n == 0 || cap < n || !f || !lines || !out || (!folded && !pts)) return -1;
  if (g_err) return g_err;
  const size_t fb = (size_t)n * HEX_WORDS * 4, lb = (size_t)n * LINE_WORDS * 4, pb = (size_t)n * 2 * NL * 4,
               ob = (size_t)cap * HEX_WORDS * 4;
  uint32_t *df = nullptr, *dl = nullptr, *dp = nullptr, *dout = nullptr;
  int err = (int)hipMalloc(&df, fb);
  if (!err) err = (int)hipMalloc(&dl, lb);
  if (!err) err = (int)hipMalloc(&dp, pb);
  if (!err) err = (int)hipMalloc(&dout, ob);
  if (!err) err = (int)hipMemcpy(df, f, fb, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(dl, lines, lb, hipMemcpyHostToDevice);
  if (!err && pts) err = (int)hipMemcpy(dp, pts, pb, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(dout, out, ob, hipMemcpyHostToDevice);
  if (!err) {
    const dim3 grid(hex_threads(n) / 64), block(64);
    if (folded) hipLaunchKernelGGL(k_hexline<true>, grid, block, 0, 0, df, dl, dp, dout, n);
    else hipLaunchKernelGGL(k_hexline<false>, grid, block, 0, 0, df, dl, dp, dout, n);
    err = (int)hipGetLastError();
  }
  if (!err) err = (int)hipDeviceSynchronize();
  if (!err) err = (int)hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
  if (!err) {
    (void)hipFree(df);
    (void)hipFree(dl);
    (void)hipFree(dp);
    (void)hipFree(dout);
  }
  if (err) g_err = err;  // (after a failure nothing more is asked of the device, frees included)
  return err;
}

}  // extern "C"
