// Device unit harness for the lane-cooperative field arithmetic: thin gfx950
// kernels around the product headers' device functions, exported as plain C
// for tests/test_gpu_devcheck.py.  TEST TOOLING ONLY -- the GPU twin of
// tests/hostcheck: never loaded by charon_amd, includes the product headers
// unchanged, and runs each primitive on real lanes (the ds_swizzle / DPP /
// shuffle bodies the host build cannot reach) with the operands the test
// chose.  Values cross as raw limbs (14 uint32 plain, 14 int32 row form);
// all Montgomery conversion is Python's.
//
// Every entry allocates, copies in, launches ONE kernel, synchronises, copies
// out and frees, and returns the HIP status.  The status is sticky: after a
// non-zero one every later entry returns it without touching the GPU.
// Output buffers are copied IN as well, so the caller's sentinel fill shows
// every word a kernel did not write.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include "../../charon_amd/csrc/bls_pairing.h"
#include "../../charon_amd/csrc/bls_hex.h"
#include "../../charon_amd/csrc/bls_pair.h"
#include "../../charon_amd/csrc/bls_batchinv.h"
#include "../../charon_amd/csrc/bls_row.h"
#include "../../charon_amd/csrc/bls_lines.h"

using namespace tbg;

namespace {

int g_err = 0;  // sticky HIP status

struct Run {
  static constexpr int MAXB = 10;
  void* dev[MAXB];
  void* host[MAXB];
  size_t len[MAXB];
  bool back[MAXB];
  int nb = 0;
  int err;
  Run() : err(g_err) {}
  void* add(const void* h, size_t bytes, bool out) {
    if (err || !h || nb >= MAXB) return nullptr;
    void* d = nullptr;
    err = (int)hipMalloc(&d, bytes ? bytes : 4);
    if (err) return nullptr;
    dev[nb] = d;
    host[nb] = const_cast<void*>(h);
    len[nb] = bytes;
    back[nb] = out;
    ++nb;
    if (bytes) err = (int)hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
    return d;
  }
  template <class T> const T* in(const T* h, size_t count) { return (const T*)add(h, count * sizeof(T), false); }
  template <class T> T* io(T* h, size_t count) { return (T*)add(h, count * sizeof(T), true); }
  bool ok() const { return err == 0; }
  int finish() {
    if (!err) err = (int)hipGetLastError();
    if (!err) err = (int)hipDeviceSynchronize();
    for (int i = 0; i < nb; ++i)
      if (!err && back[i] && len[i]) err = (int)hipMemcpy(host[i], dev[i], len[i], hipMemcpyDeviceToHost);
    if (!err)
      for (int i = 0; i < nb; ++i) (void)hipFree(dev[i]);
    if (err) g_err = err;  // (after a failure nothing more is asked of the device, frees included)
    return err;
  }
};

__device__ __forceinline__ Fp ld_fp(const uint32_t* p) {
  Fp r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = p[i];
  return r;
}
__device__ __forceinline__ void st_fp(uint32_t* p, const Fp& a) {
#pragma unroll
  for (int i = 0; i < NL; ++i) p[i] = a.l[i];
}

// ---------------------------------------------------------------------------
// lane-private Fp (bls_field.h): one operand tuple per thread
enum {
  FP_MUL, FP_MUL2, FP_SQR, FP_ADD, FP_SUB, FP_ADDL_MUL, FP_SUBL_MUL, FP_NEG, FP_NEGL_MUL, FP_MUL_SMALL, FP_REDUCE,
  FP_CANON, FP_INV, FP_INV_FERMAT, FP_FROM_SIGNED, FP_LEX, FP_NOPS
};
template <int OP>
__global__ void __launch_bounds__(64) k_fp(const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
                                           uint32_t k, uint32_t* out, uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const size_t o = (size_t)t * NL;
  Fp r;
  if constexpr (OP == FP_MUL) r = fp_mul(ld_fp(a + o), ld_fp(b + o));
  else if constexpr (OP == FP_MUL2) r = fp_mul2(ld_fp(a + o), ld_fp(b + o), ld_fp(c + o), ld_fp(d + o));
  else if constexpr (OP == FP_SQR) r = fp_sqr(ld_fp(a + o));
  else if constexpr (OP == FP_ADD) r = fp_add(ld_fp(a + o), ld_fp(b + o));
  else if constexpr (OP == FP_SUB) r = fp_sub(ld_fp(a + o), ld_fp(b + o));
  else if constexpr (OP == FP_ADDL_MUL) r = fp_mul(fp_add_l(ld_fp(a + o), ld_fp(b + o)), ld_fp(c + o));
  else if constexpr (OP == FP_SUBL_MUL) r = fp_mul(fp_sub_l(ld_fp(a + o), ld_fp(b + o)), ld_fp(c + o));
  else if constexpr (OP == FP_NEG) r = fp_neg(ld_fp(a + o));
  else if constexpr (OP == FP_NEGL_MUL) r = fp_mul(ld_fp(a + o), fp_neg_l(ld_fp(b + o)));
  else if constexpr (OP == FP_MUL_SMALL) r = fp_mul_small(ld_fp(a + o), k);
  else if constexpr (OP == FP_REDUCE) r = fp_reduce(ld_fp(a + o));
  else if constexpr (OP == FP_CANON) r = fp_canon(ld_fp(a + o));
  else if constexpr (OP == FP_INV) r = fp_inv(ld_fp(a + o));
  else if constexpr (OP == FP_INV_FERMAT) r = fp_inv_fermat(ld_fp(a + o));
  else if constexpr (OP == FP_FROM_SIGNED) r = fp_from_signed((const int32_t*)a + o);
  else {  // the sign rule's comparison: the verdict in word 0, the other words 0
    r = fp_zero();
    r.l[0] = fp_lex_largest_canon(fp_from_mont(ld_fp(a + o))) ? 1u : 0u;
  }
  st_fp(out + o, r);
}

// ---------------------------------------------------------------------------
// row Fp (bls_row.h): one operand tuple per 16-lane row; rows past `nrows`
// leave (whole rows, as the product's partly filled last workgroups do)
enum { ROW_MUL, ROW_MUL2, ROW_REDUCE, ROW_NORM, ROW_NOPS };
constexpr uint32_t ROW_BLOCK_MAX = 16 * RW_PROD;  // L0_FINAL_THREADS
template <int OP>
__global__ void __launch_bounds__(ROW_BLOCK_MAX) k_row(const int32_t* a, const int32_t* b, const int32_t* c,
                                                       const int32_t* d, int32_t* out, uint32_t nrows) {
  const uint32_t row = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, j = threadIdx.x & 15u;
  if (row >= nrows) return;
  auto ld = [&](const int32_t* p) { return row_from_limbs((const uint32_t*)(p + (size_t)row * NL)); };
  R32 r;
  if constexpr (OP == ROW_MUL) r = row_mul(ld(a), ld(b));
  else if constexpr (OP == ROW_MUL2) r = row_mul2(ld(a), ld(b), ld(c), ld(d));
  else if constexpr (OP == ROW_REDUCE) r = row_reduce(r_norm(ld(a)));
  else r = r_norm(ld(a));
  out[(size_t)row * 16 + j] = r.v[0];
}

// ---------------------------------------------------------------------------
// row Fp12: one 576-thread workgroup, slots in LDS, loaded as k_l0_final /
// k_l0_fe load them (12 x 14 limbs in row order)
enum { R12_MUL, R12_CYC, R12_FROB, R12_CONJ, R12_FE, R12_ISONE, R12_NOPS };
template <int OP>
__global__ void __launch_bounds__(ROW_BLOCK_MAX) k_row12(const uint32_t* x, const uint32_t* y, int32_t* out,
                                                         uint32_t* flag) {
  __shared__ RowSlots S;
  RowDevExec ex;
  const int r = threadIdx.x >> 4, j = threadIdx.x & 15;
  constexpr int XS = (OP == R12_FROB || OP == R12_CONJ) ? 1 : 0;
  constexpr int YS = OP == R12_FE ? 5 : 1;
  ex([&](int) {
    if (r < RW_FP) {
      row_st(S.v[XS][r], row_from_limbs(x + r * NL));
      if constexpr (OP == R12_MUL || OP == R12_FE) row_st(S.v[YS][r], row_from_limbs(y + r * NL));
    }
  });
  if constexpr (OP == R12_MUL) row_mul_to(ex, S, 0, 0, 1);
  else if constexpr (OP == R12_CYC) row_cyc_sqr(ex, S, 0);
  else if constexpr (OP == R12_FROB) ex([&](int rr) { row_frob(rr, S.v[0], S.v[1]); });
  else if constexpr (OP == R12_CONJ) ex([&](int rr) { row_conj(rr, S.v[0], S.v[1]); });
  else if constexpr (OP == R12_FE) row_final_exp_inv(ex, S);
  if constexpr (OP == R12_FE || OP == R12_ISONE) {
    if (threadIdx.x == 0) flag[0] = row_is_one(S.v[0]) ? 1u : 0u;
  }
  if (r < RW_FP) out[r * 16 + j] = S.v[0][r][j];
}

// the 68 -g1-folded lines of one affine G2 point on rows, as k_l0_lines
constexpr uint32_t ROW_LINES_THREADS = 16 * 12;
__global__ void __launch_bounds__(ROW_LINES_THREADS) k_row_lines(const uint32_t* q, uint32_t* out) {
  __shared__ RowLineSlots S;
  RowDevExec ex;
  const int r = threadIdx.x >> 4;
  ex([&](int) {
    const G2A& Q = *(const G2A*)q;
    const Fp nx = fp_reduce(fp_neg(fp_from_const(G1_X))), y = fp_from_const(G1_NEG_Y);
    const Fp* c[12] = {&Q.x.c0, &Q.x.c1, &Q.y.c0, &Q.y.c1, nullptr, nullptr, &Q.x.c0, &Q.x.c1, &Q.y.c0, &Q.y.c1, &nx, &y};
    const Fp one = fp_one(), zero = fp_zero();
    const Fp* v = r == 4 ? &one : (r == 5 ? &zero : c[r]);
    row_st(r < 10 ? S.s[r] : S.k[r - 10], row_from_limbs(v->l));
  });
  auto out6 = [&](int buf, int idx) {
    const int t = (int)threadIdx.x - 128;
    if (t >= 0 && t < 6) rl_line_out(S, buf, t, out + (size_t)LINE_WORDS * idx);
  };
  row_g2_lines(ex, out6, S);
}

// ---------------------------------------------------------------------------
// hexad (bls_hex.h): hex_slot / hex_threads geometry, the product kernels'
// early return for lane 15 and slots past n
enum { HEX_MUL, HEX_SQR, HEX_CYC, HEX_FROB, HEX_CONJ, HEX_LINE, HEX_INV, HEX_FE, HEX_ISONE, HEX_NOPS };
constexpr int HEX_WORDS = 12 * NL;  // quad layout: 3 trio lanes x [a.c0, a.c1, b.c0, b.c1]
template <int OP>
__global__ void __launch_bounds__(64, TBG_HEX_WAVES) k_hex(const uint32_t* a, const uint32_t* b, const uint32_t* lines,
                                                           const uint32_t* pts, uint32_t* out, uint32_t* flags,
                                                           uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t s = hex_slot(t);
  if (s == 0xFFFFFFFFu || s >= n) return;
  const Fp4h A = hex_load(a + (size_t)HEX_WORDS * s);
  Fp4h R = A;
  if constexpr (OP == HEX_MUL) R = hex_mul(A, hex_load(b + (size_t)HEX_WORDS * s));
  else if constexpr (OP == HEX_SQR) R = hex_sqr(A);
  else if constexpr (OP == HEX_CYC) R = hex_cyc_sqr(A);
  else if constexpr (OP == HEX_FROB) R = hex_frob(A);
  else if constexpr (OP == HEX_CONJ) R = hex_conj(A);
  else if constexpr (OP == HEX_LINE)
    R = hex_line_at(A, lines + (size_t)LINE_WORDS * s, 0, ld_fp(pts + (size_t)2 * NL * s),
                    ld_fp(pts + (size_t)2 * NL * s + NL));
  else if constexpr (OP == HEX_INV) R = hex_inv_ni(A);
  else if constexpr (OP == HEX_FE) R = hex_final_exp_in(A);
  if constexpr (OP == HEX_FE || OP == HEX_ISONE) {
    const bool one = hex_is_one(R);
    // every lane of the hexad reports: word (3 c + q) of the slot's six
    flags[(size_t)6 * s + 3 * hex_c() + (uint32_t)quad_lane()] = one ? 1u : 0u;
  }
  if constexpr (OP != HEX_ISONE) hex_store(out + (size_t)HEX_WORDS * s, R);
}

// ---------------------------------------------------------------------------
// lane pair (bls_pair.h, Fp2x): pair k on lanes 2k, 2k + 1
enum { PAIR_MUL, PAIR_SQR, PAIR_INV, PAIR_CONJ, PAIR_MUL_XI, PAIR_MUL_CONST, PAIR_EQ, PAIR_GATHER, PAIR_NOPS };
template <int OP>
__global__ void __launch_bounds__(64) k_pair(const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* flags,
                                             uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, pr = t >> 1;
  if (pr >= n) return;
  const Fp2* A = (const Fp2*)a;
  const Fp2* B = (const Fp2*)b;
  const Fp2x x = px_load(A[pr]);
  if constexpr (OP == PAIR_EQ) {
    // each lane reports: bit 0 f_eq(a, b), bit 1 f_is_zero(a)
    const bool eq = f_eq(x, px_load(B[pr])), z = f_is_zero(x);
    flags[t] = (eq ? 1u : 0u) | (z ? 2u : 0u);
  } else if constexpr (OP == PAIR_GATHER) {
    ((Fp2*)out)[t] = px_gather(x);  // the whole Fp2, from each lane
  } else {
    Fp2x r;
    if constexpr (OP == PAIR_MUL) r = f_mul(x, px_load(B[pr]));
    else if constexpr (OP == PAIR_SQR) r = f_sqr(x);
    else if constexpr (OP == PAIR_INV) r = f_inv(x);
    else if constexpr (OP == PAIR_CONJ) r = px_conj(x);
    else if constexpr (OP == PAIR_MUL_XI) r = px_mul_xi(x);
    else r = px_mul_const(x, PSI_X);
    px_store(((Fp2*)out)[pr], r);
  }
}
// the 68 -g1-folded lines of each point, one pair per point (k_lines_fold)
__global__ void __launch_bounds__(64) k_pair_lines(const uint32_t* q, uint32_t* out, uint32_t n) {
  const uint32_t pr = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  if (pr >= n) return;
  const Fp nx = fp_reduce(fp_neg(fp_from_const(G1_X)));
  px_g2_lines<true>(px_load(((const G2A*)q)[pr]), nx, fp_from_const(G1_NEG_Y), out + (size_t)LINES_WORDS * pr);
}

// ---------------------------------------------------------------------------
// workgroup batch inversion (bls_batchinv.h): one value per thread, every
// thread of every workgroup calls (barriers); threads past n hold nothing
template <int W>
__global__ void __launch_bounds__(64 * W) k_binv(const uint32_t* z, const uint32_t* present, uint32_t* out, uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = t < n;
  const Fp v = in ? ld_fp(z + (size_t)t * NL) : fp_zero();
  const Fp r = block_batch_inv<W>(v, in && present[t] != 0);
  if (in) st_fp(out + (size_t)t * NL, r);
}
template <int W, class F>
__global__ void __launch_bounds__(64 * W) k_j2a(const uint32_t* p, const uint32_t* want, uint32_t* out, uint32_t* ok,
                                                uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = t < n;
  Jac<F> P{};
  if (in) P = ((const Jac<F>*)p)[t];
  Aff<F> A;
  const bool got = block_jac_to_aff<W>(P, in && want[t] != 0, A);
  if (in) {
    ok[t] = got ? 1u : 0u;
    if (got) ((Aff<F>*)out)[t] = A;
  }
}

}  // namespace

// ===========================================================================
extern "C" {

int dc_sticky_error(void) { return g_err; }
int dc_binv_waves(void) { return BINV_WAVES; }

#define DC_CASE(K, OP, ...) \
  case OP: hipLaunchKernelGGL(K<OP>, grid, block, 0, 0, __VA_ARGS__); break;

// lane-private Fp: n tuples, operands a..d (null where the op takes none), 14 words each
int dc_fp(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t k,
          uint32_t* out, uint32_t n) {
  static const int need[FP_NOPS] = {2, 4, 1, 2, 2, 3, 3, 1, 2, 1, 1, 1, 1, 1, 1, 1};
  if (op < 0 || op >= FP_NOPS || n == 0 || !out) return -1;
  const uint32_t* given[4] = {a, b, c, d};
  for (int i = 0; i < need[op]; ++i)
    if (!given[i]) return -1;
  Run R;
  const size_t w = (size_t)n * NL;
  const uint32_t *da = R.in(a, w), *db = R.in(b, w), *dc = R.in(c, w), *dd = R.in(d, w);
  uint32_t* dout = R.io(out, w);
  const dim3 grid((n + 63) / 64), block(64);
  if (R.ok()) switch (op) {
    DC_CASE(k_fp, FP_MUL, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_MUL2, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_SQR, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_ADD, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_SUB, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_ADDL_MUL, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_SUBL_MUL, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_NEG, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_NEGL_MUL, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_MUL_SMALL, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_REDUCE, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_CANON, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_INV, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_INV_FERMAT, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_FROM_SIGNED, da, db, dc, dd, k, dout, n)
    DC_CASE(k_fp, FP_LEX, da, db, dc, dd, k, dout, n)
  }
  return R.finish();
}

// row Fp: nrows tuples of 14 signed limbs; out 16 words per row; `threads`
// = 64 (four rows a wave, as many workgroups as needed) or 576 (ONE
// workgroup of 36 rows: nrows <= 36)
int dc_row(int op, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d, int32_t* out,
           uint32_t nrows, uint32_t threads) {
  static const int need[ROW_NOPS] = {2, 4, 1, 1};
  if (op < 0 || op >= ROW_NOPS || nrows == 0 || !out) return -1;
  const int32_t* given[4] = {a, b, c, d};
  for (int i = 0; i < need[op]; ++i)
    if (!given[i]) return -1;
  if (threads != 64 && !(threads == ROW_BLOCK_MAX && nrows <= RW_PROD)) return -1;
  Run R;
  const size_t w = (size_t)nrows * NL;
  const int32_t *da = R.in(a, w), *db = R.in(b, w), *dc = R.in(c, w), *dd = R.in(d, w);
  int32_t* dout = R.io(out, (size_t)nrows * 16);
  const dim3 grid((nrows * 16 + threads - 1) / threads), block(threads);
  if (R.ok()) switch (op) {
    DC_CASE(k_row, ROW_MUL, da, db, dc, dd, dout, nrows)
    DC_CASE(k_row, ROW_MUL2, da, db, dc, dd, dout, nrows)
    DC_CASE(k_row, ROW_REDUCE, da, db, dc, dd, dout, nrows)
    DC_CASE(k_row, ROW_NORM, da, db, dc, dd, dout, nrows)
  }
  return R.finish();
}

// row Fp12: x, y = 12 x 14 limbs in row order (y: the second factor, or the
// inverse for R12_FE); out 12 x 16 words; flag: row_is_one (R12_FE, R12_ISONE)
int dc_row12(int op, const uint32_t* x, const uint32_t* y, int32_t* out, uint32_t* flag) {
  if (op < 0 || op >= R12_NOPS || !x || !out || !flag || ((op == R12_MUL || op == R12_FE) && !y)) return -1;
  Run R;
  const uint32_t *dx = R.in(x, (size_t)RW_FP * NL), *dy = R.in(y, (size_t)RW_FP * NL);
  int32_t* dout = R.io(out, (size_t)RW_FP * 16);
  uint32_t* dflag = R.io(flag, 1);
  const dim3 grid(1), block(ROW_BLOCK_MAX);
  if (R.ok()) switch (op) {
    DC_CASE(k_row12, R12_MUL, dx, dy, dout, dflag)
    DC_CASE(k_row12, R12_CYC, dx, dy, dout, dflag)
    DC_CASE(k_row12, R12_FROB, dx, dy, dout, dflag)
    DC_CASE(k_row12, R12_CONJ, dx, dy, dout, dflag)
    DC_CASE(k_row12, R12_FE, dx, dy, dout, dflag)
    DC_CASE(k_row12, R12_ISONE, dx, dy, dout, dflag)
  }
  return R.finish();
}

// q: x.c0 x.c1 y.c0 y.c1 (14 words each); out: LINES_WORDS
int dc_row_lines(const uint32_t* q, uint32_t* out) {
  if (!q || !out) return -1;
  Run R;
  const uint32_t* dq = R.in(q, (size_t)4 * NL);
  uint32_t* dout = R.io(out, (size_t)LINES_WORDS);
  if (R.ok()) hipLaunchKernelGGL(k_row_lines, dim3(1), dim3(ROW_LINES_THREADS), 0, 0, dq, dout);
  return R.finish();
}

// hexad: n slots of 168 words (quad layout); `cap` >= n is the size of the
// out / flags buffers in slots (the words past n must come back untouched).
// lines: one stored line (LINE_WORDS) per slot; pts: (-x, y) per slot.
int dc_hex(int op, const uint32_t* a, const uint32_t* b, const uint32_t* lines, const uint32_t* pts, uint32_t* out,
           uint32_t* flags, uint32_t n, uint32_t cap) {
  if (op < 0 || op >= HEX_NOPS || n == 0 || cap < n || !a || !out || !flags) return -1;
  if ((op == HEX_MUL && !b) || (op == HEX_LINE && (!lines || !pts))) return -1;
  Run R;
  const uint32_t *da = R.in(a, (size_t)n * HEX_WORDS), *db = R.in(b, (size_t)n * HEX_WORDS);
  const uint32_t *dl = R.in(lines, (size_t)n * LINE_WORDS), *dp = R.in(pts, (size_t)n * 2 * NL);
  uint32_t* dout = R.io(out, (size_t)cap * HEX_WORDS);
  uint32_t* dflags = R.io(flags, (size_t)cap * 6);
  const dim3 grid(hex_threads(n) / 64), block(64);
  if (R.ok()) switch (op) {
    DC_CASE(k_hex, HEX_MUL, da, db, dl, dp, dout, dflags, n)
    DC_CASE(k_hex, HEX_SQR, da, db, dl, dp, dout, dflags, n)
    DC_CASE(k_hex, HEX_CYC, da, db, dl, dp, dout, dflags, n)
    DC_CASE(k_hex, HEX_FROB, da, db, dl, dp, dout, dflags, n)
    DC_CASE(k_hex, HEX_CONJ, da, db, dl, dp, dout, dflags, n)
    DC_CASE(k_hex, HEX_LINE, da, db, dl, dp, dout, dflags, n)
    DC_CASE(k_hex, HEX_INV, da, db, dl, dp, dout, dflags, n)
    DC_CASE(k_hex, HEX_FE, da, db, dl, dp, dout, dflags, n)
    DC_CASE(k_hex, HEX_ISONE, da, db, dl, dp, dout, dflags, n)
  }
  return R.finish();
}

// lane pair: n Fp2 (28 words); out n Fp2 (PAIR_GATHER: 2 n, one per lane);
// flags 2 n words (PAIR_EQ: one per lane); `cap` as dc_hex
int dc_pair(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* flags, uint32_t n, uint32_t cap) {
  if (op < 0 || op >= PAIR_NOPS || n == 0 || cap < n || !a) return -1;
  if (((op == PAIR_MUL || op == PAIR_EQ) && !b) || (op == PAIR_EQ ? !flags : !out)) return -1;
  Run R;
  const uint32_t *da = R.in(a, (size_t)n * 2 * NL), *db = R.in(b, (size_t)n * 2 * NL);
  uint32_t* dout = R.io(out, (size_t)cap * 2 * NL * (op == PAIR_GATHER ? 2 : 1));
  uint32_t* dflags = R.io(flags, (size_t)cap * 2);
  const dim3 grid((2 * n + 63) / 64), block(64);
  if (R.ok()) switch (op) {
    DC_CASE(k_pair, PAIR_MUL, da, db, dout, dflags, n)
    DC_CASE(k_pair, PAIR_SQR, da, db, dout, dflags, n)
    DC_CASE(k_pair, PAIR_INV, da, db, dout, dflags, n)
    DC_CASE(k_pair, PAIR_CONJ, da, db, dout, dflags, n)
    DC_CASE(k_pair, PAIR_MUL_XI, da, db, dout, dflags, n)
    DC_CASE(k_pair, PAIR_MUL_CONST, da, db, dout, dflags, n)
    DC_CASE(k_pair, PAIR_EQ, da, db, dout, dflags, n)
    DC_CASE(k_pair, PAIR_GATHER, da, db, dout, dflags, n)
  }
  return R.finish();
}
int dc_pair_lines(const uint32_t* q, uint32_t* out, uint32_t n, uint32_t cap) {
  if (n == 0 || cap < n || !q || !out) return -1;
  Run R;
  const uint32_t* dq = R.in(q, (size_t)n * 4 * NL);
  uint32_t* dout = R.io(out, (size_t)cap * LINES_WORDS);
  if (R.ok()) hipLaunchKernelGGL(k_pair_lines, dim3((2 * n + 63) / 64), dim3(64), 0, 0, dq, dout, n);
  return R.finish();
}

// batch inversion over workgroups of `waves` waves (BINV_WAVES or 4)
int dc_batch_inv(int waves, const uint32_t* z, const uint32_t* present, uint32_t* out, uint32_t n, uint32_t cap) {
  if ((waves != BINV_WAVES && waves != 4) || n == 0 || cap < n || !z || !present || !out) return -1;
  Run R;
  const uint32_t *dz = R.in(z, (size_t)n * NL), *dp = R.in(present, n);
  uint32_t* dout = R.io(out, (size_t)cap * NL);
  const uint32_t bs = 64u * (uint32_t)waves;
  const dim3 grid((n + bs - 1) / bs), block(bs);
  if (R.ok()) {
    if (waves == 4) hipLaunchKernelGGL(k_binv<4>, grid, block, 0, 0, dz, dp, dout, n);
    else hipLaunchKernelGGL(k_binv<BINV_WAVES>, grid, block, 0, 0, dz, dp, dout, n);
  }
  return R.finish();
}
// Jacobian -> affine, g = 1 (Fp: 3 x 14 words in, 2 x 14 out) or 2 (Fp2)
int dc_jac_to_aff(int g, int waves, const uint32_t* p, const uint32_t* want, uint32_t* out, uint32_t* ok, uint32_t n,
                  uint32_t cap) {
  if ((g != 1 && g != 2) || (waves != BINV_WAVES && waves != 4) || n == 0 || cap < n || !p || !want || !out ||
      !ok)
    return -1;
  Run R;
  const uint32_t *dp = R.in(p, (size_t)n * 3 * g * NL), *dw = R.in(want, n);
  uint32_t* dout = R.io(out, (size_t)cap * 2 * g * NL);
  uint32_t* dok = R.io(ok, cap);
  const uint32_t bs = 64u * (uint32_t)waves;
  const dim3 grid((n + bs - 1) / bs), block(bs);
  if (R.ok()) {
    if (g == 1 && waves == 4) hipLaunchKernelGGL((k_j2a<4, Fp>), grid, block, 0, 0, dp, dw, dout, dok, n);
    else if (g == 1) hipLaunchKernelGGL((k_j2a<BINV_WAVES, Fp>), grid, block, 0, 0, dp, dw, dout, dok, n);
    else if (waves == 4) hipLaunchKernelGGL((k_j2a<4, Fp2>), grid, block, 0, 0, dp, dw, dout, dok, n);
    else hipLaunchKernelGGL((k_j2a<BINV_WAVES, Fp2>), grid, block, 0, 0, dp, dw, dout, dok, n);
  }
  return R.finish();
}

}  // extern "C"
