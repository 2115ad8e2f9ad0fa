// Device unit harness for the hash-to-G2 kernel chain: the third source of
// tests/devcheck.  TEST TOOLING ONLY.
//
// This source #includes charon_amd/csrc/k_hash.hip itself, so k_hash_map,
// k_hash_sswu, k_hash_affine and launch_hash_msgs below are the product's own
// text compiled with the product's macros and that unit's flags (none beyond
// the common ones).  The cofactor-clearing kernels are included the same way
// by devcheck_h2c_clear.hip, which takes k_hash_clear.hip's per-unit flags.
//
// dc_h2c runs a contiguous run of the chain's stages on a zeroed DevBatch in
// which only n_msgs, msgs, msg_off, h_jac, h_aff and h_status are set, with
// the product's grids and blocks.  Entering at a later stage means the caller
// preloads the h_jac slots that stage reads.  As the other devcheck sources:
// the entry allocates, copies in (the outputs too, so a sentinel shows every
// unwritten word), runs, synchronises, copies out and frees; the HIP status
// is sticky, and after a failure nothing is freed and nothing runs.
#include "../../charon_amd/csrc/k_hash.hip"

namespace tbg {
// TBG_KLAUNCH's hooks (tbls_engine.hip in the product): nothing to record here
void kprof_pre(const char*, hipStream_t) {}
void kprof_post(hipStream_t) {}
void debug_after_launch(const char*, hipStream_t) {}

// k_hash_map's body from injected field elements: u holds u0, u1 per message
__global__ void __launch_bounds__(BINV_BLOCK, TBG_DECODE_WAVES) k_hash_map_u(DevBatch B, const Fp2* u) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = m < B.n_msgs;
  const Fp2 u0 = in ? u[2 * m] : fp2_zero(), u1 = in ? u[2 * m + 1] : fp2_zero();
  hash_map_from_u(B, m, in, u0, u1);
}

// fp2_sqrt_or_z_in as k_hash_sswu calls it, one lane per value: the input
// waits in a memory slot across the two exponentiations.  flags: bit 0 the
// return value, bit 1 `sq`; the root is zero where the function wrote none.
__global__ void TBG_LAUNCH_N(TBG_DECODE_WAVES) k_sqrt_or_z(const Fp2* a, Fp2* slot, Fp2* root, uint32_t* flags,
                                                           uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Fp2 r = fp2_zero();
  bool sq = false;
  const bool done = fp2_sqrt_or_z_in<SSWU_WIN>(a[t], r, sq, SlotKeep{&slot[t]});
  root[t] = r;
  flags[t] = (done ? 1u : 0u) | (sq ? 2u : 0u);
}
}  // namespace tbg

using namespace tbg;

// devcheck_h2c_clear.hip: one cofactor-clearing kernel with the product's grid
void dc_h2c_clear_stage(int stage, const DevBatch& B, hipStream_t st);

namespace {

int g_err = 0;  // sticky HIP status (this source's own)

constexpr uint32_t FP2_W = 2 * NL, AFF_W = 4 * NL, JAC_W = 6 * NL;
static_assert(sizeof(Fp2) == FP2_W * 4 && sizeof(G2A) == AFF_W * 4 && sizeof(G2J) == JAC_W * 4, "raw-limb layout");

enum { H2C_MAP_MSG, H2C_MAP_U, H2C_SSWU, H2C_CLEAR_X1, H2C_CLEAR_X2, H2C_CLEAR_FIN, H2C_AFFINE, H2C_NSTAGES };

}  // namespace

extern "C" {

int dc_sticky_error(void);     // devcheck.hip
int dc_g2_sticky_error(void);  // devcheck_g2.hip
int dc_h2c_sticky_error(void) { return g_err; }
int dc_h2c_binv_block(void) { return BINV_BLOCK; }

// Stages first..last of the chain for n messages (MAP_MSG and MAP_U are the
// two forms of the first stage: a run that starts at MAP_MSG goes on at SSWU).
//   msgs, msg_off   [msg_off[n]] bytes, [n + 1] offsets (MAP_MSG only)
//   u_words         [n][2] Fp2: u0, u1 per message (MAP_U only)
//   hjac_words      in + out: the 3 n Jacobian slots of h_jac, then cap - n more
//                   that must come back untouched
//   haff_words      out: cap affine points;  hstatus: out, cap words
int dc_h2c(int first, int last, uint32_t n, const uint8_t* msgs, const uint32_t* msg_off, const uint32_t* u_words,
           uint32_t* hjac_words, uint32_t* haff_words, int32_t* hstatus, uint32_t cap) {
  if (first < 0 || last >= H2C_NSTAGES || last < first || (first == H2C_MAP_MSG && last == H2C_MAP_U)) return -1;
  if (n == 0 || cap < n || n > (1u << 20) || !hjac_words || !haff_words || !hstatus) return -1;
  if (first == H2C_MAP_MSG) {
    if (!msgs || !msg_off || msg_off[0] != 0) return -1;
    for (uint32_t i = 0; i < n; ++i)
      if (msg_off[i + 1] < msg_off[i]) return -1;
  }
  if (first == H2C_MAP_U && !u_words) return -1;
  if (g_err) return g_err;
  if (dc_sticky_error()) return dc_sticky_error();
  if (dc_g2_sticky_error()) return dc_g2_sticky_error();
  const size_t wm = first == H2C_MAP_MSG ? msg_off[n] : 0, wo = first == H2C_MAP_MSG ? (size_t)(n + 1) * 4 : 0;
  const size_t wu = first == H2C_MAP_U ? (size_t)n * 2 * FP2_W * 4 : 0;
  const size_t wj = ((size_t)3 * n + (cap - n)) * JAC_W * 4, wa = (size_t)cap * AFF_W * 4, ws = (size_t)cap * 4;
  uint8_t* dm = nullptr;
  uint32_t *doff = nullptr, *du = nullptr, *dj = nullptr, *da = nullptr;
  int32_t* ds = nullptr;
  int err = (int)hipMalloc((void**)&dm, wm ? wm : 4);
  if (!err) err = (int)hipMalloc((void**)&doff, wo ? wo : 4);
  if (!err) err = (int)hipMalloc((void**)&du, wu ? wu : 4);
  if (!err) err = (int)hipMalloc((void**)&dj, wj);
  if (!err) err = (int)hipMalloc((void**)&da, wa);
  if (!err) err = (int)hipMalloc((void**)&ds, ws);
  if (!err && wm) err = (int)hipMemcpy(dm, msgs, wm, hipMemcpyHostToDevice);
  if (!err && wo) err = (int)hipMemcpy(doff, msg_off, wo, hipMemcpyHostToDevice);
  if (!err && wu) err = (int)hipMemcpy(du, u_words, wu, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(dj, hjac_words, wj, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(da, haff_words, wa, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(ds, hstatus, ws, hipMemcpyHostToDevice);
  if (!err) {
    DevBatch B = {};
    B.n_msgs = n;
    B.msgs = dm;
    B.msg_off = doff;
    B.h_jac = (G2J*)dj;
    B.h_aff = (G2A*)da;
    B.h_status = ds;
    const hipStream_t st = 0;
    const dim3 grid((n + BINV_BLOCK - 1) / BINV_BLOCK);
    if (first == H2C_MAP_MSG && last == H2C_AFFINE) {
      launch_hash_msgs(B, st);  // the product's launcher, whole
    } else {
      for (int s = first; s <= last; ++s) {
        if (s == H2C_MAP_U && first != H2C_MAP_U) continue;
        if (s == H2C_MAP_MSG) TBG_KLAUNCH(k_hash_map, grid, dim3(BINV_BLOCK), st, B);
        else if (s == H2C_MAP_U) TBG_KLAUNCH(k_hash_map_u, grid, dim3(BINV_BLOCK), st, B, (const Fp2*)du);
        else if (s == H2C_SSWU) TBG_KLAUNCH(k_hash_sswu, grid_for(2 * n), dim3(kBlock), st, B);
        else if (s == H2C_CLEAR_X1 && last >= H2C_CLEAR_FIN) {
          launch_hash_clear(B, st);  // the product's launcher for the three clearing kernels
          s = H2C_CLEAR_FIN;
        } else if (s == H2C_AFFINE) TBG_KLAUNCH(k_hash_affine, grid, dim3(BINV_BLOCK), st, B);
        else dc_h2c_clear_stage(s - H2C_CLEAR_X1, B, st);
      }
    }
    err = (int)hipGetLastError();
  }
  if (!err) err = (int)hipDeviceSynchronize();
  if (!err) err = (int)hipMemcpy(hjac_words, dj, wj, hipMemcpyDeviceToHost);
  if (!err) err = (int)hipMemcpy(haff_words, da, wa, hipMemcpyDeviceToHost);
  if (!err) err = (int)hipMemcpy(hstatus, ds, ws, hipMemcpyDeviceToHost);
  if (!err) {
    (void)hipFree(dm);
    (void)hipFree(doff);
    (void)hipFree(du);
    (void)hipFree(dj);
    (void)hipFree(da);
    (void)hipFree(ds);
  } else {
    g_err = err;  // (after a failure nothing more is asked of the device, frees included)
  }
  return err;
}

// n values a (Fp2 each); root: cap Fp2, flags: cap words (cap >= n: the words
// past item n must come back untouched)
int dc_h2c_sqrt(const uint32_t* a_words, uint32_t* root_words, uint32_t* flags, uint32_t n, uint32_t cap) {
  if (n == 0 || cap < n || n > (1u << 20) || !a_words || !root_words || !flags) return -1;
  if (g_err) return g_err;
  if (dc_sticky_error()) return dc_sticky_error();
  if (dc_g2_sticky_error()) return dc_g2_sticky_error();
  const size_t wi = (size_t)n * FP2_W * 4, wr = (size_t)cap * FP2_W * 4, wf = (size_t)cap * 4;
  uint32_t *da = nullptr, *dslot = nullptr, *dr = nullptr, *df = nullptr;
  int err = (int)hipMalloc((void**)&da, wi);
  if (!err) err = (int)hipMalloc((void**)&dslot, wi);
  if (!err) err = (int)hipMalloc((void**)&dr, wr);
  if (!err) err = (int)hipMalloc((void**)&df, wf);
  if (!err) err = (int)hipMemcpy(da, a_words, wi, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemset(dslot, 0, wi);
  if (!err) err = (int)hipMemcpy(dr, root_words, wr, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(df, flags, wf, hipMemcpyHostToDevice);
  if (!err) {
    hipLaunchKernelGGL(k_sqrt_or_z, grid_for(n), dim3(kBlock), 0, 0, (const Fp2*)da, (Fp2*)dslot, (Fp2*)dr, df, n);
    err = (int)hipGetLastError();
  }
  if (!err) err = (int)hipDeviceSynchronize();
  if (!err) err = (int)hipMemcpy(root_words, dr, wr, hipMemcpyDeviceToHost);
  if (!err) err = (int)hipMemcpy(flags, df, wf, hipMemcpyDeviceToHost);
  if (!err) {
    (void)hipFree(da);
    (void)hipFree(dslot);
    (void)hipFree(dr);
    (void)hipFree(df);
  } else {
    g_err = err;
  }
  return err;
}

}  // extern "C"
