// Device unit harness for the decode kernels: the fifth source of
// tests/devcheck.  TEST TOOLING ONLY.
//
// This source #includes charon_amd/csrc/k_decode.hip itself and is compiled
// with the flags charon_amd/_native.py gives that unit, so k_decode_sigs,
// k_subgroup_sigs, k_decode_pubkeys, launch_decode_sigs and
// launch_decode_pubkeys below are the product's own text as the product
// builds it: the decode window, the SlotKeep slot inside the output record,
// TBG_SCHED_FENCE, TBG_ADD_DBL_INLINE and the workgroup-wide
// block_jac_to_aff, none of which the host build has.
//
// dc_decode_sigs runs k_decode_sigs, k_subgroup_sigs or both on a zeroed
// DevBatch in which only n_partials, sigs, sig_aff, partial_status, counters,
// msm_off, rlc_batch, sgb, sgb_m and sgb_bad are set.  As the other devcheck
// sources: the entry allocates, copies in (the outputs too, so a sentinel
// shows every unwritten word), runs, synchronises, copies out and frees; the
// HIP status is sticky, and after a failure nothing is freed and nothing runs.
#include "../../charon_amd/csrc/k_decode.hip"

namespace tbg {
// launch_decode_sigs queues the batched subgroup test (k_sgb.hip) between its
// two kernels; that chain is not part of this library.  With B.sgb set the
// caller supplies sgb_bad, which is all k_subgroup_sigs reads of it.
void launch_subgroup_batch(const DevBatch&, hipStream_t) {}
}  // namespace tbg

using namespace tbg;

namespace {

int g_err = 0;  // sticky HIP status (this source's own)

constexpr uint32_t AFF_W = 4 * NL, G1A_W = 2 * NL;
static_assert(sizeof(G2A) == AFF_W * 4 && sizeof(G1A) == G1A_W * 4, "raw-limb layout");

enum { DEC_DECODE, DEC_SUBGROUP, DEC_NSTAGES };

}  // namespace

extern "C" {

int dc_sticky_error(void);      // devcheck.hip
int dc_g2_sticky_error(void);   // devcheck_g2.hip
int dc_h2c_sticky_error(void);  // devcheck_h2c.hip
int dc_decode_sticky_error(void) { return g_err; }
int dc_decode_binv_block(void) { return BINV_BLOCK; }
int dc_decode_cnt_words(void) { return CNT_WORDS; }
int dc_decode_msm_buckets(void) { return MSM_BUCKETS; }

// Stages first..last (0: k_decode_sigs, 1: k_subgroup_sigs) for n partials.
//   sigs            [n][96] bytes (DECODE only)
//   sig_aff         in + out: cap affine points (56 words each); entering at
//                   SUBGROUP the caller preloads the first n
//   partial_status  in + out: cap words, preloaded likewise
//   counters        in + out: CNT_WORDS + 1 words
//   msm_off         in + out: MSM_BUCKETS + 2 words
//   rlc_batch       DevBatch::rlc_batch (rlc_group stays 0: level 0 unfused)
//   sgb, sgb_m      DevBatch::sgb, sgb_m;  sgb_bad: [(n + sgb_m - 1) / sgb_m] words
// n == 0 is allowed from DECODE: the first kernel's duties remain.
int dc_decode_sigs(int first, int last, uint32_t n, const uint8_t* sigs, uint32_t* sig_aff, int32_t* partial_status,
                   uint32_t* counters, uint32_t* msm_off, uint32_t rlc_batch, uint32_t sgb, uint32_t sgb_m,
                   const uint32_t* sgb_bad, uint32_t cap) {
  if (first < 0 || last >= DEC_NSTAGES || last < first) return -1;
  if (cap < n || cap == 0 || cap > (1u << 20) || !sig_aff || !partial_status || !counters || !msm_off) return -1;
  if (first == DEC_DECODE && n && !sigs) return -1;
  if (first == DEC_SUBGROUP && n == 0) return -1;
  if (sgb && (sgb_m == 0 || !sgb_bad)) return -1;
  if (g_err) return g_err;
  if (dc_sticky_error()) return dc_sticky_error();
  if (dc_g2_sticky_error()) return dc_g2_sticky_error();
  if (dc_h2c_sticky_error()) return dc_h2c_sticky_error();
  const size_t wsig = first == DEC_DECODE ? (size_t)n * 96 : 0, wa = (size_t)cap * AFF_W * 4, ws = (size_t)cap * 4;
  const size_t wc = (size_t)(CNT_WORDS + 1) * 4, wm = (size_t)(MSM_BUCKETS + 2) * 4;
  const size_t wb = sgb ? (size_t)((n + sgb_m - 1) / sgb_m) * 4 : 0;
  uint8_t* dsig = nullptr;
  uint32_t *da = nullptr, *dc = nullptr, *dm = nullptr, *db = nullptr;
  int32_t* ds = nullptr;
  int err = (int)hipMalloc((void**)&dsig, wsig ? wsig : 4);
  if (!err) err = (int)hipMalloc((void**)&da, wa);
  if (!err) err = (int)hipMalloc((void**)&ds, ws);
  if (!err) err = (int)hipMalloc((void**)&dc, wc);
  if (!err) err = (int)hipMalloc((void**)&dm, wm);
  if (!err) err = (int)hipMalloc((void**)&db, wb ? wb : 4);
  if (!err && wsig) err = (int)hipMemcpy(dsig, sigs, wsig, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(da, sig_aff, wa, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(ds, partial_status, ws, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(dc, counters, wc, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(dm, msm_off, wm, hipMemcpyHostToDevice);
  if (!err && wb) err = (int)hipMemcpy(db, sgb_bad, wb, hipMemcpyHostToDevice);
  if (!err) {
    DevBatch B = {};
    B.n_partials = n;
    B.sigs = dsig;
    B.sig_aff = (G2A*)da;
    B.partial_status = ds;
    B.counters = dc;
    B.msm_off = dm;
    B.rlc_batch = rlc_batch;
    B.sgb = sgb;
    B.sgb_m = sgb_m;
    B.sgb_bad = db;
    const hipStream_t st = 0;
    if (first == DEC_DECODE && last == DEC_SUBGROUP) {
      launch_decode_sigs(B, st);  // the product's launcher, whole
    } else if (first == DEC_DECODE) {
      // k_decode_sigs alone, with launch_decode_sigs' grid
      uint32_t lanes = B.n_partials > CNT_WORDS ? B.n_partials : CNT_WORDS;
      if (B.rlc_batch && !l0_fused(B) && lanes < MSM_BUCKETS + 1) lanes = MSM_BUCKETS + 1;
      TBG_KLAUNCH(k_decode_sigs, grid_for(lanes), dim3(kBlock), st, B);
    } else {
      // k_subgroup_sigs alone, with launch_decode_sigs' grid
      TBG_KLAUNCH(k_subgroup_sigs, grid_for(2 * B.n_partials), dim3(kBlock), st, B);
    }
    err = (int)hipGetLastError();
  }
  if (!err) err = (int)hipDeviceSynchronize();
  if (!err) err = (int)hipMemcpy(sig_aff, da, wa, hipMemcpyDeviceToHost);
  if (!err) err = (int)hipMemcpy(partial_status, ds, ws, hipMemcpyDeviceToHost);
  if (!err) err = (int)hipMemcpy(counters, dc, wc, hipMemcpyDeviceToHost);
  if (!err) err = (int)hipMemcpy(msm_off, dm, wm, hipMemcpyDeviceToHost);
  if (!err) {
    (void)hipFree(dsig);
    (void)hipFree(da);
    (void)hipFree(ds);
    (void)hipFree(dc);
    (void)hipFree(dm);
    (void)hipFree(db);
  } else {
    g_err = err;  // (after a failure nothing more is asked of the device, frees included)
  }
  return err;
}

// launch_decode_pubkeys on n keys.  out, out_x: in + out, cap entries of 28
// words (the key, [x] key); status: in + out, cap words.
int dc_decode_pubkeys(uint32_t n, const uint8_t* pk48, uint32_t* out, uint32_t* out_x, int32_t* status, uint32_t cap) {
  if (n == 0 || cap < n || cap > (1u << 20) || !pk48 || !out || !out_x || !status) return -1;
  if (g_err) return g_err;
  if (dc_sticky_error()) return dc_sticky_error();
  if (dc_g2_sticky_error()) return dc_g2_sticky_error();
  if (dc_h2c_sticky_error()) return dc_h2c_sticky_error();
  const size_t wk = (size_t)n * 48, wo = (size_t)cap * G1A_W * 4, ws = (size_t)cap * 4;
  uint8_t* dk = nullptr;
  uint32_t *dout = nullptr, *doutx = nullptr;
  int32_t* ds = nullptr;
  int err = (int)hipMalloc((void**)&dk, wk);
  if (!err) err = (int)hipMalloc((void**)&dout, wo);
  if (!err) err = (int)hipMalloc((void**)&doutx, wo);
  if (!err) err = (int)hipMalloc((void**)&ds, ws);
  if (!err) err = (int)hipMemcpy(dk, pk48, wk, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(dout, out, wo, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(doutx, out_x, wo, hipMemcpyHostToDevice);
  if (!err) err = (int)hipMemcpy(ds, status, ws, hipMemcpyHostToDevice);
  if (!err) {
    launch_decode_pubkeys(dk, n, (G1A*)dout, (G1A*)doutx, ds, 0);
    err = (int)hipGetLastError();
  }
  if (!err) err = (int)hipDeviceSynchronize();
  if (!err) err = (int)hipMemcpy(out, dout, wo, hipMemcpyDeviceToHost);
  if (!err) err = (int)hipMemcpy(out_x, doutx, wo, hipMemcpyDeviceToHost);
  if (!err) err = (int)hipMemcpy(status, ds, ws, hipMemcpyDeviceToHost);
  if (!err) {
    (void)hipFree(dk);
    (void)hipFree(dout);
    (void)hipFree(doutx);
    (void)hipFree(ds);
  } else {
    g_err = err;
  }
  return err;
}

}  // extern "C"
