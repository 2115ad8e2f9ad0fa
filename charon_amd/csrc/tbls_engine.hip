// libtbls_gpu.so: the C ABI of include/tbls_gpu.h on top of the HIP kernels.
//
// Per context: one HIP stream on one device, a resident public-key table,
// and a ring of in-flight batch slots.  tbg_submit packs the caller's
// structure-of-arrays batch into one pinned buffer, issues a single H2D copy,
// the kernel chain and a single D2H copy of the results, then returns a
// ticket; tbg_collect waits for (or polls) the slot's event and unpacks.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <functional>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <new>
#include <random>
#include <thread>
#include <vector>
#include "tbls_launch.h"
#include "bls_l0msg.h"
#include "bls_lines.h"

using namespace tbg;

namespace tbg {
void debug_after_launch(const char* kernel, hipStream_t st) {
  static const bool on = getenv("TBG_DEBUG_SYNC") && getenv("TBG_DEBUG_SYNC")[0] == '1';
  if (!on) return;
  hipEvent_t a;
  (void)hipEventCreate(&a);
  (void)hipEventRecord(a, st);
  hipError_t e = hipEventSynchronize(a);
  (void)hipEventDestroy(a);
  fprintf(stderr, "[tbg] %s done: %s\n", kernel, hipGetErrorString(e));
}

struct KProfRec {
  const char* name;
  hipEvent_t a, b;
};
static thread_local std::vector<KProfRec>* g_kprof = nullptr;
// Every launch pushes a record, even when an event could not be created (its
// null events are skipped by kprof_post and reported as failed by the
// readout), so a record never takes a neighbour's end event.
void kprof_pre(const char* kernel, hipStream_t st) {
  if (!g_kprof) return;
  KProfRec r{kernel, nullptr, nullptr};
  if (hipEventCreate(&r.a) != hipSuccess) r.a = nullptr;
  if (r.a && hipEventCreate(&r.b) != hipSuccess) {
    (void)hipEventDestroy(r.a);
    r.a = r.b = nullptr;
  }
  if (r.a) (void)hipEventRecord(r.a, st);
  g_kprof->push_back(r);
}
void kprof_post(hipStream_t st) {
  if (!g_kprof || g_kprof->empty() || !g_kprof->back().b) return;
  (void)hipEventRecord(g_kprof->back().b, st);
}
}  // namespace tbg

namespace {

constexpr int kChainEvents = 11;

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// One caller batch inside a slot: tbg_submit_group packs several batches into
// one device batch (one launch per kernel for all of them); each keeps its
// own ticket and its slice of the outputs.
struct Part {
  tbg_ticket ticket = 0;
  uint32_t d0 = 0, nd = 0, p0 = 0, np = 0, m0 = 0, nm = 0;
  // level 0 by message (bls_l0msg.h): the chunks of the messages up to this part's
  // last, and the largest message's chunks among them -- a replayed prefix's own plan
  uint32_t ch1 = 0, maxch = 0;
  bool pending = false;     // not collected yet
  bool collecting = false;  // a blocking tbg_collect waits on the slot outside the context mutex
};

struct Slot {
  bool busy = false;        // some part is still pending
  bool express = false;     // the high-priority slot of small batches (tbg_config.express_partials)
  std::vector<Part> parts;
  tbg_ticket ticket = 0;    // first part's ticket (LRU order of the slots)
  uint32_t op = 0, n_duties = 0, n_partials = 0, n_msgs = 0;
  // pinned host staging
  uint8_t* h_in = nullptr;
  size_t h_in_cap = 0;
  uint8_t* h_out = nullptr;
  size_t h_out_cap = 0;
  // device memory: one input arena + one work/output arena
  uint8_t* d_in = nullptr;
  size_t d_in_cap = 0;
  uint8_t* d_work = nullptr;
  size_t d_work_cap = 0;
  size_t out_bytes = 0;
  hipStream_t st = nullptr;   // per-signature chain (decode, lines, verify, aggregate)
  hipStream_t st2 = nullptr;  // per-message chain (hash_to_G2, H(m) lines), joins st before verify
  hipEvent_t ev[kChainEvents] = {};  // see launch_chain
  hipEvent_t done = nullptr;
  float ms[8] = {};
  uint64_t seen_bad = 0, seen_total = 0;  // invalid / verified partials of the parts collected so far
  uint64_t seen_nsub = 0, seen_dec = 0;   // non-subgroup / all partials of the parts collected so far
  tbg::DevBatch B{};           // device view of the last batch (resident until the slot is reused)
  tbg::DevBatch last{};        // the batch as its last run launched it (a replay's prefix and shape):
                               // what tbg_fetch_stats / _fallback / _shape / _subgroup describe
  size_t w_out = 0;
  uint32_t sgb_m_small = 0;    // the group size of a prefix below sgb_tri_partials (its arena holds both layouts)
  // a set launch (tbg_submit_sets): its one part spans the padded device batch
  bool sets = false;
  uint32_t n_sets = 0;
  size_t o_sets = 0;           // set_status in the output image
};

}  // namespace

struct tbg_ctx {
  int device = 0;
  hipStream_t stream = nullptr;  // utility stream (pubkey table, test-vector generation)
  std::mutex mu;
  G1A* d_pk = nullptr;
  G1A* d_xpk = nullptr;  // [x] pk per entry (k_decode_pubkeys)
  G1A* d_pktab = nullptr;  // [PK_TAB per key] the RLC products' key tables (k_msm.hip k_pubkey_tables)
  int32_t* d_pk_status = nullptr;
  uint32_t n_pk = 0, cap_pk = 0;
  hipEvent_t retire_ev = nullptr;  // orders frees of outgrown pubkey tables after the slots' queued work
  hipEvent_t keys_ready = nullptr;  // the key table's last load / growth (slot streams wait on it)
  std::vector<Slot> slots;
  tbg_ticket next_ticket = 1;
  float last_ms[8] = {};
  // Defaults measured on MI355X (tools/sweep_rlc.sh, config 2): 16 duties per
  // level-1 group, 4 per Miller quad beat 8 / 2 by ~8 %: half the final
  // exponentiations and Fp12 squarings per duty.
  uint32_t rlc_group = 16;  // 0 = per-partial checks (TBG_VERIFY_EACH)
  uint32_t rlc_chunk = 4;
  bool chunk_auto = true;    // rlc_chunk not configured: level-0 launches of many duties take 8
  bool rlc_auto = false;     // rlc_group follows the observed invalid share (tbg_config.rlc_group = 0)
  uint32_t rlc_batch = TBG_RLC_L0_AUTO;  // level 0 (the whole device batch as one check)
  double invalid_ema = 0.0;  // exponential average of the invalid share of collected verified partials
  uint64_t rlc_seed = 0;   // 0 = OS randomness per batch
  uint64_t seed_ctr = 0;
  uint32_t gident = TBG_GIDENT_OFF;  // level 1g routing (tbg_config.gident)
  uint32_t fb_window = TBG_FB_WINDOW;  // fallback line buffer positions per pass (tbg_config.fb_window)
  uint32_t sgb_mode = TBG_SGB_AUTO;    // batched subgroup test (tbg_config.subgroup_batch)
  uint32_t express_max = TBG_EXPRESS_PARTIALS;  // batches up to this many partials prefer the express slot
  uint32_t l0_duty_partials = TBG_L0_DUTY_PARTIALS;  // fused level 0: P_d per duty from this many partials (tbg_config.l0_duty_partials)
  uint32_t l0_tail_partials = TBG_L0_TAIL_PARTIALS;  // fused level 0: S inside the key-side grid from this many partials (tbg_config.l0_tail_partials)
  uint32_t l0_msg_share = TBG_L0_MSG_SHARE;  // fused level 0: per message from this many duties per message (tbg_config.l0_msg_share)
  uint32_t sgb_tri_partials = TBG_SGB_TRI_PARTIALS;  // batched subgroup test: triple schedule from this many partials (tbg_config.sgb_tri_partials)
  uint32_t sgb_tri_m = SGB_TRI_M;                    // its group size (tbg_config.sgb_tri_m)
  uint32_t n_simd = 1024;  // SIMDs of the device (CUs x 4): the level-0 shape rule's unit (l0_shape)
  // host-side work of the submit / collect calls (tbg_host_stats): [submits,
  // partials submitted, pack ns, enqueue ns, collects, partials collected,
  // gather ns, wait ns]
  std::atomic<uint64_t> host[8] = {};
  double nonsub_ema = 0.0;  // exponential average of the non-subgroup share of collected partials
};

#define HIP_TRY(x)                       \
  do {                                   \
    hipError_t e_ = (x);                 \
    if (e_ != hipSuccess) return TBG_E_DEVICE; \
  } while (0)

// Capacity for an arena of `need` bytes: 25 % headroom for small arenas; big
// ones (a 16 x 10k-DV slot's work arena is ~5.9 GB) get 1/16 headroom rounded
// up to 256 MiB, so batch sizes that jitter around a boundary do not hipFree
// + hipMalloc (a device-wide synchronisation) on every submit.
static size_t arena_size(size_t need) {
  return need < (1ull << 30) ? align_up(need + need / 4, 1 << 20) : align_up(need + need / 16, 1ull << 28);
}

static int grow_pinned(uint8_t** p, size_t* cap, size_t need) {
  if (*cap >= need) return TBG_OK;
  if (*p) hipHostFree(*p);
  *p = nullptr;
  const size_t n = arena_size(need);
  if (hipHostMalloc((void**)p, n, hipHostMallocDefault) != hipSuccess) { *cap = 0; return TBG_E_OOM; }
  *cap = n;
  return TBG_OK;
}

static int grow_device(uint8_t** p, size_t* cap, size_t need) {
  if (*cap >= need) return TBG_OK;
  if (*p) hipFree(*p);
  *p = nullptr;
  const size_t n = arena_size(need);
  if (hipMalloc((void**)p, n) != hipSuccess) { *cap = 0; return TBG_E_OOM; }
  *cap = n;
  return TBG_OK;
}

extern "C" {

const char* tbg_strerror(int code) {
  switch (code) {
    case TBG_OK: return "ok";
    case TBG_E_INVALID_ARG: return "invalid argument";
    case TBG_E_DEVICE: return "HIP device error";
    case TBG_E_OOM: return "out of memory";
    case TBG_E_NO_DEVICE: return "no gfx950 device";
    case TBG_E_BUSY: return "all batch slots busy";
    case TBG_E_PENDING: return "batch still running";
    case TBG_E_TICKET: return "unknown ticket";
    default: return "unknown error";
  }
}

int tbg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int tbg_device_cu_count(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return TBG_E_NO_DEVICE;
  if (device < 0 || device >= ndev) return TBG_E_INVALID_ARG;
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return TBG_E_DEVICE;
  return n_cu;
}

int tbg_synchronize(tbg_ctx* c) {
  if (!c) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (c->stream) HIP_TRY(hipStreamSynchronize(c->stream));
  for (auto& s : c->slots) {
    if (s.st) HIP_TRY(hipStreamSynchronize(s.st));
    if (s.st2 && s.st2 != s.st) HIP_TRY(hipStreamSynchronize(s.st2));
  }
  return TBG_OK;
}

int tbg_init(const tbg_config* cfg, tbg_ctx** out) {
  if (!out) return TBG_E_INVALID_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return TBG_E_NO_DEVICE;
  int dev = cfg ? cfg->device : 0;
  if (dev < 0 || dev >= ndev) return TBG_E_INVALID_ARG;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return TBG_E_DEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return TBG_E_NO_DEVICE;
  tbg_ctx* c = new (std::nothrow) tbg_ctx();
  if (!c) return TBG_E_OOM;
  c->device = dev;
  if (cfg && cfg->verify_mode == TBG_VERIFY_EACH) c->rlc_group = 0;
  else if (cfg && cfg->verify_mode != TBG_VERIFY_RLC) { delete c; return TBG_E_INVALID_ARG; }
  else if (cfg && cfg->rlc_group) c->rlc_group = cfg->rlc_group;
  else c->rlc_auto = true;
  if (cfg && cfg->rlc_chunk) {
    c->rlc_chunk = cfg->rlc_chunk;
    c->chunk_auto = false;
  }
  if (c->rlc_group > 4096 || c->rlc_chunk > 4096) { delete c; return TBG_E_INVALID_ARG; }
  if (cfg && cfg->rlc_batch > TBG_RLC_L0_OFF) { delete c; return TBG_E_INVALID_ARG; }
  if (cfg) c->rlc_batch = cfg->rlc_batch;
  c->rlc_seed = cfg ? cfg->rlc_seed : 0;
  if (cfg && cfg->gident > TBG_GIDENT_CHUNKS) { delete c; return TBG_E_INVALID_ARG; }
  c->gident = cfg ? cfg->gident : (uint32_t)TBG_GIDENT_OFF;
  if (cfg && cfg->fb_window) c->fb_window = cfg->fb_window;
  if (cfg && cfg->subgroup_batch > TBG_SGB_OFF) { delete c; return TBG_E_INVALID_ARG; }
  if (cfg) c->sgb_mode = cfg->subgroup_batch;
  if (cfg && cfg->express_partials) c->express_max = cfg->express_partials;
  if (cfg && cfg->l0_duty_partials) c->l0_duty_partials = cfg->l0_duty_partials;
  if (cfg && cfg->l0_tail_partials) c->l0_tail_partials = cfg->l0_tail_partials;
  if (cfg && cfg->l0_msg_share) c->l0_msg_share = cfg->l0_msg_share;
  if (cfg && cfg->sgb_tri_partials) c->sgb_tri_partials = cfg->sgb_tri_partials;
  if (cfg && cfg->sgb_tri_m) c->sgb_tri_m = cfg->sgb_tri_m;
  if (!sgb_triple(c->sgb_tri_m) || c->sgb_tri_m > SGB_TRI_M_MAX || (c->sgb_tri_m & (c->sgb_tri_m - 1))) {
    delete c;
    return TBG_E_INVALID_ARG;
  }
  if (hipSetDevice(dev) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->retire_ev, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->keys_ready, hipEventDisableTiming) != hipSuccess) {
    if (c->retire_ev) hipEventDestroy(c->retire_ev);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return TBG_E_DEVICE;
  }
  // Every in-flight slot owns its two streams, so back-to-back submits
  // overlap on the GPU (one batch's latency-bound stages fill the CUs the
  // other leaves idle).
  uint32_t nslots = (cfg && cfg->slots) ? cfg->slots : 3;
  const uint32_t spp = (cfg && cfg->streams_per_slot > 1) ? cfg->streams_per_slot : 1;
  // The express slot takes one stream more; a configuration with no stream
  // left for it runs without one rather than being refused.
  if (nslots * spp + 1 > TBG_MAX_SLOT_STREAMS) c->express_max = TBG_EXPRESS_OFF;
  const bool express = c->express_max != TBG_EXPRESS_OFF;
  if (nslots > TBG_MAX_SLOTS || spp > 2 || nslots * spp + (express ? 1 : 0) > TBG_MAX_SLOT_STREAMS) {
    hipStreamDestroy(c->stream);
    hipEventDestroy(c->retire_ev);
    hipEventDestroy(c->keys_ready);
    delete c;
    return TBG_E_INVALID_ARG;
  }
  // (+ the express slot: one more slot, last, on a high-priority stream)
  c->slots.resize(nslots + (express ? 1 : 0));
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n_cu > 0)
    c->n_simd = (uint32_t)n_cu * 4u;
  // One stream per slot by default: the HIP runtime maps streams onto a
  // few hardware queues (GPU_MAX_HW_QUEUES, 4 by default), so concurrency
  // comes from several batches in flight, one queue each.  Two streams
  // per slot also overlap a batch's hash_to_G2 with its decode (lower
  // single-batch latency when queues are plentiful).
  const bool two = cfg && cfg->streams_per_slot >= 2;
  // (Per-slot stream priorities were measured within noise, round 3.)
  int prio_least = 0, prio_greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) prio_greatest = prio_least = 0;
  for (size_t k = 0; k < c->slots.size(); ++k) {
    auto& s = c->slots[k];
    s.express = express && k == nslots;
    auto mk = [&](hipStream_t* st) { return hipStreamCreateWithFlags(st, hipStreamNonBlocking); };
    if (s.express) {
      // A small batch's chain is ~50 short kernels in series: on a
      // high-priority queue their dispatches go ahead of the throughput
      // launches' pending workgroups instead of queueing behind them.
      if (hipStreamCreateWithPriority(&s.st, hipStreamNonBlocking, prio_greatest) != hipSuccess) {
        tbg_destroy(c);
        return TBG_E_DEVICE;
      }
      s.st2 = s.st;
    } else {
      if (mk(&s.st) != hipSuccess || (two && mk(&s.st2) != hipSuccess)) {
        tbg_destroy(c);
        return TBG_E_DEVICE;
      }
      if (!two) s.st2 = s.st;
    }
    for (auto& e : s.ev) hipEventCreate(&e);
    hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
  }
  *out = c;
  return TBG_OK;
}

void tbg_destroy(tbg_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  for (auto& s : c->slots) {
    if (s.st) hipStreamSynchronize(s.st);
    if (s.st2 && s.st2 != s.st) hipStreamSynchronize(s.st2);
    if (s.h_in) hipHostFree(s.h_in);
    if (s.h_out) hipHostFree(s.h_out);
    if (s.d_in) hipFree(s.d_in);
    if (s.d_work) hipFree(s.d_work);
    for (auto& e : s.ev)
      if (e) hipEventDestroy(e);
    if (s.done) hipEventDestroy(s.done);
    if (s.st2 && s.st2 != s.st) hipStreamDestroy(s.st2);
    if (s.st) hipStreamDestroy(s.st);
  }
  // the key tables are stream-ordered allocations of the utility stream
  if (c->stream) {
    for (void* p : {(void*)c->d_pk, (void*)c->d_xpk, (void*)c->d_pktab, (void*)c->d_pk_status})
      if (p) hipFreeAsync(p, c->stream);
    hipStreamSynchronize(c->stream);
    hipStreamDestroy(c->stream);
  }
  if (c->retire_ev) hipEventDestroy(c->retire_ev);
  if (c->keys_ready) hipEventDestroy(c->keys_ready);
  delete c;
}

uint32_t tbg_pubkey_count(const tbg_ctx* c) { return c ? c->n_pk : 0; }

int tbg_load_pubkeys(tbg_ctx* c, const uint8_t* pk48, uint32_t count, uint32_t* first_id, int32_t* status) {
  if (!c || (count && !pk48)) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (c->n_pk + (uint64_t)count > 0xFFFFFFF0ull) return TBG_E_INVALID_ARG;
  uint32_t need = c->n_pk + count;
  void* old_tabs[4] = {nullptr, nullptr, nullptr, nullptr};  // outgrown tables, freed below
  if (need > c->cap_pk) {
    // Stream-ordered allocations on the utility stream: no device-wide
    // synchronisation (hipMalloc / hipFree would wait for every batch in flight).
    uint32_t ncap = need + need / 2 + 1024;
    G1A* npk = nullptr;
    G1A* nxpk = nullptr;
    G1A* ntab = nullptr;
    int32_t* nst = nullptr;
    hipStream_t us = c->stream;
    if (hipMallocAsync((void**)&npk, sizeof(G1A) * (size_t)ncap, us) != hipSuccess) return TBG_E_OOM;
    if (hipMallocAsync((void**)&nxpk, sizeof(G1A) * (size_t)ncap, us) != hipSuccess) {
      hipFreeAsync(npk, us);
      return TBG_E_OOM;
    }
    if (hipMallocAsync((void**)&ntab, PK_TAB * sizeof(G1A) * (size_t)ncap, us) != hipSuccess) {
      hipFreeAsync(npk, us);
      hipFreeAsync(nxpk, us);
      return TBG_E_OOM;
    }
    if (hipMallocAsync((void**)&nst, sizeof(int32_t) * (size_t)ncap, us) != hipSuccess) {
      hipFreeAsync(npk, us);
      hipFreeAsync(nxpk, us);
      hipFreeAsync(ntab, us);
      return TBG_E_OOM;
    }
    if (c->n_pk) {
      HIP_TRY(hipMemcpyAsync(npk, c->d_pk, sizeof(G1A) * (size_t)c->n_pk, hipMemcpyDeviceToDevice, us));
      HIP_TRY(hipMemcpyAsync(nxpk, c->d_xpk, sizeof(G1A) * (size_t)c->n_pk, hipMemcpyDeviceToDevice, us));
      HIP_TRY(hipMemcpyAsync(ntab, c->d_pktab, PK_TAB * sizeof(G1A) * (size_t)c->n_pk, hipMemcpyDeviceToDevice, us));
      HIP_TRY(hipMemcpyAsync(nst, c->d_pk_status, sizeof(int32_t) * (size_t)c->n_pk, hipMemcpyDeviceToDevice, us));
    }
    old_tabs[0] = c->d_pk;
    old_tabs[1] = c->d_xpk;
    old_tabs[2] = c->d_pktab;
    old_tabs[3] = c->d_pk_status;
    c->d_pk = npk;
    c->d_xpk = nxpk;
    c->d_pktab = ntab;
    c->d_pk_status = nst;
    c->cap_pk = ncap;
  }
  if (first_id) *first_id = c->n_pk;
  uint8_t* d_bytes = nullptr;  // stream-ordered staging (freed on the same stream)
  if (count && hipMallocAsync((void**)&d_bytes, 48ull * count, c->stream) != hipSuccess) return TBG_E_OOM;
  int rc = TBG_OK;
  if (count == 0) goto ready;
  if (hipMemcpyAsync(d_bytes, pk48, 48ull * count, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = TBG_E_DEVICE;
  if (rc == TBG_OK) {
    launch_decode_pubkeys(d_bytes, count, c->d_pk + c->n_pk, c->d_xpk + c->n_pk, c->d_pk_status + c->n_pk, c->stream);
    launch_pubkey_tables(c->d_pk + c->n_pk, c->d_xpk + c->n_pk, c->d_pk_status + c->n_pk, count,
                         c->d_pktab + (size_t)PK_TAB * c->n_pk, c->stream);
    if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  }
  if (rc == TBG_OK && status &&
      hipMemcpyAsync(status, c->d_pk_status + c->n_pk, sizeof(int32_t) * count, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
    rc = TBG_E_DEVICE;
ready:
  // Submits order their slot streams after this event, not after the frees below.
  if (hipEventRecord(c->keys_ready, c->stream) != hipSuccess) rc = TBG_E_DEVICE;
  if (old_tabs[0]) {
    // Batches already queued on the slot streams captured the old tables'
    // addresses: their free is ordered after everything queued so far on
    // every slot stream (one event recorded per stream, waited on by the
    // utility stream), without blocking the host or the device.
    for (auto& sl : c->slots)
      for (hipStream_t q : {sl.st, sl.st2}) {
        if (!q || (q == sl.st2 && sl.st2 == sl.st)) continue;
        if (hipEventRecord(c->retire_ev, q) != hipSuccess || hipStreamWaitEvent(c->stream, c->retire_ev, 0) != hipSuccess)
          rc = TBG_E_DEVICE;
      }
    for (void* p : old_tabs) hipFreeAsync(p, c->stream);
  }
  if (d_bytes) hipFreeAsync(d_bytes, c->stream);
  if (hipEventSynchronize(c->keys_ready) != hipSuccess) rc = TBG_E_DEVICE;
  if (rc == TBG_OK) c->n_pk += count;
  return rc;
}

// The aggregation the checks will mostly confirm (every candidate valid),
// enqueued mid-chain so the launch's tail is the verification plus the redo of
// the few duties with an invalid partial (none after a level-0 pass).
static void spec_aggregation(const DevBatch& B, hipStream_t st) {
  launch_lagrange(B, st, true);
  launch_aggregate(B, st, true);
  launch_aggregate_finish(B, st, true);
}

// The kernel chain of one batch.  Per-message work (hash_to_G2, H(m) lines)
// runs on st2 concurrently with the per-signature work (decode, RLC sums and
// group lines) on st; the product checks join both.
// Events: ev[0] start, ev[1] decode done, ev[2] combine done, ev[3]/ev[4]
// hash start/done and ev[5] H lines done (st2), ev[6] verify start, ev[7]
// verify done, ev[8] lagrange done, ev[9] aggregate done, ev[10] decode start.
// `stage` enqueues one part (0: start + the first chain, 1: the second
// chain, 2: the checks and the aggregation; -1: all three): a replay of
// several slots enqueues stage 0 of every slot before stage 1 of any, so the
// slots' first kernels start together instead of one chain's enqueue time
// (~100 launches) apart.
// TBG_OP_AGGREGATE_VERIFY: the recombination is on the path -- decode,
// lagrange (ev[8]), aggregate (ev[9]), then the checks of the batch's view V
// (aggver_view: one candidate per duty, the affine aggregate), whose key side
// ends at ev[2]; after the join, V's check levels and their verdicts as duty
// codes, ev[6] to ev[7], the chain's end (chain_end).  The per-message chain
// runs on st2 beside all of it.  Nothing is speculative.
static int launch_chain(tbg_ctx* c, const Slot& sl, const DevBatch& B, hipEvent_t* ev, int stage = -1) {
  hipStream_t st = sl.st, st2 = sl.st2;
  const bool verify = B.op != TBG_OP_AGGREGATE;
  const bool aggver = B.op == TBG_OP_AGGREGATE_VERIFY;
  const DevBatch V = checked_batch(B);  // (B itself but for TBG_OP_AGGREGATE_VERIFY)
  const G1A* pk = (const G1A*)c->d_pk;
  // With one stream per slot the two independent chains run one after the
  // other, the per-message chain first (running the per-signature chain
  // first on odd slots was measured no better, round 2).
  // The aggregation runs speculatively as soon as the candidates are final
  // (every candidate taken as valid), off the launch's serial tail, while
  // level 0 is on (on every VERIFY_AGGREGATE chain, redoing only the duties
  // with an invalid partial, was measured slower, round 5).
  const bool spec = B.op == TBG_OP_VERIFY_AGGREGATE && B.rlc_batch && B.rlc_group;
  auto msg_chain = [&]() -> int {
    HIP_TRY(hipEventRecord(ev[3], st2));
    if (verify) launch_hash_msgs(B, st2);
    HIP_TRY(hipEventRecord(ev[4], st2));
    if (verify) launch_h_lines(B, st2);
    HIP_TRY(hipEventRecord(ev[5], st2));
    return TBG_OK;
  };
  auto sig_chain = [&]() -> int {
    HIP_TRY(hipEventRecord(ev[10], st));
    launch_decode_sigs(B, st);  // zeroes B.counters (and level 0's bucket sizes) first
    HIP_TRY(hipEventRecord(ev[1], st));
    if (aggver) {
      launch_lagrange(B, st);
      HIP_TRY(hipEventRecord(ev[8], st));
      launch_aggregate(B, st);
      launch_aggregate_finish(B, st);
      HIP_TRY(hipEventRecord(ev[9], st));
      launch_aggver_candidates(B, V, st);  // zeroes V.counters (and level 0's bucket sizes) first
      launch_rlc_prepare(V, pk, (const G1A*)c->d_pktab, (const int32_t*)c->d_pk_status, c->n_pk, st);
      HIP_TRY(hipEventRecord(ev[2], st));
      return TBG_OK;
    }
    // The aggregation a level-0 pass will confirm runs as soon as the
    // candidates are final (after the key checks), before the bucket MSM:
    // placed after it, its small kernels waited behind the other launches'
    // long Miller waves for a free slot and delayed this launch's own Miller
    // kernel (k_lagrange<true> 7.7 ms instead of 0.05, profiles/r04/base/
    // timeline_s20.txt).
    if (verify)
      launch_rlc_prepare(B, pk, (const G1A*)c->d_pktab, (const int32_t*)c->d_pk_status, c->n_pk, st,
                         spec ? spec_aggregation : nullptr);
    HIP_TRY(hipEventRecord(ev[2], st));
    return TBG_OK;
  };
  int rc;
  if (stage < 0 || stage == 0) {
    HIP_TRY(hipEventRecord(ev[0], st));
    HIP_TRY(hipStreamWaitEvent(st2, ev[0], 0));
    if ((rc = msg_chain()) != TBG_OK) return rc;
  }
  if (stage < 0 || stage == 1)
    if ((rc = sig_chain()) != TBG_OK) return rc;
  if (stage >= 0 && stage != 2) return TBG_OK;
  HIP_TRY(hipStreamWaitEvent(st, ev[5], 0));
  HIP_TRY(hipEventRecord(ev[6], st));
  if (aggver) {
    launch_rlc_check(V, pk, (const G1A*)c->d_pktab, (const int32_t*)c->d_pk_status, c->n_pk, st);
    launch_aggver_status(B, V, st);
    HIP_TRY(hipEventRecord(ev[7], st));
    HIP_TRY(hipGetLastError());
    return TBG_OK;
  }
  if (verify) launch_rlc_check(B, pk, (const G1A*)c->d_pktab, (const int32_t*)c->d_pk_status, c->n_pk, st);
  HIP_TRY(hipEventRecord(ev[7], st));
  if (B.op != TBG_OP_VERIFY) launch_lagrange(B, st);
  HIP_TRY(hipEventRecord(ev[8], st));
  launch_aggregate(B, st);
  if (B.op != TBG_OP_VERIFY) launch_aggregate_finish(B, st);
  HIP_TRY(hipEventRecord(ev[9], st));
  HIP_TRY(hipGetLastError());
  return TBG_OK;
}

// The event a chain ends with (launch_chain).
static int chain_end(uint32_t op) { return op == TBG_OP_AGGREGATE_VERIFY ? 7 : 9; }

// [decode, hash, combine, H lines, verify, lagrange, aggregate, total]
static void chain_times(hipEvent_t* e, float* ms, uint32_t op) {
  const bool aggver = op == TBG_OP_AGGREGATE_VERIFY;  // (the recombination before the checks)
  hipEventElapsedTime(&ms[0], e[10], e[1]);
  hipEventElapsedTime(&ms[1], e[3], e[4]);
  hipEventElapsedTime(&ms[2], e[aggver ? 9 : 1], e[2]);
  hipEventElapsedTime(&ms[3], e[4], e[5]);
  hipEventElapsedTime(&ms[4], e[6], e[7]);
  hipEventElapsedTime(&ms[5], e[aggver ? 1 : 7], e[8]);
  hipEventElapsedTime(&ms[6], e[8], e[9]);
  hipEventElapsedTime(&ms[7], e[0], e[chain_end(op)]);
}

static int validate(const tbg_batch* b) {
  if (!b) return TBG_E_INVALID_ARG;
  if (b->op < TBG_OP_VERIFY || b->op > TBG_OP_AGGREGATE_VERIFY) return TBG_E_INVALID_ARG;
  if (b->n_duties == 0) return TBG_E_INVALID_ARG;
  if (!b->duty_first || (b->n_partials && (!b->sigs || !b->identifiers))) return TBG_E_INVALID_ARG;
  if (b->duty_first[0] != 0 || b->duty_first[b->n_duties] != b->n_partials) return TBG_E_INVALID_ARG;
  for (uint32_t d = 0; d < b->n_duties; ++d) {
    if (b->duty_first[d + 1] < b->duty_first[d]) return TBG_E_INVALID_ARG;
    if (b->duty_first[d + 1] - b->duty_first[d] > 255) return TBG_E_INVALID_ARG;
  }
  if (b->op != TBG_OP_AGGREGATE) {
    // (pubkey_ids: [n_partials]; under TBG_OP_AGGREGATE_VERIFY [n_duties], one group key per
    // duty -- required either way; duty_threshold is not read under that op)
    if (!b->msg_off || !b->duty_msg || !b->pubkey_ids || b->n_msgs == 0) return TBG_E_INVALID_ARG;
    if (b->msg_off[0] != 0) return TBG_E_INVALID_ARG;
    for (uint32_t m = 0; m < b->n_msgs; ++m)
      if (b->msg_off[m + 1] < b->msg_off[m]) return TBG_E_INVALID_ARG;
    if (b->msg_off[b->n_msgs] && !b->msgs) return TBG_E_INVALID_ARG;
    for (uint32_t d = 0; d < b->n_duties; ++d)
      if (b->duty_msg[d] >= b->n_msgs) return TBG_E_INVALID_ARG;
  }
  if (b->op == TBG_OP_VERIFY_AGGREGATE && !b->duty_threshold) return TBG_E_INVALID_ARG;
  return TBG_OK;
}

// The slot and part a ticket names.  want_busy: the part must be pending
// (collect / poll) or the slot idle (replay / fetch of a collected batch).
static Slot* find_ticket(tbg_ctx* c, tbg_ticket t, bool want_pending, Part** part) {
  for (auto& x : c->slots)
    for (auto& q : x.parts)
      if (q.ticket == t && (want_pending ? q.pending : !x.busy)) {
        if (part) *part = &q;
        return &x;
      }
  return nullptr;
}

static int submit_impl(tbg_ctx* c, const tbg_batch* const* bs, uint32_t n_batches, tbg_ticket* tickets,
                       const uint32_t* set_first, uint32_t n_sets);

int tbg_submit(tbg_ctx* c, const tbg_batch* b, tbg_ticket* ticket) { return tbg_submit_group(c, &b, 1, ticket); }

int tbg_submit_group(tbg_ctx* c, const tbg_batch* const* bs, uint32_t n_batches, tbg_ticket* tickets) {
  return submit_impl(c, bs, n_batches, tickets, nullptr, 0);
}

int tbg_submit_sets(tbg_ctx* c, const tbg_batch* b, const uint32_t* set_first, uint32_t n_sets, tbg_ticket* ticket) {
  if (!c || !b || !set_first || !ticket) return TBG_E_INVALID_ARG;
  int rc = validate(b);
  if (rc != TBG_OK) return rc;
  if (b->op != TBG_OP_VERIFY || set_first[0] != 0 || set_first[n_sets] != b->n_duties) return TBG_E_INVALID_ARG;
  for (uint32_t k = 0; k < n_sets; ++k)
    if (set_first[k + 1] < set_first[k]) return TBG_E_INVALID_ARG;
  return submit_impl(c, &b, 1, ticket, set_first, n_sets);
}

// Level-0 launch shape.  The level-0 Miller kernel's
// waves are long -- one hexad = the whole 68-step loop over C duties -- and
// issue-bound at ONE wave per SIMD: a lone wave runs its loop in 3.6 ms at
// C = 4, two sharing a SIMD take 6.8 ms each (profiles/r05/waves), so the
// kernel's time is ~ceil(waves / SIMDs) hexad lengths, and a launch whose
// waves spill just past a multiple of the SIMD count pays a whole hexad
// length for the remainder: config 4's 125k-duty shard at (G, C) = (16, 4)
// is 3,126 waves on 1,024 SIMDs.  A hexad of C duties costs 62 squarings +
// 68 C line products, w(C) = 0.95 M + 1.39 M C u32 mul-adds
// (profiles/work_model.json, l0_chunk_*), so fewer, longer hexads win where
// they save a unit: (16, 8) halves the squarings, (14, 7) runs 125k duties
// in 2 units instead of 4.  The rule picks the cheapest of (16, 4), (16, 8),
// (14, 7) by ceil(waves / SIMDs) x w(C) -- 100k duties keep (16, 4), 125k
// take (14, 7), 160k (16, 8), as the A/B runs of profiles/r05/chunk8_ab,
// shape_ab and sqrt_x2_ab measured best.  A configured group size G keeps G
// (C = 4 or 8 only).  tbg_replay_plan applies it to the duties of the
// launches it runs together (their Miller kernels share the SIMDs).
static double l0_shape_cost(uint64_t nd, uint32_t n_simd, uint32_t g, uint32_t ch) {
  const uint64_t hexads = (uint64_t)((nd + g - 1) / g) * ((g + ch - 1) / ch);
  const uint64_t waves = (hexads + 9) / 10;
  return (0.948 + 1.395 * ch) * (double)((waves + n_simd - 1) / n_simd);
}
// Round 6: with the group size free, every chunk C of
// 5 .. 10 duties is a candidate too, as (G, C) = (C, C) -- one chunk per
// group -- so the hexads can fill whole wave-slot rounds: the 20-step plan's
// 200k duties take (10, 10) (2,000 waves: 2 rounds) instead of (14, 7) (2,858
// waves: 3 rounds; +2.6 % at the driver shape, profiles/r06/shape), config
// 3's 100k (10, 10) instead of (16, 4) (Miller 8.0 vs 9.4 ms).  Chunks of 13
// and 16 duties were measured far off the model (a round of ~1,000 lone
// waves: (16, 16) 20.4 ms vs (16, 8) 12.2 ms at 160k duties, (13, 13) 16.8
// vs (14, 7) 11.0 ms at 125k: the C line loads of a step are not hidden by a
// second wave), so C stops at L0_SHAPE_MAX_C.
// `fits` (a replay's arenas, below) drops the candidates a launch cannot hold.
static bool l0_fits_any(uint32_t, uint32_t) { return true; }
static void l0_shape(uint64_t nd, uint32_t n_simd, bool g_free, uint32_t& G, uint32_t& C,
                     const std::function<bool(uint32_t, uint32_t)>& fits) {
  C = 4;
  if (G < 8) return;
  constexpr uint32_t L0_SHAPE_MAX_C = 10;
  uint32_t cand[3 + L0_SHAPE_MAX_C][2] = {{g_free ? 16u : G, 4}, {g_free ? 16u : G, 8}, {14, 7}};
  uint32_t n_cand = g_free ? 3u : 2u;
  for (uint32_t c = 5; g_free && c <= L0_SHAPE_MAX_C; ++c) {
    cand[n_cand][0] = c;
    cand[n_cand][1] = c;
    ++n_cand;
  }
  double best = 1e300;
  const uint32_t G0 = G;
  for (uint32_t k = 0; k < n_cand; ++k) {
    if (!fits(cand[k][0], cand[k][1])) continue;
    const double cost = l0_shape_cost(nd, n_simd, cand[k][0], cand[k][1]);
    if (cost < best - 1e-9) {
      best = cost;
      G = cand[k][0];
      C = cand[k][1];
    }
  }
  if (best == 1e300) G = G0;  // (nothing fits: the caller keeps its shapes)
}
// A launch of nd duties (a prefix of its slot's device batch) at (G, C) fits
// the slot's arena, whose group / chunk sections were sized at submit for
// the slot's nd0 duties at (G0, C0) (tbg_submit_group).
static bool l0_shape_fits(uint32_t nd0, uint32_t G0, uint32_t C0, uint32_t nd, uint32_t G, uint32_t C) {
  const uint64_t ng0 = (nd0 + G0 - 1) / G0, nch0 = (G0 + C0 - 1) / C0;
  const uint64_t ng = (nd + G - 1) / G, nch = (G + C - 1) / C;
  // every group / chunk section of the arena (tbg_submit_group's w_cf,
  // w_gidf: ng (nch + 1); w_cl, w_cfe, w_cidl: ng nch -- ADVICE r05: the
  // max() below alone let nd0 hide an overflow of these; w_cidp: ng nch C;
  // w_gidp: ng G; w_pend: max(ng nch, nd); grp_f: ng)
  return ng <= ng0 && ng * (nch + 1) <= ng0 * (nch0 + 1) && ng * nch <= ng0 * nch0 && ng * nch * C <= ng0 * nch0 * C0 &&
         ng * G <= ng0 * G0 && std::max(ng * nch, (uint64_t)nd) <= std::max(ng0 * nch0, (uint64_t)nd0) &&
         (G <= 64) == (G0 <= 64);
}

// Batched subgroup test plan from the non-subgroup share `rho` of the
// collected partials.  Per signature, in units of one
// per-signature test (psi(s) == [x] s: 63 doublings + 5 additions): the 16.6
// bucket additions with the sort and running sums 0.55 (measured: k_sgb_*
// 0.47-0.57 of k_subgroup_sigs' time per signature, profiles/r06/sgb), the
// group's 18 tests 1.1 x 18 / m (each on a lone lane pair), and the failed
// groups' members tested alone 1 - (1 - rho)^m.  The group size m is the
// cheapest power of two in [SGB_M_MIN, SGB_M]; the test runs while that
// costs under 0.95 of testing every signature alone -- up to rho ~ 2.5e-3
// (TBG_SGB_AUTO_MAX).  Clean traffic keeps m = 1,024; config 5's 1.25e-3
// takes m = 128 (at 1,024, 72 % of its groups would fail).  The 0.55 is the
// classic schedule's; the paired schedule of groups >= SGB_PAIR_M
// (tbls_launch.h) is cheaper, which only widens the test's margin, and the
// sizes this plan picks are left as they were.
static bool sgb_plan(double rho, uint32_t& m) {
  double best = 1e9;
  m = SGB_M;
  for (uint32_t k = SGB_M; k >= SGB_M_MIN; k >>= 1) {
    const double cost = 0.55 + 1.1 * (double)SGB_K / k + (1.0 - std::pow(1.0 - std::min(rho, 1.0), (double)k));
    if (cost < best - 1e-12) {
      best = cost;
      m = k;
    }
  }
  return best < 0.95;
}

// The triple schedule (tbls_launch.h sgb_triple) in the same units.  Whether
// its arithmetic pays at a launch's size is the threshold's business
// (tbg_config.sgb_tri_partials, set from an A/B like l0_duty_partials): the
// count model (tools/sgb_pair_model.py) has bucket
// additions, ranked slots and reductions at 7.30 per member in groups of
// 16,384 against the paired 11.66 at 1,024, so 0.55 x (1 - 7.30 / 11.66) =
// 0.21 less per signature.  What the plan weighs is the term that grows with
// the group: a failed group's members are tested alone, 1 - (1 - rho)^m of
// them, against the same term at the size `m_small` that sgb_plan picked.
// The triple schedule runs while that difference stays under the modelled
// saving -- rho up to ~1.4e-5 at 16,384, the clean regime; any measurable
// non-subgroup share falls back to the paired sizes exactly as before.
static bool sgb_plan_triple(double rho, uint32_t m_small, uint32_t m_tri) {
  const double r = std::min(rho, 1.0);
  const double extra = std::pow(1.0 - r, (double)m_small) - std::pow(1.0 - r, (double)m_tri) +
                       1.1 * (double)SGB_K * (1.0 / m_tri - 1.0 / m_small);
  return extra < 0.55 * (1.0 - 7.30 / 11.66);
}
// The launch's group size: sgb_plan's, or the triple schedule's in a clean
// launch of at least sgb_tri_partials partials.  (A replayed prefix asks
// again with its own partial count.)
static uint32_t sgb_group_size(const tbg_ctx* c, uint32_t np, uint32_t m_small, bool clean_tri) {
  return clean_tri && np >= c->sgb_tri_partials ? c->sgb_tri_m : m_small;
}

// Device duties of a set launch at group size G: every non-empty set starts on
// a multiple of G (the duties between are empty padding), so no level-1 group
// holds duties of two sets.
static uint64_t sets_padded(const uint32_t* set_first, uint32_t n_sets, uint32_t G) {
  uint64_t e = 0;
  for (uint32_t k = 0; k < n_sets; ++k) {
    const uint32_t n = set_first[k + 1] - set_first[k];
    if (n) e = (e + G - 1) / G * G + n;
  }
  return e;
}

static int submit_impl(tbg_ctx* c, const tbg_batch* const* bs, uint32_t n_batches, tbg_ticket* tickets,
                       const uint32_t* set_first, uint32_t n_sets) {
  if (!c || !bs || !tickets || n_batches == 0) return TBG_E_INVALID_ARG;
  int rc;
  for (uint32_t k = 0; k < n_batches; ++k) {
    if ((rc = validate(bs[k])) != TBG_OK) return rc;
    if (bs[k]->op != bs[0]->op) return TBG_E_INVALID_ARG;  // one kernel chain per device batch
  }
  const uint32_t op = bs[0]->op;
  const bool verify = op != TBG_OP_AGGREGATE;
  // TBG_OP_AGGREGATE_VERIFY: the checks run on the batch's view (aggver_view), one
  // candidate per duty, so every array of the check levels is sized by duties (vp below)
  // and the per-duty key ids are packed by duty count
  const bool aggver = op == TBG_OP_AGGREGATE_VERIFY;
  if (aggver && set_first) return TBG_E_INVALID_ARG;
  uint64_t nd64 = 0, np64 = 0, nm64 = 0, mb64 = 0;
  for (uint32_t k = 0; k < n_batches; ++k) {
    nd64 += bs[k]->n_duties;
    np64 += bs[k]->n_partials;
    if (verify) {
      nm64 += bs[k]->n_msgs;
      mb64 += bs[k]->msg_off[bs[k]->n_msgs];
    }
  }
  if (np64 > 0x7FFFFFFFull || nd64 > 0x7FFFFFFFull || nm64 > 0x7FFFFFFFull || mb64 > 0xFFFFFFFFull)
    return TBG_E_INVALID_ARG;
  std::unique_lock<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  // Least recently used free slot: a collected batch stays resident (for
  // tbg_replay / tbg_fetch) until every other slot has been reused.  A batch
  // of at most express_max partials takes the express slot when it is free.
  Slot* s = nullptr;
  const bool small = np64 <= c->express_max;
  for (auto& x : c->slots)
    if (x.express && small && !x.busy) s = &x;
  if (!s)
    for (auto& x : c->slots)
      if (!x.express && !x.busy && (!s || x.ticket < s->ticket)) s = &x;
  if (!s) return TBG_E_BUSY;

  const uint32_t np = (uint32_t)np64, nm = (uint32_t)nm64;
  const size_t msg_bytes = (size_t)mb64;
  if (c->rlc_auto)
    c->rlc_group = c->invalid_ema < TBG_RLC_AUTO_TO8 ? 16 : c->invalid_ema < TBG_RLC_AUTO_TO4 ? 8 : 4;
  uint32_t G = verify ? c->rlc_group : 0;
  if (set_first) {
    // An unconfigured group size shrinks (to 8, then 4) while the sets'
    // padding would pass 1/8 of the duties: a launch of small sets keeps its
    // groups full instead of checking mostly padding.
    while (c->rlc_auto && G > 4 && sets_padded(set_first, n_sets, G) > nd64 + nd64 / 8) G /= 2;
    nd64 = sets_padded(set_first, n_sets, G ? G : 1);  // (>= the caller's duties: validate() wants one at least)
    if (nd64 > 0x7FFFFFFFull) return TBG_E_INVALID_ARG;
  }
  const uint32_t nd = (uint32_t)nd64;
  const uint32_t vp = aggver ? nd : np;  // candidates of the check levels

  // ---- input arena layout (16-byte aligned sections) ----
  size_t o = 0;
  auto sec = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 16); return at; };
  size_t o_msgs = sec(msg_bytes);
  size_t o_msg_off = sec(4ull * (nm + 1));
  size_t o_duty_msg = sec(4ull * nd);
  size_t o_duty_first = sec(4ull * (nd + 1));
  size_t o_thr = sec(4ull * nd);
  size_t o_pduty = sec(4ull * np);
  size_t o_sigs = sec(96ull * np);
  size_t o_ids = sec(np);
  size_t o_pk = sec(4ull * vp);
  size_t o_dset = sec(set_first ? 4ull * nd : 0);
  size_t o_iota = sec(aggver ? 4ull * (nd + 1) : 0);
  // Level 0 by message (bls_l0msg.h): the duties sorted by message and the
  // chunk plan, packed with the inputs.  Reserved whenever a fused level 0
  // may run with the knob on, whatever the launch's own duties per message:
  // a replayed prefix decides from its own (l0_by_msg).  The work arena's
  // sections follow below, once `fused` is known; this side is sized by the
  // same conditions except the subgroup test's, which only shrink it.
  // Nothing is reserved or sorted when no prefix of the caller batches
  // reaches the share (one message per duty: the headline workload).
  bool l0m_in = false;
  if (verify && !aggver && c->rlc_group != 0 && c->rlc_batch != TBG_RLC_L0_OFF && c->sgb_mode != TBG_SGB_OFF &&
      c->l0_msg_share != TBG_L0_MSG_NEVER && np >= SGB_MIN_PARTIALS) {
    uint64_t cd = 0, cm = 0;
    for (uint32_t k = 0; k < n_batches; ++k) {
      cd = set_first ? nd : cd + bs[k]->n_duties;
      cm += bs[k]->n_msgs;
      l0m_in = l0m_in || cm * c->l0_msg_share <= cd;
    }
  }
  const size_t l0m_chunks = l0m_in ? (size_t)l0m_chunk_bound(nm, nd) : 0;
  size_t o_mfirst = sec(l0m_in ? 4ull * (nm + 1) : 0);
  size_t o_mduty = sec(l0m_in ? 4ull * nd : 0);
  size_t o_cfirst = sec(l0m_in ? 4ull * (nm + 1) : 0);
  size_t o_cmsg = sec(l0m_in ? 4ull * l0m_chunks : 0);
  size_t in_bytes = o;
  // ---- work/output arena ----
  o = 0;
  size_t w_sig_aff = sec(sizeof(G2A) * (size_t)np);
  size_t w_h_aff = sec(sizeof(G2A) * (size_t)nm);
  size_t w_h_st = sec(4ull * nm);
  size_t w_h_jac = sec(3 * sizeof(G2J) * (size_t)nm);  // H(m) + the cofactor clearing's two temporaries
  size_t w_lam = sec(32ull * np);
  // The fallback levels' lines share one buffer of fb_w list positions,
  // consumed in passes (DevBatch::fb_window): a slot no longer holds 22.8 KB
  // per partial for lists that a clean batch leaves empty.
  const uint32_t fb_w = verify ? std::max<uint32_t>(1u, std::min<uint32_t>(c->fb_window, vp)) : 0u;
  size_t w_sl = sec(4ull * LINES_WORDS * fb_w);
  size_t w_hl = sec(4ull * LINES_WORDS * nm);
  // Level 0 while the collected batches are clean (or as configured): one
  // failed level-0 check costs its own work on top of the group levels.
  const bool l0 = G != 0 && vp < (1u << 28) &&
                  (c->rlc_batch == TBG_RLC_L0_ON || (c->rlc_batch == TBG_RLC_L0_AUTO && c->invalid_ema < TBG_RLC_AUTO_L0));
  uint32_t C = c->rlc_chunk;
  // (a set launch keeps its G: the sets are padded to it)
  if (l0 && c->chunk_auto) l0_shape(nd, c->n_simd, !set_first && c->rlc_auto && G == 16, G, C, l0_fits_any);
  if (C > G) C = G ? G : 1;
  const uint32_t ng = G ? (nd + G - 1) / G : 0;
  const uint32_t nch = G ? (G + C - 1) / C : 0;
  size_t w_pp = sec(G ? sizeof(G1J) * (size_t)vp : 0);
  size_t w_ps = sec(G ? sizeof(G2J) * (size_t)vp : 0);
  size_t w_cf = sec(G ? 4ull * 3 * 4 * NL * ng * (nch + 1) : 0);
  size_t w_cl = sec(G > 1 ? 4ull * ng * nch : 0);

  size_t w_dvp = sec(G ? sizeof(G1A) * (size_t)nd : 0);
  size_t w_dvs = sec(G ? sizeof(G2J) * (size_t)nd : 0);
  size_t w_dvst = sec(G ? 4ull * nd : 0);
  size_t w_gst = sec(4ull * ng);
  size_t w_gl = sec(4ull * LINES_WORDS * ng);
  size_t w_cnt = sec(4ull * CNT_WORDS);
  size_t w_pl = sec(verify ? 4ull * vp : 0);
  size_t w_dvfe = sec(G > 1 ? 4ull * 3 * 4 * NL * nd : 0);
  size_t w_pend = sec(G ? sizeof(G2A) * (size_t)std::max<size_t>(std::max<size_t>(ng, (size_t)ng * nch), nd) : 0);
  size_t w_cfe = sec(G > 1 ? 4ull * 3 * 4 * NL * ng * nch : 0);
  size_t w_cidl = sec(G > 1 ? 4ull * ng * nch : 0);
  size_t w_cidp = sec(G > 1 ? sizeof(G1A) * (size_t)ng * nch * C : 0);

  size_t w_gfe = sec(G > 1 ? 4ull * 3 * 4 * NL * ng : 0);
  size_t w_gidl = sec(G > 1 ? 4ull * ng : 0);
  size_t w_gidp = sec(G > 1 ? sizeof(G1A) * (size_t)ng * G : 0);
  size_t w_gidf = sec(G > 1 ? 4ull * 3 * 4 * NL * ng * (nch + 1) : 0);
  size_t w_idl = sec(G > 1 ? 4ull * nd : 0);
  size_t w_idp = sec(G > 1 ? sizeof(G1A) * (size_t)nd : 0);
  size_t w_bpt = sec(l0 ? sizeof(G2A) : 0);
  size_t w_blines = sec(l0 ? 4ull * LINES_WORDS : 0);
  size_t w_bf = sec(l0 ? 4ull * 3 * 4 * NL : 0);
  size_t w_gf = sec(l0 ? 4ull * 3 * 4 * NL * grp_f_entries(ng) : 0);
  // level 1's group MSM (k_gmsm.hip): entries, offsets, bucket sums, leads, the failed groups' candidates
  size_t w_gmoff = sec(G ? 4ull * (GM_BUCKETS + 1) * ng : 0);
  size_t w_gment = sec(G ? 64ull * vp : 0);
  size_t w_gmpart = sec(G ? sizeof(G2J) * GM_BUCKETS * (size_t)ng : 0);
  size_t w_gmlead = sec(G ? 4ull * ng : 0);
  size_t w_gmlist = sec(G ? 4ull * vp : 0);
  size_t w_gmhist = sec(G ? 4ull * 256 : 0);
  size_t w_gmorder = sec(G ? 4ull * GM_BUCKETS * ng : 0);
  // Batched subgroup test while the collected batches carry (almost) no
  // non-subgroup signature: groups of 1,024 partials, a failed group's members
  // tested alone (k_sgb.hip); small batches test every signature alone.
  uint32_t sgb_m = SGB_M;
  const bool sgb = np >= SGB_MIN_PARTIALS && c->sgb_mode != TBG_SGB_OFF &&
                   (sgb_plan(c->nonsub_ema, sgb_m) || c->sgb_mode == TBG_SGB_ON);
  // A clean launch of at least sgb_tri_partials partials takes the triple
  // schedule's large groups.  A replayed prefix below the threshold goes back
  // to sgb_m_small, so such a launch's sections hold either layout.
  const uint32_t sgb_m_small = sgb_m;
  const bool sgb_tri_ok = sgb && sgb_plan_triple(c->nonsub_ema, sgb_m_small, c->sgb_tri_m);
  sgb_m = sgb_group_size(c, np, sgb_m_small, sgb_tri_ok);
  const bool sgb_tri = sgb_triple(sgb_m);
  const uint32_t sgb_split = sgb_tri ? 1u : sgb_split_for(sgb_m);
  const size_t n_sg = sgb ? sgb_groups(np, sgb_m) : 0;
  const size_t n_sg_small = sgb ? sgb_groups(np, sgb_m_small) : 0;  // (the most groups a prefix can have)
  auto sgsec = [&](auto&& per_group) {  // a section of per_group(m) units per group, in either layout
    return std::max<size_t>(per_group(sgb_m) * n_sg, sgb_tri ? per_group(sgb_m_small) * n_sg_small : 0);
  };
  size_t w_sgoff = sec(4ull * sgsec([](uint32_t m) { return (size_t)sgb_off_stride(m); }));
  size_t w_sgent = sec(4ull * sgsec([](uint32_t m) { return (size_t)sgb_ent_stride(m); }));
  size_t w_sgpart = sec(sizeof(G2J) * sgsec([](uint32_t m) { return (size_t)sgb_part_stride(m); }));
  size_t w_sgrank = sec(4ull * sgsec([](uint32_t m) { return (size_t)sgb_rank_stride(m); }));
  size_t w_sgcode = sec(sgb_tri ? 4ull * SGB_TRIPLES * np : 0);
  size_t w_sgbad = sec(4ull * std::max(n_sg, sgb_tri ? n_sg_small : 0));
  // Level 0's signature side: with the batched test on, S comes from the
  // test's sums (l0_fused, tbls_launch.h; a replayed prefix of the launch
  // keeps both flags, so it takes the same path) and the bucket MSM's
  // arrays are not needed; otherwise the bucket MSM of k_msm.hip.
  // (TBG_OP_AGGREGATE_VERIFY: the subgroup test is the partials', the level 0 the view's,
  // which has no digits to take S from -- always the bucket MSM, over the duties)
  const bool fused = l0 && sgb && !aggver;
  const bool msm = l0 && !fused;
  size_t w_mr = sec(msm ? 8ull * vp : 0);
  size_t w_moff = sec(msm ? 4ull * (MSM_BUCKETS + 1) : 0);
  size_t w_mcur = sec(msm ? 4ull * MSM_BUCKETS : 0);
  size_t w_ment = sec(msm ? 16ull * vp : 0);
  size_t w_mbkt = sec(msm ? sizeof(G2J) * (size_t)MSM_BUCKETS : 0);
  size_t w_mpart = sec(msm ? sizeof(G2J) * (size_t)MSM_BUCKETS * MSM_SPLIT : 0);
  size_t w_msum = sec(msm ? sizeof(G2J) * (size_t)MSM_SUM_ENTRIES : 0);
  size_t w_sgt = sec(fused ? sizeof(G2J) * sgsec([](uint32_t m) { return (size_t)sgb_t_slices(m); }) : 0);
  size_t w_l0fsum = sec(fused ? sizeof(G2J) * std::max<size_t>(l0f_sum_entries((uint32_t)n_sg, sgb_m),
                                                               sgb_tri ? l0f_sum_entries((uint32_t)n_sg_small, sgb_m_small) : 0)
                              : 0);
  size_t w_l0fu = sec(fused ? 16ull * np : 0);
  // level 0 by message: chunk sums and their member counts, Q_m, the messages' states
  const bool l0m = fused && l0m_in;
  size_t w_l0mpart = sec(l0m ? sizeof(G1J) * l0m_chunks : 0);
  size_t w_l0mcnt = sec(l0m ? 4ull * l0m_chunks : 0);
  size_t w_l0mq = sec(l0m ? sizeof(G1A) * (size_t)nm : 0);
  size_t w_l0mst = sec(l0m ? 4ull * nm : 0);
  size_t w_aacc = sec(op != TBG_OP_VERIFY ? sizeof(G2J) * (size_t)nd : 0);
  size_t w_alist = sec(op != TBG_OP_VERIFY ? 4ull * nd : 0);
  size_t w_aaff = sec(aggver ? sizeof(G2A) * (size_t)nd : 0);
  size_t w_avst = sec(aggver ? 4ull * nd : 0);
  size_t w_avcnt = sec(aggver ? 4ull * CNT_WORDS : 0);
  size_t w_out = o;  // outputs are contiguous so one D2H copy brings them back
  size_t w_pst = sec(4ull * np);
  size_t w_dst = sec(4ull * nd);
  size_t w_agg = sec(96ull * nd);
  size_t w_sst = sec(set_first ? 4ull * ((size_t)n_sets + SET_TAIL) : 0);
  size_t work_bytes = o;
  size_t out_bytes = work_bytes - w_out;

  if ((rc = grow_pinned(&s->h_in, &s->h_in_cap, in_bytes)) != TBG_OK) return rc;
  if ((rc = grow_pinned(&s->h_out, &s->h_out_cap, out_bytes)) != TBG_OK) return rc;
  if ((rc = grow_device(&s->d_in, &s->d_in_cap, in_bytes)) != TBG_OK) return rc;
  if ((rc = grow_device(&s->d_work, &s->d_work_cap, work_bytes)) != TBG_OK) return rc;
  // Reserve the slot (busy, its old tickets expired) and pack WITHOUT the
  // context lock: a 16-batch group is ~70 MB of host copies, during which
  // other threads' tbg_poll / tbg_collect / tbg_submit must not wait.
  s->parts.clear();
  s->busy = true;
  lk.unlock();
  const auto t_pack = std::chrono::steady_clock::now();

  // ---- pack: batch k's duties / partials / messages follow batch k-1's,
  // every index rebased by the running offsets ----
  uint8_t* h = s->h_in;
  uint32_t* msg_off = (uint32_t*)(h + o_msg_off);
  uint32_t* duty_msg = (uint32_t*)(h + o_duty_msg);
  uint32_t* duty_first = (uint32_t*)(h + o_duty_first);
  uint32_t* thr = (uint32_t*)(h + o_thr);
  uint32_t* pd = (uint32_t*)(h + o_pduty);
  // offsets first, then every caller batch packed by its own worker (the
  // sections are disjoint): a 16-batch group is ~70 MB of host copies, which
  // one thread would take longer to pack than the GPU takes to run it
  std::vector<Part> parts(n_batches);
  std::vector<uint32_t> mb0(n_batches);
  uint32_t D = 0, P = 0, M = 0, MB = 0;
  for (uint32_t k = 0; k < n_batches; ++k) {
    const tbg_batch* b = bs[k];
    parts[k].d0 = D;
    parts[k].nd = b->n_duties;
    parts[k].p0 = P;
    parts[k].np = b->n_partials;
    parts[k].m0 = M;
    parts[k].nm = verify ? b->n_msgs : 0;
    mb0[k] = MB;
    D += parts[k].nd;
    P += parts[k].np;
    M += parts[k].nm;
    if (verify) MB += b->msg_off[b->n_msgs];
  }
  auto pack = [&](uint32_t k) {
    const tbg_batch* b = bs[k];
    const uint32_t D = parts[k].d0, P = parts[k].p0, M = parts[k].m0, MB = mb0[k];
    const uint32_t bnd = b->n_duties, bnp = b->n_partials, bnm = parts[k].nm;
    if (verify) {
      const uint32_t bmb = b->msg_off[bnm];
      if (bmb) memcpy(h + o_msgs + MB, b->msgs, bmb);
      for (uint32_t m = 0; m < bnm; ++m) msg_off[M + m] = MB + b->msg_off[m];
      for (uint32_t d = 0; d < bnd; ++d) duty_msg[D + d] = M + b->duty_msg[d];
      if (aggver) memcpy(h + o_pk + 4ull * D, b->pubkey_ids, 4ull * bnd);  // (one group key per duty)
      else memcpy(h + o_pk + 4ull * P, b->pubkey_ids, 4ull * bnp);
      if (l0m) {  // this batch's duties by message (sections disjoint from the other batches')
        std::vector<uint32_t> cursor(bnm);
        l0m_sort_batch(duty_msg, D, bnd, M, bnm, (uint32_t*)(h + o_mfirst), (uint32_t*)(h + o_mduty), cursor.data());
      }
    }
    for (uint32_t d = 0; d < bnd; ++d) {
      duty_first[D + d] = P + b->duty_first[d];
      for (uint32_t j = b->duty_first[d]; j < b->duty_first[d + 1]; ++j) pd[P + j] = D + d;
    }
    if (op == TBG_OP_VERIFY_AGGREGATE) memcpy(thr + D, b->duty_threshold, 4ull * bnd);
    else memset(thr + D, 0, 4ull * bnd);
    if (bnp) {
      memcpy(h + o_sigs + 96ull * P, b->sigs, 96ull * bnp);
      memcpy(h + o_ids + P, b->identifiers, bnp);
    }
  };
  // A set launch (one caller batch): the duties move to their padded places,
  // set k's first on a multiple of Gp; a padding duty is empty (no partials,
  // message 0), which k_rlc_duty_sum leaves RLC_NONE.  Partials and messages
  // keep their indices.
  auto pack_sets = [&]() {
    const tbg_batch* b = bs[0];
    const uint32_t Gp = G ? G : 1;
    uint32_t* dset = (uint32_t*)(h + o_dset);
    if (msg_bytes) memcpy(h + o_msgs, b->msgs, msg_bytes);
    memcpy(msg_off, b->msg_off, 4ull * nm);
    if (np) {
      memcpy(h + o_pk, b->pubkey_ids, 4ull * np);
      memcpy(h + o_sigs, b->sigs, 96ull * np);
      memcpy(h + o_ids, b->identifiers, np);
    }
    uint32_t e = 0;
    for (uint32_t k = 0; k < n_sets; ++k) {
      const uint32_t a = set_first[k], z = set_first[k + 1];
      if (a == z) continue;
      for (; e % Gp; ++e) {
        duty_first[e] = b->duty_first[a];
        duty_msg[e] = 0;
        dset[e] = k;
      }
      for (uint32_t d = a; d < z; ++d, ++e) {
        duty_first[e] = b->duty_first[d];
        duty_msg[e] = b->duty_msg[d];
        dset[e] = k;
        for (uint32_t j = b->duty_first[d]; j < b->duty_first[d + 1]; ++j) pd[j] = e;
      }
    }
    memset(thr, 0, 4ull * nd);
    parts[0].nd = nd;
    if (l0m) {  // (the padded duties: a padding duty names message 0 and is never combined)
      std::vector<uint32_t> cursor(nm);
      l0m_sort_batch(duty_msg, 0, nd, 0, nm, (uint32_t*)(h + o_mfirst), (uint32_t*)(h + o_mduty), cursor.data());
    }
  };
  if (l0m) ((uint32_t*)(h + o_mfirst))[0] = 0;
  const uint32_t workers = (np >= (1u << 16) && n_batches > 1) ? std::min<uint32_t>(n_batches, 8) : 1;
  if (set_first) {
    pack_sets();
  } else if (workers == 1) {
    for (uint32_t k = 0; k < n_batches; ++k) pack(k);
  } else {
    std::vector<std::thread> th;
    for (uint32_t w = 0; w < workers; ++w)
      th.emplace_back([&, w] {
        for (uint32_t k = w; k < n_batches; k += workers) pack(k);
      });
    for (auto& t : th) t.join();
  }
  duty_first[nd] = np;
  if (verify) msg_off[nm] = MB;
  if (aggver)
    for (uint32_t d = 0; d <= nd; ++d) ((uint32_t*)(h + o_iota))[d] = d;
  // Level 0 by message, the chunk plan (chunk -> message, message -> first
  // chunk; the shape of SumPlan, k_sum.hip).  Invariant: the messages of
  // caller batch j follow those of batch j - 1 and a message never spans
  // caller batches (every batch brings its own), so batch j's duties, CSR
  // rows and chunks all follow batch j - 1's -- the first n_msgs entries of
  // msg_first / chunk_first, with the duties and chunks they cover, are a
  // prefix's own plan (tbg_replay_plan n_parts; Part::ch1, ::maxch).
  if (l0m) {
    uint32_t nc = 0, largest = 0;
    for (uint32_t k = 0; k < n_batches; ++k) {
      const uint32_t big = l0m_chunk_plan((const uint32_t*)(h + o_mfirst), parts[k].m0, parts[k].nm,
                                          (uint32_t*)(h + o_cfirst), (uint32_t*)(h + o_cmsg), &nc);
      largest = std::max(largest, big);
      parts[k].ch1 = nc;
      parts[k].maxch = largest;
    }
  }
  const auto t_packed = std::chrono::steady_clock::now();

  lk.lock();
  // from here on a failure releases the reserved slot
  auto release = [&](int code) {
    s->busy = false;
    return code;
  };
  if (hipSetDevice(c->device) != hipSuccess) return release(TBG_E_DEVICE);
  DevBatch B{};
  memset(&B, 0, sizeof(B));
  B.op = op;
  B.n_duties = nd;
  B.n_partials = np;
  B.n_msgs = nm;
  uint8_t* di = s->d_in;
  uint8_t* dw = s->d_work;
  B.msgs = di + o_msgs;
  B.msg_off = (const uint32_t*)(di + o_msg_off);
  B.duty_msg = (const uint32_t*)(di + o_duty_msg);
  B.duty_first = (const uint32_t*)(di + o_duty_first);
  B.duty_threshold = (const uint32_t*)(di + o_thr);
  B.partial_duty = (const uint32_t*)(di + o_pduty);
  B.sigs = di + o_sigs;
  B.identifiers = di + o_ids;
  B.pubkey_ids = (const uint32_t*)(di + o_pk);
  B.sig_aff = (G2A*)(dw + w_sig_aff);
  B.h_aff = (G2A*)(dw + w_h_aff);
  B.h_status = (int32_t*)(dw + w_h_st);
  B.h_jac = (G2J*)(dw + w_h_jac);
  B.lam = (uint32_t*)(dw + w_lam);
  B.sig_lines = (uint32_t*)(dw + w_sl);
  B.h_lines = (uint32_t*)(dw + w_hl);
  B.rlc_group = aggver ? 0u : G;  // (the batch itself runs no check: its view does, av_group)
  {
    uint64_t k[4];
    if (c->rlc_seed) {
      uint64_t z = c->rlc_seed;  // splitmix64: fixed, reproducible scalars (tests only)
      for (auto& w : k) {
        z += 0x9E3779B97F4A7C15ull;
        uint64_t x = z;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        w = x ^ (x >> 31);
      }
    } else {
      std::random_device rd;  // the OS entropy source (getrandom / /dev/urandom)
      for (auto& w : k) w = ((uint64_t)rd() << 32) ^ rd() ^ (++c->seed_ctr * 0x9E3779B97F4A7C15ull);
    }
    for (int j = 0; j < 4; ++j) {
      B.rlc_seed[2 * j] = (uint32_t)(k[j] >> 32);
      B.rlc_seed[2 * j + 1] = (uint32_t)k[j];
    }
    // The batched subgroup test's key never follows rlc_seed:
    // its soundness needs coefficients a submitter cannot predict.
    std::random_device rd;
    for (auto& w : B.sgb_seed) w = rd() ^ (uint32_t)(++c->seed_ctr * 0x9E3779B9u);
  }
  B.rlc_chunk = C;
  B.part_p = (G1J*)(dw + w_pp);
  B.part_s = (G2J*)(dw + w_ps);
  B.chunk_f = (uint32_t*)(dw + w_cf);
  B.chunk_list = (uint32_t*)(dw + w_cl);
  B.chunk_lines = B.sig_lines;  // (one fallback line buffer, see w_sl)
  B.dv_p = (G1A*)(dw + w_dvp);
  B.dv_s = (G2J*)(dw + w_dvs);
  B.dv_state = (int32_t*)(dw + w_dvst);
  B.grp_state = (int32_t*)(dw + w_gst);
  B.grp_lines = (uint32_t*)(dw + w_gl);
  B.counters = (uint32_t*)(dw + w_cnt);
  B.part_list = (uint32_t*)(dw + w_pl);
  B.id_fe = (uint32_t*)(dw + w_dvfe);
  B.pend_pts = (G2A*)(dw + w_pend);
  B.chunk_fe = (uint32_t*)(dw + w_cfe);
  B.cid_list = (uint32_t*)(dw + w_cidl);
  B.cid_p = (G1A*)(dw + w_cidp);
  B.cid_lines = B.sig_lines;
  // Level 1g is opt-in (tbg_config.gident).  Measured
  // (profiles/r03/gident/): +7 % at 1 % invalid in 20-step runs, whose three
  // launches reach their latency-bound fallback levels together, but -3 % at
  // 48 steps and -11 % on config 5, where launches overlap and the
  // narrowing's shorter lists matter more than its extra levels.
  B.gident = G > 1 && G <= 64 ? c->gident : 0u;  // (level 1g's lines kernel runs a lane per duty of a group)
  B.grp_fe = (uint32_t*)(dw + w_gfe);
  B.gid_list = (uint32_t*)(dw + w_gidl);
  B.gid_p = (G1A*)(dw + w_gidp);
  B.gid_lines = B.sig_lines;
  B.gid_f = (uint32_t*)(dw + w_gidf);
  B.id_list = (uint32_t*)(dw + w_idl);
  B.id_p = (G1A*)(dw + w_idp);
  B.id_lines = B.sig_lines;
  B.fb_window = fb_w;
  {
    // full-grid passes of the duty / partial lists: those the collected
    // batches' invalid share makes likely (10x margin), every pass for the
    // per-partial schedule
    const double share = std::min(1.0, 10.0 * c->invalid_ema);
    const uint64_t expect = (uint64_t)((double)vp * share);
    B.fb_full = (G == 0 || fb_w == 0) ? 0xFFFFFFFFu
                                      : (uint32_t)std::min<uint64_t>(0xFFFFFFFFull, (expect / fb_w + 1) * (uint64_t)fb_w);
  }
  B.fb_base = 0;
  B.partial_status = (int32_t*)(dw + w_pst);
  B.duty_status = (int32_t*)(dw + w_dst);
  B.agg = dw + w_agg;
  if (set_first) {
    B.sets = 1;
    B.n_sets = n_sets;
    B.duty_set = (const uint32_t*)(di + o_dset);
    B.set_status = (int32_t*)(dw + w_sst);
    B.gident = 0;  // (no level 1g: a failed group is not narrowed)
  }
  B.rlc_batch = l0 && !aggver ? 1u : 0u;
  if (aggver) {
    B.agg_aff = (G2A*)(dw + w_aaff);
    B.av_status = (int32_t*)(dw + w_avst);
    B.av_counters = (uint32_t*)(dw + w_avcnt);
    B.av_iota = (const uint32_t*)(di + o_iota);
    B.av_group = G;
    B.av_chunk = C;
    B.av_batch = l0 ? 1u : 0u;
  }
  B.msm_r = (uint64_t*)(dw + w_mr);
  B.msm_off = (uint32_t*)(dw + w_moff);
  B.msm_cur = (uint32_t*)(dw + w_mcur);
  B.msm_ent = (uint32_t*)(dw + w_ment);
  B.msm_bkt = (G2J*)(dw + w_mbkt);
  B.msm_part = (G2J*)(dw + w_mpart);
  B.msm_sum = (G2J*)(dw + w_msum);
  B.batch_pt = (G2A*)(dw + w_bpt);
  B.batch_lines = (uint32_t*)(dw + w_blines);
  B.batch_f = (uint32_t*)(dw + w_bf);
  B.grp_f = (uint32_t*)(dw + w_gf);
  B.gm_off = (uint32_t*)(dw + w_gmoff);
  B.gm_ent = (uint32_t*)(dw + w_gment);
  B.gm_part = (G2J*)(dw + w_gmpart);
  B.gm_lead = (uint32_t*)(dw + w_gmlead);
  B.gm_list = (uint32_t*)(dw + w_gmlist);
  B.gm_hist = (uint32_t*)(dw + w_gmhist);
  B.gm_order = (uint32_t*)(dw + w_gmorder);
  B.sgb = sgb ? 1u : 0u;
  B.sgb_m = sgb_m;
  B.sgb_split = sgb_split;
  B.sgb_off = (uint32_t*)(dw + w_sgoff);
  B.sgb_ent = (uint32_t*)(dw + w_sgent);
  B.sgb_part = (G2J*)(dw + w_sgpart);
  B.sgb_rank = (uint32_t*)(dw + w_sgrank);
  B.sgb_code = (uint32_t*)(dw + w_sgcode);
  B.sgb_bad = (uint32_t*)(dw + w_sgbad);
  B.sgb_t = (G2J*)(dw + w_sgt);
  B.l0f_sum = (G2J*)(dw + w_l0fsum);
  B.l0f_u = (uint32_t*)(dw + w_l0fu);
  B.l0_duty_partials = c->l0_duty_partials;
  B.l0_tail_partials = c->l0_tail_partials;
  B.l0_msg_share = l0m ? c->l0_msg_share : TBG_L0_MSG_NEVER;  // (no plan: never by message)
  B.l0m_n_chunks = l0m ? parts[n_batches - 1].ch1 : 0;
  B.l0m_max_chunks = l0m ? parts[n_batches - 1].maxch : 0;
  B.msg_first = (const uint32_t*)(di + o_mfirst);
  B.msg_duty = (const uint32_t*)(di + o_mduty);
  B.l0m_chunk_first = (const uint32_t*)(di + o_cfirst);
  B.l0m_chunk_msg = (const uint32_t*)(di + o_cmsg);
  B.l0m_part = (G1J*)(dw + w_l0mpart);
  B.l0m_cnt = (uint32_t*)(dw + w_l0mcnt);
  B.l0m_q = (G1A*)(dw + w_l0mq);
  B.l0m_state = (int32_t*)(dw + w_l0mst);
  B.agg_acc = (G2J*)(dw + w_aacc);
  B.agg_list = (uint32_t*)(dw + w_alist);

  hipStream_t st = s->st;
  // The resident pubkey table may have been (re)loaded on the utility stream
  // (already complete: tbg_load_pubkeys waits for it; ordered anyway).
  if (hipStreamWaitEvent(st, c->keys_ready, 0) != hipSuccess ||
      hipMemcpyAsync(s->d_in, s->h_in, in_bytes, hipMemcpyHostToDevice, st) != hipSuccess)
    return release(TBG_E_DEVICE);
  rc = launch_chain(c, *s, B, s->ev);
  if (rc != TBG_OK) return release(rc);
  if (hipMemcpyAsync(s->h_out, dw + w_out, out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipEventRecord(s->done, st) != hipSuccess)
    return release(TBG_E_DEVICE);
  {
    const auto t_end = std::chrono::steady_clock::now();
    using ns = std::chrono::nanoseconds;
    c->host[0] += 1;
    c->host[1] += np;
    c->host[2] += (uint64_t)std::chrono::duration_cast<ns>(t_packed - t_pack).count();
    c->host[3] += (uint64_t)std::chrono::duration_cast<ns>(t_end - t_packed).count();
  }

  for (uint32_t k = 0; k < n_batches; ++k) {
    parts[k].ticket = c->next_ticket++;
    parts[k].pending = true;
    tickets[k] = parts[k].ticket;
  }
  s->parts = std::move(parts);
  s->seen_bad = s->seen_total = 0;
  s->seen_nsub = s->seen_dec = 0;
  s->busy = true;
  s->ticket = s->parts[0].ticket;
  s->op = op;
  s->n_duties = nd;
  s->n_partials = np;
  s->n_msgs = nm;
  s->out_bytes = out_bytes;
  s->B = B;
  s->last = B;
  s->sgb_m_small = sgb_m_small;
  s->w_out = w_out;
  s->sets = set_first != nullptr;
  s->n_sets = set_first ? n_sets : 0;
  s->o_sets = w_sst - w_out;
  return TBG_OK;
}

int tbg_poll(tbg_ctx* c, tbg_ticket t) {
  if (!c) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  Slot* s = find_ticket(c, t, true, nullptr);
  if (!s) return TBG_E_TICKET;
  HIP_TRY(hipSetDevice(c->device));
  hipError_t q = hipEventQuery(s->done);
  if (q == hipErrorNotReady) return TBG_E_PENDING;
  return q == hipSuccess ? TBG_OK : TBG_E_DEVICE;
}

// A part's slice of the slot's (pinned) output image.
static void copy_part(const Slot* s, const Part& q, int32_t* pst, int32_t* dst, uint8_t* agg) {
  const uint32_t np = s->n_partials, nd = s->n_duties;
  size_t o = 0;
  auto sec = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 16); return at; };
  size_t o_pst = sec(4ull * np), o_dst = sec(4ull * nd), o_agg = sec(96ull * nd);
  if (pst) memcpy(pst, s->h_out + o_pst + 4ull * q.p0, 4ull * q.np);
  if (dst) memcpy(dst, s->h_out + o_dst + 4ull * q.d0, 4ull * q.nd);
  if (agg) memcpy(agg, s->h_out + o_agg + 96ull * q.d0, 96ull * q.nd);
}

static void part_done(Slot* s, Part* q) {
  q->pending = false;
  bool any = false;
  for (const auto& x : s->parts) any |= x.pending;
  s->busy = any;
}

// A set launch's slice of the output image: the sets' statuses, and the
// partial statuses (partials keep their caller indices in the padded batch).
static void copy_sets(const Slot* s, int32_t* sst, int32_t* pst) {
  if (sst) memcpy(sst, s->h_out + s->o_sets, 4ull * s->n_sets);
  if (pst) memcpy(pst, s->h_out, 4ull * s->n_partials);  // (partial statuses lead the output image)
}

// tbg_collect (sets = false) and tbg_collect_sets (sets = true: sst / pst).
static int collect_impl(tbg_ctx* c, tbg_ticket t, int32_t* pst, int32_t* dst, uint8_t* agg, int32_t* sst, bool sets,
                        int block) {
  if (!c) return TBG_E_INVALID_ARG;
  std::unique_lock<std::mutex> lk(c->mu);
  Part* q = nullptr;
  Slot* s = find_ticket(c, t, true, &q);
  if (!s || q->collecting || s->sets != sets) return TBG_E_TICKET;
  HIP_TRY(hipSetDevice(c->device));
  hipError_t e = hipEventQuery(s->done);
  if (e == hipErrorNotReady) {
    if (!block) return TBG_E_PENDING;
    // Wait without the context mutex: other threads keep submitting and
    // polling meanwhile.  The slot stays busy (this part is pending) and
    // `collecting` keeps a second collect of the same ticket out.
    q->collecting = true;
    hipEvent_t done = s->done;
    int dev = c->device;
    lk.unlock();
    const auto t_wait = std::chrono::steady_clock::now();
    (void)hipSetDevice(dev);  // the HIP current device is per thread
    e = hipEventSynchronize(done);
    c->host[7] += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() -
                                                                                 t_wait).count();
    lk.lock();
    q->collecting = false;
  }
  if (e != hipSuccess) {
    part_done(s, q);
    return TBG_E_DEVICE;
  }
  const auto t_gather = std::chrono::steady_clock::now();
  if (sets) copy_sets(s, sst, pst);
  else copy_part(s, *q, pst, dst, agg);
  if (sets) {
    // every candidate of a failed group counts as invalid: an upper bound of
    // the invalid share, so level 0 switches off under bad sets as it does
    // under bad partials
    s->seen_bad += (uint32_t)((const int32_t*)(s->h_out + s->o_sets))[s->n_sets + SET_BAD];
    s->seen_total += q->np;
  } else if (s->op == TBG_OP_AGGREGATE_VERIFY) {  // the duties whose aggregate failed, over the duties checked
    const int32_t* ds = (const int32_t*)(s->h_out + align_up(4ull * s->n_partials, 16));  // (copy_part's layout)
    uint32_t bad = 0, checked = 0;
    for (uint32_t d = 0; d < q->nd; ++d) {
      const int32_t v = ds[q->d0 + d];
      bad += v == TBG_DS_AGG_INVALID ? 1u : 0u;
      checked += v == TBG_DS_AGG_INVALID || v == TBG_DS_OK ? 1u : 0u;
    }
    s->seen_bad += bad;
    s->seen_total += checked;
  } else if (s->op != TBG_OP_AGGREGATE && q->np) {  // the adaptive group size's and level 0's input
    const int32_t* st = (const int32_t*)s->h_out;  // partial statuses lead the output region
    uint32_t bad = 0;
    for (uint32_t i = 0; i < q->np; ++i) bad += st[q->p0 + i] == TBG_PS_INVALID ? 1u : 0u;
    s->seen_bad += bad;
    s->seen_total += q->np;
  }
  if (q->np) {  // the batched subgroup test's input: non-subgroup share of all partials
    const int32_t* st = (const int32_t*)s->h_out;
    uint32_t ns = 0;
    for (uint32_t i = 0; i < q->np; ++i) ns += st[q->p0 + i] == TBG_PS_ERR_SUBGROUP ? 1u : 0u;
    s->seen_nsub += ns;
    s->seen_dec += q->np;
  }
  c->host[4] += 1;
  c->host[5] += q->np;
  c->host[6] += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() -
                                                                               t_gather).count();
  chain_times(s->ev, s->ms, s->op);
  memcpy(c->last_ms, s->ms, sizeof(c->last_ms));
  part_done(s, q);
  // One update per DEVICE batch, over all of its parts (whatever order they
  // are collected in), once its last part is collected.
  if (!s->busy && s->seen_total) {
    c->invalid_ema = 0.5 * c->invalid_ema + 0.5 * (double)s->seen_bad / (double)s->seen_total;
    s->seen_bad = s->seen_total = 0;
  }
  if (!s->busy && s->seen_dec) {
    c->nonsub_ema = 0.5 * c->nonsub_ema + 0.5 * (double)s->seen_nsub / (double)s->seen_dec;
    s->seen_nsub = s->seen_dec = 0;
  }
  return TBG_OK;
}

int tbg_collect(tbg_ctx* c, tbg_ticket t, int32_t* pst, int32_t* dst, uint8_t* agg, int block) {
  return collect_impl(c, t, pst, dst, agg, nullptr, false, block);
}

int tbg_collect_sets(tbg_ctx* c, tbg_ticket t, int32_t* set_status, int32_t* partial_status, int block) {
  return collect_impl(c, t, partial_status, nullptr, nullptr, set_status, true, block);
}

int tbg_run(tbg_ctx* c, const tbg_batch* b, int32_t* pst, int32_t* dst, uint8_t* agg) {
  tbg_ticket t;
  int rc = tbg_submit(c, b, &t);
  if (rc != TBG_OK) return rc;
  return tbg_collect(c, t, pst, dst, agg, 1);
}

int tbg_replay_plan(tbg_ctx* c, const tbg_ticket* tickets, const uint32_t* n_parts, uint32_t n_launches, float* ms8) {
  if (!c || !tickets || n_launches == 0) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  std::vector<Slot*> sl(n_launches, nullptr);
  std::vector<DevBatch> bs(n_launches);
  for (uint32_t k = 0; k < n_launches; ++k) {
    sl[k] = find_ticket(c, tickets[k], false, nullptr);
    if (!sl[k]) return TBG_E_TICKET;
    // A prefix of the packed device batch is itself a batch: batch j's
    // duties, partials and messages all follow batch j-1's.
    DevBatch B = sl[k]->B;
    const uint32_t np = n_parts ? n_parts[k] : 0;
    if (np > sl[k]->parts.size()) return TBG_E_INVALID_ARG;
    if (np && np < sl[k]->parts.size()) {
      const Part& last = sl[k]->parts[np - 1];
      B.n_duties = last.d0 + last.nd;
      B.n_partials = last.p0 + last.np;
      B.n_msgs = last.m0 + last.nm;
      B.l0m_n_chunks = last.ch1;  // (the prefix's own plan, see submit_impl)
      B.l0m_max_chunks = last.maxch;
      // the subgroup test's schedule follows the prefix's own partials
      if (B.sgb && sgb_triple(B.sgb_m)) {
        B.sgb_m = sgb_group_size(c, B.n_partials, sl[k]->sgb_m_small, true);
        B.sgb_split = sgb_triple(B.sgb_m) ? 1u : sgb_split_for(B.sgb_m);
      }
    }
    bs[k] = B;
  }
  HIP_TRY(hipSetDevice(c->device));
  std::vector<hipEvent_t> ev((size_t)kChainEvents * n_launches);
  for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
  int rc = TBG_OK;
  // Launch k on the streams of its slot: launches of different slots are in
  // flight together, launches of one slot run in order.  Runs of launches on
  // distinct slots are enqueued stage by stage (launch_chain), so their
  // first kernels start together (each launch waiting for the previous one's
  // hash or H(m) lines was measured 11-12 % slower at 20 steps, round 5:
  // profiles/r05/stagger/).
  for (uint32_t k0 = 0; k0 < n_launches && rc == TBG_OK;) {
    uint32_t k1 = k0 + 1;
    while (k1 < n_launches && std::find(sl.begin() + k0, sl.begin() + k1, sl[k1]) == sl.begin() + k1) ++k1;
    // The level-0 launches run together share the SIMDs: their shape follows
    // their duties together (l0_shape), where each launch's arena fits it.
    if (c->chunk_auto && c->rlc_auto) {
      uint64_t nd = 0;
      bool all_l0 = true;
      for (uint32_t k = k0; k < k1; ++k) {
        nd += bs[k].n_duties;
        all_l0 = all_l0 && bs[k].rlc_batch && bs[k].rlc_group >= 8 && !bs[k].sets;  // (sets are padded to their G)
      }
      // the cheapest shape every launch of the run can hold (round 6: the
      // candidates that one of them cannot are skipped, not the reshape)
      uint32_t G = 16, C = 4;
      auto fits_all = [&](uint32_t g, uint32_t ch) {
        for (uint32_t k = k0; k < k1; ++k)
          if (!l0_shape_fits(sl[k]->n_duties, sl[k]->B.rlc_group, sl[k]->B.rlc_chunk, bs[k].n_duties, g, ch))
            return false;
        return true;
      };
      if (all_l0) l0_shape(nd, c->n_simd, true, G, C, fits_all);
      for (uint32_t k = k0; k < k1 && all_l0; ++k)
        if (l0_shape_fits(sl[k]->n_duties, sl[k]->B.rlc_group, sl[k]->B.rlc_chunk, bs[k].n_duties, G, C)) {
          bs[k].rlc_group = G;
          bs[k].rlc_chunk = C;
        }
    }
    for (int stage = 0; stage < 3 && rc == TBG_OK; ++stage)
      for (uint32_t k = k0; k < k1 && rc == TBG_OK; ++k)
        rc = launch_chain(c, *sl[k], bs[k], ev.data() + (size_t)kChainEvents * k, stage);
    for (uint32_t k = k0; k < k1; ++k) sl[k]->last = bs[k];
    k0 = k1;
  }
  for (uint32_t k = 0; k < n_launches; ++k) {
    if (hipStreamSynchronize(sl[k]->st) != hipSuccess) rc = TBG_E_DEVICE;
    if (hipStreamSynchronize(sl[k]->st2) != hipSuccess) rc = TBG_E_DEVICE;
  }
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (rc == TBG_OK) {
    for (uint32_t k = 0; k < n_launches; ++k) {
      float m[8];
      chain_times(ev.data() + (size_t)kChainEvents * k, m, bs[k].op);
      for (int j = 0; j < 7; ++j) acc[j] += m[j];
    }
    // wall time: first launch's start to the latest chain end
    for (uint32_t k = 0; k < n_launches; ++k) {
      float w = 0;
      hipEventElapsedTime(&w, ev[0], ev[(size_t)kChainEvents * k + chain_end(bs[k].op)]);
      if (w > acc[7]) acc[7] = w;
    }
    if (ms8) memcpy(ms8, acc, sizeof(acc));
    memcpy(c->last_ms, acc, sizeof(acc));
  }
  for (auto& e : ev) hipEventDestroy(e);
  return rc;
}

int tbg_replay_profile(tbg_ctx* c, tbg_ticket t, tbg_kernel_time* out, uint32_t max_entries, uint32_t* n_entries) {
  if (!c || !n_entries || (max_entries && !out)) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  Slot* s = find_ticket(c, t, false, nullptr);
  if (!s) return TBG_E_TICKET;
  HIP_TRY(hipSetDevice(c->device));
  // nothing else of this context in flight: every kernel runs alone
  for (auto& x : c->slots) {
    HIP_TRY(hipStreamSynchronize(x.st));
    HIP_TRY(hipStreamSynchronize(x.st2));
  }
  std::vector<KProfRec> rec;
  hipEvent_t ev[kChainEvents];
  for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
  g_kprof = &rec;
  int rc = launch_chain(c, *s, s->B, ev);
  s->last = s->B;
  g_kprof = nullptr;
  if (hipStreamSynchronize(s->st) != hipSuccess || hipStreamSynchronize(s->st2) != hipSuccess) rc = TBG_E_DEVICE;
  uint32_t n = 0;
  for (auto& r : rec) {
    if (rc == TBG_OK && n < max_entries) {
      float ms = 0;
      if (!r.a || !r.b || hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) rc = TBG_E_DEVICE;
      snprintf(out[n].name, sizeof(out[n].name), "%s", r.name);
      out[n].ms = ms;
      ++n;
    }
    if (r.a) hipEventDestroy(r.a);
    if (r.b) hipEventDestroy(r.b);
  }
  for (auto& e : ev) hipEventDestroy(e);
  *n_entries = n;
  return rc;
}

int tbg_replay_multi(tbg_ctx* c, const tbg_ticket* tickets, uint32_t n_tickets, uint32_t iters, float* ms8) {
  if (!c || !tickets || n_tickets == 0 || iters == 0) return TBG_E_INVALID_ARG;
  std::vector<tbg_ticket> plan(iters);
  for (uint32_t k = 0; k < iters; ++k) plan[k] = tickets[k % n_tickets];  // round-robin over the resident batches
  return tbg_replay_plan(c, plan.data(), nullptr, iters, ms8);
}

int tbg_replay(tbg_ctx* c, tbg_ticket t, uint32_t iters, float* ms8) { return tbg_replay_multi(c, &t, 1, iters, ms8); }

static int fetch_impl(tbg_ctx* c, tbg_ticket t, int32_t* pst, int32_t* dst, uint8_t* agg, int32_t* sst, bool sets) {
  if (!c) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  Part* q = nullptr;
  Slot* s = find_ticket(c, t, false, &q);
  if (!s || s->sets != sets) return TBG_E_TICKET;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(s->h_out, s->d_work + s->w_out, s->out_bytes, hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  if (sets) copy_sets(s, sst, pst);
  else copy_part(s, *q, pst, dst, agg);
  return TBG_OK;
}

int tbg_fetch(tbg_ctx* c, tbg_ticket t, int32_t* pst, int32_t* dst, uint8_t* agg) {
  return fetch_impl(c, t, pst, dst, agg, nullptr, false);
}

int tbg_fetch_sets(tbg_ctx* c, tbg_ticket t, int32_t* set_status, int32_t* partial_status) {
  return fetch_impl(c, t, partial_status, nullptr, nullptr, set_status, true);
}

int tbg_fetch_stats(tbg_ctx* c, tbg_ticket t, uint32_t* out4) {
  if (!c || !out4) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  Slot* s = find_ticket(c, t, false, nullptr);
  if (!s) return TBG_E_TICKET;
  HIP_TRY(hipSetDevice(c->device));
  uint32_t cnt[CNT_WORDS] = {};
  const DevBatch L = checked_batch(s->last);  // (TBG_OP_AGGREGATE_VERIFY: the aggregates' checks)
  if (s->op != TBG_OP_AGGREGATE) {
    HIP_TRY(hipMemcpyAsync(cnt, L.counters, sizeof(cnt), hipMemcpyDeviceToHost, s->st));
    HIP_TRY(hipStreamSynchronize(s->st));
  }
  uint32_t ng = L.rlc_group ? (L.n_duties + L.rlc_group - 1) / L.rlc_group : 0;
  out4[0] = ng;
  out4[1] = cnt[CNT_DUTIES];
  out4[2] = cnt[CNT_PARTIALS];
  out4[3] = L.rlc_group;
  return TBG_OK;
}

int tbg_fetch_fallback(tbg_ctx* c, tbg_ticket t, uint32_t* out8) {
  if (!c || !out8) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  Slot* s = find_ticket(c, t, false, nullptr);
  if (!s) return TBG_E_TICKET;
  HIP_TRY(hipSetDevice(c->device));
  uint32_t cnt[CNT_WORDS] = {};
  const DevBatch L = checked_batch(s->last);  // (TBG_OP_AGGREGATE_VERIFY: the aggregates' checks)
  if (s->op != TBG_OP_AGGREGATE) {
    HIP_TRY(hipMemcpyAsync(cnt, L.counters, sizeof(cnt), hipMemcpyDeviceToHost, s->st));
    HIP_TRY(hipStreamSynchronize(s->st));
  }
  out8[0] = L.rlc_group ? (L.n_duties + L.rlc_group - 1) / L.rlc_group : 0;
  out8[1] = cnt[CNT_GID];
  out8[2] = cnt[CNT_CHUNKS];
  out8[3] = cnt[CNT_CID];
  out8[4] = cnt[CNT_DUTIES];
  out8[5] = cnt[CNT_PARTIALS];
  out8[6] = L.rlc_group;
  out8[7] = s->op == TBG_OP_AGGREGATE || !L.rlc_batch ? (uint32_t)TBG_L0_NOT_RUN
            : cnt[CNT_L0_OK]                              ? (uint32_t)TBG_L0_PASSED
                                                          : (uint32_t)TBG_L0_FAILED;
  return TBG_OK;
}

int tbg_fetch_shape(tbg_ctx* c, tbg_ticket t, uint32_t* out4) {
  if (!c || !out4) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  Slot* s = find_ticket(c, t, false, nullptr);
  if (!s) return TBG_E_TICKET;
  const DevBatch L = checked_batch(s->last);  // (TBG_OP_AGGREGATE_VERIFY: the aggregates' checks)
  const uint32_t G = L.rlc_group, C = L.rlc_chunk;
  out4[0] = G;
  out4[1] = G ? C : 0;
  out4[2] = L.rlc_batch ? 1u : 0u;
  out4[3] = G ? ((s->last.n_duties + G - 1) / G) * ((G + C - 1) / C) : 0;
  return TBG_OK;
}

int tbg_fetch_subgroup(tbg_ctx* c, tbg_ticket t, uint32_t* out3) {
  if (!c || !out3) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  Slot* s = find_ticket(c, t, false, nullptr);
  if (!s) return TBG_E_TICKET;
  HIP_TRY(hipSetDevice(c->device));
  out3[0] = out3[1] = out3[2] = 0;
  if (!s->last.sgb) return TBG_OK;
  out3[2] = s->last.sgb_m;
  const uint32_t n_sg = sgb_groups(s->last.n_partials, s->last.sgb_m);
  std::vector<uint32_t> bad(n_sg);
  HIP_TRY(hipMemcpyAsync(bad.data(), s->last.sgb_bad, 4ull * n_sg, hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  out3[0] = n_sg;
  for (uint32_t g = 0; g < n_sg; ++g) out3[1] += bad[g] ? 1u : 0u;
  return TBG_OK;
}

int tbg_fetch_subgroup_schedule(tbg_ctx* c, tbg_ticket t, uint32_t* out1) {
  if (!c || !out1) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  Slot* s = find_ticket(c, t, false, nullptr);
  if (!s) return TBG_E_TICKET;
  // (the launch's own fields: the kernels took their schedule from the same ones)
  *out1 = !s->last.sgb                 ? (uint32_t)TBG_SGB_SCHED_NONE
          : sgb_triple(s->last.sgb_m) ? (uint32_t)TBG_SGB_SCHED_TRIPLE
          : sgb_paired(s->last.sgb_m) ? (uint32_t)TBG_SGB_SCHED_PAIRED
                                      : (uint32_t)TBG_SGB_SCHED_CLASSIC;
  return TBG_OK;
}

int tbg_host_stats(tbg_ctx* c, uint64_t* out8, int reset) {
  if (!c || !out8) return TBG_E_INVALID_ARG;
  for (int k = 0; k < 8; ++k) out8[k] = reset ? c->host[k].exchange(0) : c->host[k].load();
  return TBG_OK;
}

int tbg_slot_bytes(tbg_ctx* c, tbg_ticket t, uint64_t* device_bytes, uint64_t* pinned_bytes) {
  if (!c || !device_bytes || !pinned_bytes) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  Slot* s = find_ticket(c, t, false, nullptr);
  if (!s) return TBG_E_TICKET;
  *device_bytes = (uint64_t)s->d_in_cap + (uint64_t)s->d_work_cap;
  *pinned_bytes = (uint64_t)s->h_in_cap + (uint64_t)s->h_out_cap;
  return TBG_OK;
}

int tbg_fetch_level0_msgs(tbg_ctx* c, tbg_ticket t, uint32_t* out2) {
  if (!c || !out2) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  Slot* s = find_ticket(c, t, false, nullptr);
  if (!s) return TBG_E_TICKET;
  // (the launch's own fields: launch_rlc_check took its path from the same ones)
  const DevBatch B = checked_batch(s->last);  // (TBG_OP_AGGREGATE_VERIFY: never by message)
  out2[0] = out2[1] = 0;
  if (s->op == TBG_OP_AGGREGATE || !B.rlc_batch || !B.rlc_group || !B.n_duties) return TBG_OK;
  const bool by_msg = l0_by_msg(B);
  const uint32_t n = by_msg ? B.n_msgs : B.n_duties;
  out2[0] = by_msg ? 1u : 0u;
  out2[1] = ((n + B.rlc_group - 1) / B.rlc_group) * ((B.rlc_group + B.rlc_chunk - 1) / B.rlc_chunk);
  return TBG_OK;
}

int tbg_fetch_level0(tbg_ctx* c, tbg_ticket t, int32_t* state) {
  if (!c || !state) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  Slot* s = find_ticket(c, t, false, nullptr);
  if (!s) return TBG_E_TICKET;
  *state = TBG_L0_NOT_RUN;
  const DevBatch L = checked_batch(s->last);  // (TBG_OP_AGGREGATE_VERIFY: the aggregates' checks)
  if (s->op == TBG_OP_AGGREGATE || !L.rlc_batch) return TBG_OK;
  HIP_TRY(hipSetDevice(c->device));
  uint32_t cnt[CNT_WORDS] = {};
  HIP_TRY(hipMemcpyAsync(cnt, L.counters, sizeof(cnt), hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  *state = cnt[CNT_L0_OK] ? TBG_L0_PASSED : TBG_L0_FAILED;
  return TBG_OK;
}

int tbg_last_timings(const tbg_ctx* c, float* ms8) {
  if (!c || !ms8) return TBG_E_INVALID_ARG;
  memcpy(ms8, c->last_ms, sizeof(c->last_ms));
  return TBG_OK;
}

}  // extern "C"

extern "C" {

int tbg_sk_to_pk(tbg_ctx* c, const uint8_t* sk32, uint32_t n, uint8_t* pk48) {
  if (!c || (n && (!sk32 || !pk48))) return TBG_E_INVALID_ARG;
  if (n == 0) return TBG_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  uint8_t *d_sk = nullptr, *d_pk = nullptr;
  if (hipMalloc(&d_sk, 32ull * n) != hipSuccess) return TBG_E_OOM;
  if (hipMalloc(&d_pk, 48ull * n) != hipSuccess) { hipFree(d_sk); return TBG_E_OOM; }
  int rc = TBG_OK;
  if (hipMemcpyAsync(d_sk, sk32, 32ull * n, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = TBG_E_DEVICE;
  if (rc == TBG_OK) {
    launch_sk_to_pk(d_sk, n, d_pk, c->stream);
    if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  }
  if (rc == TBG_OK && hipMemcpyAsync(pk48, d_pk, 48ull * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = TBG_E_DEVICE;
  if (hipStreamSynchronize(c->stream) != hipSuccess) rc = TBG_E_DEVICE;
  hipFree(d_sk);
  hipFree(d_pk);
  return rc;
}

int tbg_sign(tbg_ctx* c, const uint8_t* sk32, uint32_t n, const uint8_t* msgs, const uint32_t* msg_off, uint32_t n_msgs,
             const uint32_t* item_msg, uint8_t* sig96) {
  if (!c || (n && (!sk32 || !sig96 || !item_msg)) || n_msgs == 0 || !msg_off) return TBG_E_INVALID_ARG;
  if (msg_off[0] != 0) return TBG_E_INVALID_ARG;
  for (uint32_t m = 0; m < n_msgs; ++m)
    if (msg_off[m + 1] < msg_off[m]) return TBG_E_INVALID_ARG;
  for (uint32_t i = 0; i < n; ++i)
    if (item_msg[i] >= n_msgs) return TBG_E_INVALID_ARG;
  if (n == 0) return TBG_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  size_t mb = msg_off[n_msgs];
  size_t need = align_up(32ull * n, 16) + align_up(mb + 1, 16) + align_up(4ull * (n_msgs + 1), 16) + align_up(4ull * n, 16) +
                align_up(sizeof(G2A) * (size_t)n_msgs, 16) + align_up(4ull * n_msgs, 16) + align_up(96ull * n, 16) +
                align_up(3 * sizeof(G2J) * (size_t)n_msgs, 16);
  uint8_t* base = nullptr;
  if (hipMalloc(&base, need) != hipSuccess) return TBG_E_OOM;
  size_t o = 0;
  auto sec = [&](size_t bytes) { uint8_t* p = base + o; o += align_up(bytes, 16); return p; };
  uint8_t* d_sk = sec(32ull * n);
  uint8_t* d_msgs = sec(mb + 1);
  uint32_t* d_off = (uint32_t*)sec(4ull * (n_msgs + 1));
  uint32_t* d_im = (uint32_t*)sec(4ull * n);
  G2A* d_h = (G2A*)sec(sizeof(G2A) * (size_t)n_msgs);
  int32_t* d_hs = (int32_t*)sec(4ull * n_msgs);
  uint8_t* d_sig = sec(96ull * n);
  G2J* d_hj = (G2J*)sec(3 * sizeof(G2J) * (size_t)n_msgs);
  int rc = TBG_OK;
  hipStream_t st = c->stream;
  if (hipMemcpyAsync(d_sk, sk32, 32ull * n, hipMemcpyHostToDevice, st) != hipSuccess ||
      (mb && hipMemcpyAsync(d_msgs, msgs, mb, hipMemcpyHostToDevice, st) != hipSuccess) ||
      hipMemcpyAsync(d_off, msg_off, 4ull * (n_msgs + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d_im, item_msg, 4ull * n, hipMemcpyHostToDevice, st) != hipSuccess)
    rc = TBG_E_DEVICE;
  if (rc == TBG_OK) {
    DevBatch B{};
    memset(&B, 0, sizeof(B));
    B.n_msgs = n_msgs;
    B.msgs = d_msgs;
    B.msg_off = d_off;
    B.h_aff = d_h;
    B.h_status = d_hs;
    B.h_jac = d_hj;
    launch_hash_msgs(B, st);
    launch_sign(d_sk, d_im, n, d_h, d_hs, d_sig, st);
    if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  }
  if (rc == TBG_OK && hipMemcpyAsync(sig96, d_sig, 96ull * n, hipMemcpyDeviceToHost, st) != hipSuccess) rc = TBG_E_DEVICE;
  if (hipStreamSynchronize(st) != hipSuccess) rc = TBG_E_DEVICE;
  hipFree(base);
  return rc;
}

}  // extern "C"

// ---- the hardened signer (k_keyed.hip, bls_ctmul.h) ------------------------
namespace {

// TBG_KS_* of a 32-byte big-endian key: zero, or a word-wise compare against
// r -- every word is read and subtracted whatever the earlier ones were.
int32_t keyed_status(const uint8_t* b) {
  static const uint32_t R_W[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u,
                                  0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};  // r, little-endian words
  uint32_t nz = 0;
  uint64_t borrow = 0;
  for (int i = 0; i < 8; ++i) {
    const uint32_t w = ((uint32_t)b[31 - 4 * i]) | ((uint32_t)b[30 - 4 * i] << 8) | ((uint32_t)b[29 - 4 * i] << 16) |
                       ((uint32_t)b[28 - 4 * i] << 24);
    nz |= w;
    borrow = (((uint64_t)w - R_W[i] - borrow) >> 63) & 1u;
  }
  const int32_t ge = (int32_t)borrow - 1;                      // all ones: sk >= r (no final borrow)
  const int32_t zero = (int32_t)((nz | (0u - nz)) >> 31) - 1;  // all ones: sk == 0
  return (TBG_KS_ZERO & zero) | (TBG_KS_RANGE & ge & ~zero);
}

void keyed_wipe(void* p, size_t n) {
  volatile uint8_t* v = (volatile uint8_t*)p;
  for (size_t i = 0; i < n; ++i) v[i] = 0;
}

// Everything of one hardened call that held key bytes: the device copy of the
// keys (inside the call's workspace) and the pinned staging they were
// uploaded from.  Whatever way the call ends, the device bytes are zeroed ON
// THE STREAM (behind the kernels that read them), the stream is drained, the
// staging is zeroed, and only then is either released.
struct KeyedScope {
  hipStream_t st = nullptr;
  uint8_t* d_base = nullptr;  // the workspace (hipMalloc)
  uint8_t* d_sk = nullptr;    // [sk_bytes] inside it
  uint8_t* h_sk = nullptr;    // [sk_bytes] pinned (hipHostMalloc)
  size_t sk_bytes = 0;
  size_t o = 0;
  ~KeyedScope() {
    if (d_sk) (void)hipMemsetAsync(d_sk, 0, sk_bytes, st);
    (void)hipStreamSynchronize(st);
    if (h_sk) {
      keyed_wipe(h_sk, sk_bytes);
      (void)hipHostFree(h_sk);
    }
    if (d_base) (void)hipFree(d_base);
  }
  uint8_t* sec(size_t bytes) {
    uint8_t* p = d_base + o;
    o += align_up(bytes, 16);
    return p;
  }
  // The workspace and the staging; the keys go into the staging with every
  // rejected one replaced by 1 (masks, no branch on a key byte), their codes into kst.
  int open(hipStream_t stream, size_t work_bytes, const uint8_t* sk32, uint32_t n, std::vector<int32_t>& kst) {
    st = stream;
    sk_bytes = 32ull * n;
    if (hipMalloc(&d_base, work_bytes) != hipSuccess) { d_base = nullptr; return TBG_E_OOM; }
    if (hipHostMalloc((void**)&h_sk, sk_bytes, hipHostMallocDefault) != hipSuccess) { h_sk = nullptr; return TBG_E_OOM; }
    kst.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
      const uint8_t* k = sk32 + 32ull * i;
      kst[i] = keyed_status(k);
      const uint8_t keep = (uint8_t)(((uint32_t)kst[i] | (0u - (uint32_t)kst[i])) >> 31) - 1;  // 0xff: accepted
      for (int j = 0; j < 32; ++j) h_sk[32ull * i + j] = (uint8_t)((k[j] & keep) | ((j == 31 ? 1 : 0) & ~keep));
    }
    d_sk = sec(sk_bytes);
    return hipMemcpyAsync(d_sk, h_sk, sk_bytes, hipMemcpyHostToDevice, st) == hipSuccess ? TBG_OK : TBG_E_DEVICE;
  }
};

// the rejected keys' outputs and codes (their lanes ran on the key 1)
void keyed_mask(const std::vector<int32_t>& kst, uint8_t* out, size_t width, int32_t* status) {
  for (size_t i = 0; i < kst.size(); ++i) {
    if (kst[i] == TBG_KS_OK) continue;
    memset(out + width * i, 0, width);
    status[i] = kst[i];
  }
}

}  // namespace

extern "C" {

int tbg_sk_to_pk_ct(tbg_ctx* c, const uint8_t* sk32, uint32_t n, uint8_t* pk48, int32_t* status) {
  if (!c || (n && (!sk32 || !pk48 || !status))) return TBG_E_INVALID_ARG;
  if (n == 0) return TBG_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const size_t tab_bytes = 4 * ct_tab_words_g1();
  std::vector<int32_t> kst;
  KeyedScope ks;
  int rc = ks.open(c->stream, align_up(32ull * n, 16) + align_up(tab_bytes, 16) + align_up(48ull * n, 16) +
                                  align_up(4ull * n, 16), sk32, n, kst);
  if (rc != TBG_OK) return rc;
  hipStream_t st = c->stream;
  uint32_t* d_tab = (uint32_t*)ks.sec(tab_bytes);
  uint8_t* d_pk = ks.sec(48ull * n);
  int32_t* d_st = (int32_t*)ks.sec(4ull * n);
  launch_ct_table_g1(d_tab, st);
  launch_sk_to_pk_ct(ks.d_sk, n, d_tab, d_pk, d_st, st);
  if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  if (rc == TBG_OK && (hipMemcpyAsync(pk48, d_pk, 48ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
                       hipMemcpyAsync(status, d_st, 4ull * n, hipMemcpyDeviceToHost, st) != hipSuccess))
    rc = TBG_E_DEVICE;
  if (hipStreamSynchronize(st) != hipSuccess) rc = TBG_E_DEVICE;
  if (rc == TBG_OK) keyed_mask(kst, pk48, 48, status);
  return rc;
}

int tbg_sign_ct(tbg_ctx* c, const uint8_t* sk32, uint32_t n, const uint8_t* msgs, const uint32_t* msg_off, uint32_t n_msgs,
                const uint32_t* item_msg, uint8_t* sig96, int32_t* status) {
  if (!c || (n && (!sk32 || !sig96 || !item_msg || !status)) || n_msgs == 0 || !msg_off) return TBG_E_INVALID_ARG;
  if (msg_off[0] != 0) return TBG_E_INVALID_ARG;
  for (uint32_t m = 0; m < n_msgs; ++m)
    if (msg_off[m + 1] < msg_off[m]) return TBG_E_INVALID_ARG;
  for (uint32_t i = 0; i < n; ++i)
    if (item_msg[i] >= n_msgs) return TBG_E_INVALID_ARG;
  if (n == 0) return TBG_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const size_t mb = msg_off[n_msgs];
  const size_t tab_bytes = 4 * ct_tab_words_g2(n_msgs);
  const size_t need = align_up(32ull * n, 16) + align_up(mb + 1, 16) + align_up(4ull * (n_msgs + 1), 16) +
                      align_up(4ull * n, 16) + align_up(sizeof(G2A) * (size_t)n_msgs, 16) + align_up(4ull * n_msgs, 16) +
                      align_up(96ull * n, 16) + align_up(3 * sizeof(G2J) * (size_t)n_msgs, 16) + align_up(tab_bytes, 16) +
                      align_up(4ull * n, 16);
  std::vector<int32_t> kst;
  KeyedScope ks;
  int rc = ks.open(c->stream, need, sk32, n, kst);
  if (rc != TBG_OK) return rc;
  hipStream_t st = c->stream;
  uint8_t* d_msgs = ks.sec(mb + 1);
  uint32_t* d_off = (uint32_t*)ks.sec(4ull * (n_msgs + 1));
  uint32_t* d_im = (uint32_t*)ks.sec(4ull * n);
  G2A* d_h = (G2A*)ks.sec(sizeof(G2A) * (size_t)n_msgs);
  int32_t* d_hs = (int32_t*)ks.sec(4ull * n_msgs);
  uint8_t* d_sig = ks.sec(96ull * n);
  G2J* d_hj = (G2J*)ks.sec(3 * sizeof(G2J) * (size_t)n_msgs);
  uint32_t* d_tab = (uint32_t*)ks.sec(tab_bytes);
  int32_t* d_st = (int32_t*)ks.sec(4ull * n);
  if ((mb && hipMemcpyAsync(d_msgs, msgs, mb, hipMemcpyHostToDevice, st) != hipSuccess) ||
      hipMemcpyAsync(d_off, msg_off, 4ull * (n_msgs + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d_im, item_msg, 4ull * n, hipMemcpyHostToDevice, st) != hipSuccess)
    rc = TBG_E_DEVICE;
  if (rc == TBG_OK) {
    DevBatch B{};
    memset(&B, 0, sizeof(B));
    B.n_msgs = n_msgs;
    B.msgs = d_msgs;
    B.msg_off = d_off;
    B.h_aff = d_h;
    B.h_status = d_hs;
    B.h_jac = d_hj;
    launch_hash_msgs(B, st);
    launch_ct_table_g2(d_h, d_hs, n_msgs, d_tab, st);
    launch_sign_ct(ks.d_sk, d_im, n, n_msgs, d_tab, d_hs, d_sig, d_st, st);
    if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  }
  if (rc == TBG_OK && (hipMemcpyAsync(sig96, d_sig, 96ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
                       hipMemcpyAsync(status, d_st, 4ull * n, hipMemcpyDeviceToHost, st) != hipSuccess))
    rc = TBG_E_DEVICE;
  if (hipStreamSynchronize(st) != hipSuccess) rc = TBG_E_DEVICE;
  if (rc == TBG_OK) keyed_mask(kst, sig96, 96, status);
  return rc;
}

// ---- plain sums and FastAggregateVerify (k_sum.hip) -----------------------
// dkg/dkg.go:466-476 (AggregateSignatures / AggregatePublicKeys of the lock
// hash), cluster/lock.go:155-177 (FastAggregateVerify over every pubshare).

}  // extern "C"

namespace {

// One device allocation for a utility call, freed on scope exit.
struct DevArena {
  uint8_t* base = nullptr;
  size_t o = 0;
  ~DevArena() {
    if (base) hipFree(base);
  }
  int alloc(size_t bytes) { return hipMalloc(&base, bytes ? bytes : 16) == hipSuccess ? TBG_OK : TBG_E_OOM; }
  uint8_t* sec(size_t bytes) {
    uint8_t* p = base + o;
    o += align_up(bytes, 16);
    return p;
  }
};

bool offsets_ok(const uint32_t* off, uint32_t n_sets) {
  if (!off || off[0] != 0) return false;
  for (uint32_t s = 0; s < n_sets; ++s)
    if (off[s + 1] < off[s]) return false;
  return true;
}

// Host half of a sum plan and its device copy inside `a`.
struct SumHost {
  std::vector<uint32_t> chunk_first, chunk_set;
  static size_t bytes(uint32_t n_sets, uint32_t n_chunks, size_t part_elem) {
    return align_up(4ull * (n_sets + 1), 16) * 2 + align_up(4ull * n_chunks + 4, 16) +
           align_up(part_elem * n_chunks + 16, 16) + align_up(4ull * n_sets + 4, 16);
  }
  SumHost(const uint32_t* off, uint32_t n_sets) {
    const uint32_t ch = tbg::sum_chunk_size();
    chunk_first.resize(n_sets + 1);
    chunk_first[0] = 0;
    for (uint32_t s = 0; s < n_sets; ++s) {
      const uint32_t nc = (off[s + 1] - off[s] + ch - 1) / ch;
      chunk_first[s + 1] = chunk_first[s] + nc;
      for (uint32_t k = 0; k < nc; ++k) chunk_set.push_back(s);
    }
  }
  uint32_t n_chunks() const { return chunk_first.back(); }
  int upload(DevArena& a, const uint32_t* off, uint32_t n_sets, size_t part_elem, hipStream_t st, tbg::SumPlan& p) {
    uint32_t* d_off = (uint32_t*)a.sec(4ull * (n_sets + 1));
    uint32_t* d_cf = (uint32_t*)a.sec(4ull * (n_sets + 1));
    uint32_t* d_cs = (uint32_t*)a.sec(4ull * n_chunks() + 4);
    p.part = a.sec(part_elem * n_chunks() + 16);
    p.set_bad = (int32_t*)a.sec(4ull * n_sets + 4);
    p.n_sets = n_sets;
    p.n_chunks = n_chunks();
    p.off = d_off;
    p.chunk_first = d_cf;
    p.chunk_set = d_cs;
    if (hipMemcpyAsync(d_off, off, 4ull * (n_sets + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_cf, chunk_first.data(), 4ull * (n_sets + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
        (n_chunks() && hipMemcpyAsync(d_cs, chunk_set.data(), 4ull * n_chunks(), hipMemcpyHostToDevice, st) != hipSuccess) ||
        hipMemsetAsync(p.set_bad, 0, 4ull * n_sets, st) != hipSuccess)
      return TBG_E_DEVICE;
    return TBG_OK;
  }
};

}  // namespace

extern "C" {

int tbg_sum_pubkeys(tbg_ctx* c, const uint32_t* pubkey_ids, const uint32_t* off, uint32_t n_sets, uint8_t* out48,
                    int32_t* status) {
  if (!c || !n_sets || !out48 || !status || !offsets_ok(off, n_sets)) return TBG_E_INVALID_ARG;
  const uint32_t ni = off[n_sets];
  if (ni && !pubkey_ids) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  SumHost h(off, n_sets);
  DevArena a;
  int rc = a.alloc(SumHost::bytes(n_sets, h.n_chunks(), sizeof(G1J)) + align_up(4ull * ni + 4, 16) +
                   align_up(48ull * n_sets, 16) + align_up(4ull * n_sets, 16));
  if (rc != TBG_OK) return rc;
  hipStream_t st = c->stream;
  tbg::SumPlan p;
  if ((rc = h.upload(a, off, n_sets, sizeof(G1J), st, p)) != TBG_OK) return rc;
  uint32_t* d_ids = (uint32_t*)a.sec(4ull * ni + 4);
  uint8_t* d_out = a.sec(48ull * n_sets);
  int32_t* d_st = (int32_t*)a.sec(4ull * n_sets);
  if (ni) HIP_TRY(hipMemcpyAsync(d_ids, pubkey_ids, 4ull * ni, hipMemcpyHostToDevice, st));
  tbg::launch_sum_g1(c->d_pk, c->d_pk_status, c->n_pk, d_ids, p, d_out, d_st, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out48, d_out, 48ull * n_sets, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(status, d_st, 4ull * n_sets, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return TBG_OK;
}

int tbg_sum_sigs(tbg_ctx* c, const uint8_t* sigs96, const uint32_t* off, uint32_t n_sets, uint8_t* out96,
                 int32_t* status, int32_t* sig_status) {
  if (!c || !n_sets || !out96 || !status || !offsets_ok(off, n_sets)) return TBG_E_INVALID_ARG;
  const uint32_t ni = off[n_sets];
  if (ni && !sigs96) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  SumHost h(off, n_sets);
  DevArena a;
  int rc = a.alloc(SumHost::bytes(n_sets, h.n_chunks(), sizeof(G2J)) + align_up(96ull * ni + 4, 16) +
                   align_up(4ull * ni + 4, 16) + align_up(96ull * n_sets, 16) + align_up(4ull * n_sets, 16));
  if (rc != TBG_OK) return rc;
  hipStream_t st = c->stream;
  tbg::SumPlan p;
  if ((rc = h.upload(a, off, n_sets, sizeof(G2J), st, p)) != TBG_OK) return rc;
  uint8_t* d_sigs = a.sec(96ull * ni + 4);
  int32_t* d_sst = (int32_t*)a.sec(4ull * ni + 4);
  uint8_t* d_out = a.sec(96ull * n_sets);
  int32_t* d_st = (int32_t*)a.sec(4ull * n_sets);
  if (ni) HIP_TRY(hipMemcpyAsync(d_sigs, sigs96, 96ull * ni, hipMemcpyHostToDevice, st));
  tbg::launch_sum_g2(d_sigs, p, d_out, d_st, d_sst, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out96, d_out, 96ull * n_sets, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(status, d_st, 4ull * n_sets, hipMemcpyDeviceToHost, st));
  if (sig_status && ni) HIP_TRY(hipMemcpyAsync(sig_status, d_sst, 4ull * ni, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return TBG_OK;
}

int tbg_fast_aggregate_verify(tbg_ctx* c, const uint32_t* pubkey_ids, const uint32_t* key_off, uint32_t n_sets,
                              const uint8_t* msgs, const uint32_t* msg_off, const uint8_t* sigs96, int32_t* status) {
  if (!c || !n_sets || !sigs96 || !status || !offsets_ok(key_off, n_sets) || !offsets_ok(msg_off, n_sets))
    return TBG_E_INVALID_ARG;
  const uint32_t nk = key_off[n_sets];
  const size_t mb = msg_off[n_sets];
  if ((nk && !pubkey_ids) || (mb && !msgs)) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t n = n_sets;
  SumHost h(key_off, n);
  std::vector<uint32_t> iota(n + 1);
  for (uint32_t i = 0; i <= n; ++i) iota[i] = i;
  const size_t lines = 4ull * LINES_WORDS * n;
  DevArena a;
  int rc = a.alloc(SumHost::bytes(n, h.n_chunks(), sizeof(G1J)) + align_up(4ull * nk + 4, 16) +
                   align_up(48ull * n, 16) * 2 + align_up(sizeof(G1A) * n, 16) * 2 + align_up(4ull * n, 16) * 6 +
                   align_up(mb + 1, 16) + align_up(4ull * (n + 1), 16) * 2 + align_up(96ull * n, 16) + align_up(n, 16) +
                   align_up(sizeof(G2A) * n, 16) * 2 + align_up(3 * sizeof(G2J) * n, 16) + 2 * align_up(lines, 16) +
                   align_up(4ull * tbg::CNT_WORDS, 16));
  if (rc != TBG_OK) return rc;
  hipStream_t st = c->stream;
  // 1. the key sums, compressed, then decoded into a table of their own
  tbg::SumPlan p;
  if ((rc = h.upload(a, key_off, n, sizeof(G1J), st, p)) != TBG_OK) return rc;
  uint32_t* d_ids = (uint32_t*)a.sec(4ull * nk + 4);
  uint8_t* d_pk48 = a.sec(48ull * n);
  int32_t* d_kst = (int32_t*)a.sec(4ull * n);
  G1A* t_pk = (G1A*)a.sec(sizeof(G1A) * n);
  G1A* t_xpk = (G1A*)a.sec(sizeof(G1A) * n);
  int32_t* t_pkst = (int32_t*)a.sec(4ull * n);
  if (nk) HIP_TRY(hipMemcpyAsync(d_ids, pubkey_ids, 4ull * nk, hipMemcpyHostToDevice, st));
  tbg::launch_sum_g1(c->d_pk, c->d_pk_status, c->n_pk, d_ids, p, d_pk48, d_kst, st);
  tbg::launch_decode_pubkeys(d_pk48, n, t_pk, t_xpk, t_pkst, st);  // a failed / identity sum: not DEC_OK
  // 2. one CoreVerify per set against that table (the per-item schedule)
  DevBatch B{};
  memset(&B, 0, sizeof(B));
  B.op = TBG_OP_VERIFY;
  B.n_duties = B.n_partials = B.n_msgs = n;
  uint8_t* d_msgs = a.sec(mb + 1);
  uint32_t* d_moff = (uint32_t*)a.sec(4ull * (n + 1));
  uint32_t* d_iota = (uint32_t*)a.sec(4ull * (n + 1));
  uint8_t* d_sigs = a.sec(96ull * n);
  uint8_t* d_idf = a.sec(n);
  B.msgs = d_msgs;
  B.msg_off = d_moff;
  B.duty_msg = B.duty_first = B.partial_duty = B.pubkey_ids = d_iota;
  B.duty_threshold = d_iota;  // unused by TBG_OP_VERIFY
  B.sigs = d_sigs;
  B.identifiers = d_idf;
  B.sig_aff = (G2A*)a.sec(sizeof(G2A) * n);
  B.h_aff = (G2A*)a.sec(sizeof(G2A) * n);
  B.h_status = (int32_t*)a.sec(4ull * n);
  B.h_jac = (G2J*)a.sec(3 * sizeof(G2J) * n);
  B.sig_lines = (uint32_t*)a.sec(lines);
  B.h_lines = (uint32_t*)a.sec(lines);
  B.counters = (uint32_t*)a.sec(4ull * tbg::CNT_WORDS);
  B.part_list = (uint32_t*)a.sec(4ull * n);
  B.partial_status = (int32_t*)a.sec(4ull * n);
  B.duty_status = (int32_t*)a.sec(4ull * n);
  B.rlc_group = 0;
  B.fb_full = 0xFFFFFFFFu;
  if (mb) HIP_TRY(hipMemcpyAsync(d_msgs, msgs, mb, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_moff, msg_off, 4ull * (n + 1), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_iota, iota.data(), 4ull * (n + 1), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_sigs, sigs96, 96ull * n, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_idf, 0, n, st));
  HIP_TRY(hipMemsetAsync(B.counters, 0, 4 * tbg::CNT_WORDS, st));
  tbg::launch_decode_sigs(B, st);
  tbg::launch_hash_msgs(B, st);
  tbg::launch_h_lines(B, st);
  tbg::launch_rlc_prepare(B, t_pk, nullptr, t_pkst, n, st);
  tbg::launch_rlc_check(B, t_pk, nullptr, t_pkst, n, st);  // (per-item schedule: no key table)
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(status, B.partial_status, 4ull * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return TBG_OK;
}

}  // extern "C"
