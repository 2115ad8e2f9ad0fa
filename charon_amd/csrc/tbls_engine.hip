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
#include "tbls_plan.h"
#include "tbls_work.h"
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
  tbg::LaunchLayout L{};       // the batch's counts and plan, and where its sections lie in the arenas (tbls_plan.h)
};

}  // namespace

// (PlanConfig: the fields that planning reads, tbls_plan.h)
struct tbg_ctx : tbg::PlanConfig {
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
  uint64_t rlc_seed = 0;   // 0 = OS randomness per batch
  uint64_t seed_ctr = 0;
  uint32_t express_max = TBG_EXPRESS_PARTIALS;  // batches up to this many partials prefer the express slot
  // host-side work of the submit / collect calls (tbg_host_stats): [submits,
  // partials submitted, pack ns, enqueue ns, collects, partials collected,
  // gather ns, wait ns]
  std::atomic<uint64_t> host[8] = {};
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

// n + 1 offsets of n consecutive ranges: from 0, non-decreasing.
static bool offsets_ok(const uint32_t* off, uint32_t n) {
  if (!off || off[0] != 0) return false;
  for (uint32_t s = 0; s < n; ++s)
    if (off[s + 1] < off[s]) return false;
  return true;
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
    if (!b->duty_msg || !b->pubkey_ids || b->n_msgs == 0 || !offsets_ok(b->msg_off, b->n_msgs)) return TBG_E_INVALID_ARG;
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

// A collected ticket's slot for the reads below: the context's lock held while
// this lives, the slot found (rc TBG_E_TICKET otherwise) and the device set.
struct Collected {
  std::lock_guard<std::mutex> lk;
  Slot* s;
  int rc;
  Collected(tbg_ctx* c, tbg_ticket t) : lk(c->mu), s(find_ticket(c, t, false, nullptr)) {
    rc = !s ? TBG_E_TICKET : hipSetDevice(c->device) != hipSuccess ? TBG_E_DEVICE : TBG_OK;
  }
};

// The counters of the checks that B (the slot's last run) made; zeros after TBG_OP_AGGREGATE, which makes none.
static int read_counters(const Slot* s, const DevBatch& B, uint32_t (&cnt)[CNT_WORDS]) {
  memset(cnt, 0, sizeof(cnt));
  if (s->L.dims.op == TBG_OP_AGGREGATE) return TBG_OK;
  HIP_TRY(hipMemcpyAsync(cnt, B.counters, sizeof(cnt), hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  return TBG_OK;
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

// ---- submit_impl's steps, in its order.  What a launch decides (plan_launch)
// and where its sections lie (layout, bind) is tbls_plan.h's. ----

// The caller batches of one submit.
struct SubmitInput {
  const tbg_batch* const* bs;
  uint32_t n_batches;
  const uint32_t* set_first;  // a set launch (one batch), else null
  uint32_t n_sets;
};

// Validate the batches and total their counts (d) and per-batch duties and
// messages (dm, plan_launch's batch_dm).
static int total_inputs(const SubmitInput& in, LaunchDims& d, std::vector<uint32_t>& dm) {
  int rc;
  for (uint32_t k = 0; k < in.n_batches; ++k) {
    if ((rc = validate(in.bs[k])) != TBG_OK) return rc;
    if (in.bs[k]->op != in.bs[0]->op) return TBG_E_INVALID_ARG;  // one kernel chain per device batch
  }
  d.op = in.bs[0]->op;
  const bool verify = d.op != TBG_OP_AGGREGATE;
  if (d.op == TBG_OP_AGGREGATE_VERIFY && in.set_first) return TBG_E_INVALID_ARG;
  uint64_t nd64 = 0, np64 = 0, nm64 = 0, mb64 = 0;
  for (uint32_t k = 0; k < in.n_batches; ++k) {
    const tbg_batch* b = in.bs[k];
    nd64 += b->n_duties;
    np64 += b->n_partials;
    if (verify) {
      nm64 += b->n_msgs;
      mb64 += b->msg_off[b->n_msgs];
    }
    dm.push_back(b->n_duties);
    dm.push_back(b->n_msgs);
  }
  if (np64 > 0x7FFFFFFFull || nd64 > 0x7FFFFFFFull || nm64 > 0x7FFFFFFFull || mb64 > 0xFFFFFFFFull)
    return TBG_E_INVALID_ARG;
  d.n_duties = (uint32_t)nd64;
  d.n_partials = (uint32_t)np64;
  d.n_msgs = (uint32_t)nm64;
  d.msg_bytes = (size_t)mb64;
  d.sets = in.set_first != nullptr;
  d.n_sets = d.sets ? in.n_sets : 0;
  return TBG_OK;
}

// Least recently used free slot: a collected batch stays resident (for
// tbg_replay / tbg_fetch) until every other slot has been reused.  A batch
// of at most express_max partials takes the express slot when it is free.
static Slot* free_slot(tbg_ctx* c, uint32_t n_partials) {
  Slot* s = nullptr;
  const bool small = n_partials <= c->express_max;
  for (auto& x : c->slots)
    if (x.express && small && !x.busy) s = &x;
  if (!s)
    for (auto& x : c->slots)
      if (!x.express && !x.busy && (!s || x.ticket < s->ticket)) s = &x;
  return s;
}

static int grow_slot(Slot* s, const LaunchLayout& L) {
  int rc;
  if ((rc = grow_pinned(&s->h_in, &s->h_in_cap, L.in_bytes)) != TBG_OK) return rc;
  if ((rc = grow_pinned(&s->h_out, &s->h_out_cap, L.out_bytes)) != TBG_OK) return rc;
  if ((rc = grow_device(&s->d_in, &s->d_in_cap, L.in_bytes)) != TBG_OK) return rc;
  return grow_device(&s->d_work, &s->d_work_cap, L.work_bytes);
}

// ---- pack: no HIP call, no lock.  H is the launch's sections in the pinned
// input image (bind over h_in), which is the packers' to write. ----

// Batch k's duties / partials / messages follow batch k-1's (mb0: its first
// message byte); a set launch's one part spans the padded device batch.
static std::vector<Part> place_parts(const SubmitInput& in, const LaunchDims& d, std::vector<uint32_t>& mb0) {
  std::vector<Part> parts(in.n_batches);
  mb0.resize(in.n_batches);
  const bool verify = d.op != TBG_OP_AGGREGATE;
  uint32_t D = 0, P = 0, M = 0, MB = 0;
  for (uint32_t k = 0; k < in.n_batches; ++k) {
    const tbg_batch* b = in.bs[k];
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
  if (d.sets) parts[0].nd = d.n_duties;
  return parts;
}

// One caller batch into its place, every index rebased by the running offsets.
static void pack_batch(const tbg_batch* b, const Part& q, uint32_t MB, const DevBatch& H, const LaunchPlan& plan) {
  const uint32_t D = q.d0, P = q.p0, M = q.m0;
  const uint32_t bnd = b->n_duties, bnp = b->n_partials, bnm = q.nm;
  uint32_t* msg_off = (uint32_t*)H.msg_off;
  uint32_t* duty_msg = (uint32_t*)H.duty_msg;
  uint32_t* duty_first = (uint32_t*)H.duty_first;
  uint32_t* thr = (uint32_t*)H.duty_threshold;
  uint32_t* pd = (uint32_t*)H.partial_duty;
  if (H.op != TBG_OP_AGGREGATE) {
    const uint32_t bmb = b->msg_off[bnm];
    if (bmb) memcpy((uint8_t*)H.msgs + MB, b->msgs, bmb);
    for (uint32_t m = 0; m < bnm; ++m) msg_off[M + m] = MB + b->msg_off[m];
    for (uint32_t d = 0; d < bnd; ++d) duty_msg[D + d] = M + b->duty_msg[d];
    if (plan.aggver) memcpy((uint32_t*)H.pubkey_ids + D, b->pubkey_ids, 4ull * bnd);  // (one group key per duty)
    else memcpy((uint32_t*)H.pubkey_ids + P, b->pubkey_ids, 4ull * bnp);
    if (plan.l0m) {  // this batch's duties by message (sections disjoint from the other batches')
      std::vector<uint32_t> cursor(bnm);
      l0m_sort_batch(duty_msg, D, bnd, M, bnm, (uint32_t*)H.msg_first, (uint32_t*)H.msg_duty, cursor.data());
    }
  }
  for (uint32_t d = 0; d < bnd; ++d) {
    duty_first[D + d] = P + b->duty_first[d];
    for (uint32_t j = b->duty_first[d]; j < b->duty_first[d + 1]; ++j) pd[P + j] = D + d;
  }
  if (H.op == TBG_OP_VERIFY_AGGREGATE) memcpy(thr + D, b->duty_threshold, 4ull * bnd);
  else memset(thr + D, 0, 4ull * bnd);
  if (bnp) {
    memcpy((uint8_t*)H.sigs + 96ull * P, b->sigs, 96ull * bnp);
    memcpy((uint8_t*)H.identifiers + P, b->identifiers, bnp);
  }
}

// A set launch (one caller batch): the duties move to their padded places,
// set k's first on a multiple of Gp; a padding duty is empty (no partials,
// message 0), which k_rlc_duty_sum leaves RLC_NONE.  Partials and messages
// keep their indices.
static void pack_sets(const SubmitInput& in, const DevBatch& H, const LaunchPlan& plan) {
  const tbg_batch* b = in.bs[0];
  const uint32_t Gp = plan.G ? plan.G : 1;
  const uint32_t nd = H.n_duties, np = H.n_partials, nm = H.n_msgs;
  uint32_t* duty_msg = (uint32_t*)H.duty_msg;
  uint32_t* duty_first = (uint32_t*)H.duty_first;
  uint32_t* pd = (uint32_t*)H.partial_duty;
  uint32_t* dset = (uint32_t*)H.duty_set;
  if (b->msg_off[nm]) memcpy((uint8_t*)H.msgs, b->msgs, b->msg_off[nm]);
  memcpy((uint32_t*)H.msg_off, b->msg_off, 4ull * nm);
  if (np) {
    memcpy((uint32_t*)H.pubkey_ids, b->pubkey_ids, 4ull * np);
    memcpy((uint8_t*)H.sigs, b->sigs, 96ull * np);
    memcpy((uint8_t*)H.identifiers, b->identifiers, np);
  }
  uint32_t e = 0;
  for (uint32_t k = 0; k < in.n_sets; ++k) {
    const uint32_t a = in.set_first[k], z = in.set_first[k + 1];
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
  memset((uint32_t*)H.duty_threshold, 0, 4ull * nd);
  if (plan.l0m) {  // (the padded duties: a padding duty names message 0 and is never combined)
    std::vector<uint32_t> cursor(nm);
    l0m_sort_batch(duty_msg, 0, nd, 0, nm, (uint32_t*)H.msg_first, (uint32_t*)H.msg_duty, cursor.data());
  }
}

// The whole input image: every caller batch packed by its own worker (the
// sections are disjoint: a 16-batch group is ~70 MB of host copies, which one
// thread would take longer to pack than the GPU takes to run it), the arrays'
// closing entries, and level 0's chunk plan (parts[k].ch1, .maxch).
static void pack_input(const SubmitInput& in, std::vector<Part>& parts, const std::vector<uint32_t>& mb0, const DevBatch& H,
                       const LaunchLayout& L) {
  const LaunchPlan& plan = L.plan;
  const uint32_t n_batches = in.n_batches, nd = H.n_duties, np = H.n_partials, nm = H.n_msgs;
  if (plan.l0m) ((uint32_t*)H.msg_first)[0] = 0;
  const uint32_t workers = (np >= (1u << 16) && n_batches > 1) ? std::min<uint32_t>(n_batches, 8) : 1;
  if (in.set_first) {
    pack_sets(in, H, plan);
  } else if (workers == 1) {
    for (uint32_t k = 0; k < n_batches; ++k) pack_batch(in.bs[k], parts[k], mb0[k], H, plan);
  } else {
    std::vector<std::thread> th;
    for (uint32_t w = 0; w < workers; ++w)
      th.emplace_back([&, w] {
        for (uint32_t k = w; k < n_batches; k += workers) pack_batch(in.bs[k], parts[k], mb0[k], H, plan);
      });
    for (auto& t : th) t.join();
  }
  ((uint32_t*)H.duty_first)[nd] = np;
  if (H.op != TBG_OP_AGGREGATE) ((uint32_t*)H.msg_off)[nm] = (uint32_t)L.dims.msg_bytes;
  if (plan.aggver)
    for (uint32_t d = 0; d <= nd; ++d) ((uint32_t*)H.av_iota)[d] = d;
  // Level 0 by message, the chunk plan (chunk -> message, message -> first
  // chunk; the shape of SumPlan, k_sum.hip).  Invariant: the messages of
  // caller batch j follow those of batch j - 1 and a message never spans
  // caller batches (every batch brings its own), so batch j's duties, CSR
  // rows and chunks all follow batch j - 1's -- the first n_msgs entries of
  // msg_first / chunk_first, with the duties and chunks they cover, are a
  // prefix's own plan (tbg_replay_plan n_parts; Part::ch1, ::maxch).
  if (plan.l0m) {
    uint32_t nc = 0, largest = 0;
    for (uint32_t k = 0; k < n_batches; ++k) {
      const uint32_t big = l0m_chunk_plan(H.msg_first, parts[k].m0, parts[k].nm, (uint32_t*)H.l0m_chunk_first,
                                          (uint32_t*)H.l0m_chunk_msg, &nc);
      largest = std::max(largest, big);
      parts[k].ch1 = nc;
      parts[k].maxch = largest;
    }
  }
}

// The launch's secret keys: of the RLC scalars, and of the subgroup test's digits.
static void draw_seeds(tbg_ctx* c, DevBatch& B) {
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

// One H2D copy of the input image, the kernel chain, one D2H copy of the outputs.
static int enqueue(tbg_ctx* c, Slot* s, const DevBatch& B, const LaunchLayout& L) {
  hipStream_t st = s->st;
  // The resident pubkey table may have been (re)loaded on the utility stream
  // (already complete: tbg_load_pubkeys waits for it; ordered anyway).
  HIP_TRY(hipStreamWaitEvent(st, c->keys_ready, 0));
  HIP_TRY(hipMemcpyAsync(s->d_in, s->h_in, L.in_bytes, hipMemcpyHostToDevice, st));
  const int rc = launch_chain(c, *s, B, s->ev);
  if (rc != TBG_OK) return rc;
  HIP_TRY(hipMemcpyAsync(s->h_out, s->d_work + L.w_out, L.out_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(s->done, st));
  return TBG_OK;
}

static int submit_impl(tbg_ctx* c, const tbg_batch* const* bs, uint32_t n_batches, tbg_ticket* tickets,
                       const uint32_t* set_first, uint32_t n_sets) {
  if (!c || !bs || !tickets || n_batches == 0) return TBG_E_INVALID_ARG;
  const SubmitInput in{bs, n_batches, set_first, n_sets};
  LaunchDims d;
  std::vector<uint32_t> dm;
  int rc = total_inputs(in, d, dm);
  if (rc != TBG_OK) return rc;
  std::unique_lock<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  Slot* s = free_slot(c, d.n_partials);
  if (!s) return TBG_E_BUSY;
  const LaunchPlan plan = plan_launch(*c, d, set_first, dm.data(), n_batches);  // (pads d.n_duties for a set launch)
  c->rlc_group = plan.rlc_group_cfg;
  if (!plan.ok) return TBG_E_INVALID_ARG;
  const LaunchLayout L = layout(plan, d);
  if ((rc = grow_slot(s, L)) != TBG_OK) return rc;
  // Reserve the slot (busy, its old tickets expired) and pack WITHOUT the
  // context lock: a 16-batch group is ~70 MB of host copies, during which
  // other threads' tbg_poll / tbg_collect / tbg_submit must not wait.
  s->parts.clear();
  s->busy = true;
  lk.unlock();
  const auto t_pack = std::chrono::steady_clock::now();
  DevBatch H{};
  memset(&H, 0, sizeof(H));
  bind(H, L, s->h_in, nullptr);
  std::vector<uint32_t> mb0;
  std::vector<Part> parts = place_parts(in, d, mb0);
  pack_input(in, parts, mb0, H, L);
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
  bind(B, L, s->d_in, s->d_work);
  B.l0m_n_chunks = plan.l0m ? parts[n_batches - 1].ch1 : 0;
  B.l0m_max_chunks = plan.l0m ? parts[n_batches - 1].maxch : 0;
  draw_seeds(c, B);
  if ((rc = enqueue(c, s, B, L)) != TBG_OK) return release(rc);
  {
    const auto t_end = std::chrono::steady_clock::now();
    using ns = std::chrono::nanoseconds;
    c->host[0] += 1;
    c->host[1] += d.n_partials;
    c->host[2] += (uint64_t)std::chrono::duration_cast<ns>(t_packed - t_pack).count();
    c->host[3] += (uint64_t)std::chrono::duration_cast<ns>(t_end - t_packed).count();
  }
  // the slot holds the launch from here on: its parts get their tickets
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
  s->B = B;
  s->last = B;
  s->L = L;
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

// The output sections in the slot's pinned image: derived from h_out and the
// layout at each use, never kept (a later submit may regrow h_out and fail
// before it takes the slot over, and the resident batch is still fetched).
static DevBatch host_outputs(const Slot* s) {
  DevBatch O{};
  memset(&O, 0, sizeof(O));
  bind(O, s->L, nullptr, nullptr, s->h_out);
  return O;
}

// A part's slice of the slot's (pinned) output image.
static void copy_part(const DevBatch& O, const Part& q, int32_t* pst, int32_t* dst, uint8_t* agg) {
  if (pst) memcpy(pst, O.partial_status + q.p0, 4ull * q.np);
  if (dst) memcpy(dst, O.duty_status + q.d0, 4ull * q.nd);
  if (agg) memcpy(agg, O.agg + 96ull * q.d0, 96ull * q.nd);
}

static void part_done(Slot* s, Part* q) {
  q->pending = false;
  bool any = false;
  for (const auto& x : s->parts) any |= x.pending;
  s->busy = any;
}

// A set launch's slice of the output image: the sets' statuses, and the
// partial statuses (partials keep their caller indices in the padded batch).
static void copy_sets(const DevBatch& O, int32_t* sst, int32_t* pst) {
  if (sst) memcpy(sst, O.set_status, 4ull * O.n_sets);
  if (pst) memcpy(pst, O.partial_status, 4ull * O.n_partials);
}

// tbg_collect (sets = false) and tbg_collect_sets (sets = true: sst / pst).
static int collect_impl(tbg_ctx* c, tbg_ticket t, int32_t* pst, int32_t* dst, uint8_t* agg, int32_t* sst, bool sets,
                        int block) {
  if (!c) return TBG_E_INVALID_ARG;
  std::unique_lock<std::mutex> lk(c->mu);
  Part* q = nullptr;
  Slot* s = find_ticket(c, t, true, &q);
  if (!s || q->collecting || s->L.dims.sets != sets) return TBG_E_TICKET;
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
  const DevBatch O = host_outputs(s);
  if (sets) copy_sets(O, sst, pst);
  else copy_part(O, *q, pst, dst, agg);
  if (sets) {
    // every candidate of a failed group counts as invalid: an upper bound of
    // the invalid share, so level 0 switches off under bad sets as it does
    // under bad partials
    s->seen_bad += (uint32_t)O.set_status[O.n_sets + SET_BAD];
    s->seen_total += q->np;
  } else if (s->L.dims.op == TBG_OP_AGGREGATE_VERIFY) {  // the duties whose aggregate failed, over the duties checked
    const int32_t* ds = O.duty_status;
    uint32_t bad = 0, checked = 0;
    for (uint32_t d = 0; d < q->nd; ++d) {
      const int32_t v = ds[q->d0 + d];
      bad += v == TBG_DS_AGG_INVALID ? 1u : 0u;
      checked += v == TBG_DS_AGG_INVALID || v == TBG_DS_OK ? 1u : 0u;
    }
    s->seen_bad += bad;
    s->seen_total += checked;
  } else if (s->L.dims.op != TBG_OP_AGGREGATE && q->np) {  // the adaptive group size's and level 0's input
    const int32_t* st = O.partial_status;
    uint32_t bad = 0;
    for (uint32_t i = 0; i < q->np; ++i) bad += st[q->p0 + i] == TBG_PS_INVALID ? 1u : 0u;
    s->seen_bad += bad;
    s->seen_total += q->np;
  }
  if (q->np) {  // the batched subgroup test's input: non-subgroup share of all partials
    const int32_t* st = O.partial_status;
    uint32_t ns = 0;
    for (uint32_t i = 0; i < q->np; ++i) ns += st[q->p0 + i] == TBG_PS_ERR_SUBGROUP ? 1u : 0u;
    s->seen_nsub += ns;
    s->seen_dec += q->np;
  }
  c->host[4] += 1;
  c->host[5] += q->np;
  c->host[6] += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() -
                                                                               t_gather).count();
  chain_times(s->ev, s->ms, s->L.dims.op);
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
        B.sgb_m = sgb_group_size(*c, B.n_partials, sl[k]->L.plan.sgb_m_small, true);
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
    // their duties together (l0_shape), where each launch's arena fits it (shape_fits).
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
          if (!shape_fits(sl[k]->L, bs[k].n_duties, bs[k].n_partials, bs[k].n_msgs, g, ch)) return false;
        return true;
      };
      if (all_l0) l0_shape(nd, c->n_simd, true, G, C, fits_all);
      for (uint32_t k = k0; k < k1 && all_l0; ++k)
        if (shape_fits(sl[k]->L, bs[k].n_duties, bs[k].n_partials, bs[k].n_msgs, G, C)) {
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
  if (!s || s->L.dims.sets != sets) return TBG_E_TICKET;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(s->h_out, s->d_work + s->L.w_out, s->L.out_bytes, hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  const DevBatch O = host_outputs(s);
  if (sets) copy_sets(O, sst, pst);
  else copy_part(O, *q, pst, dst, agg);
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
  Collected k(c, t);
  if (k.rc != TBG_OK) return k.rc;
  Slot* s = k.s;
  const DevBatch L = checked_batch(s->last);  // (TBG_OP_AGGREGATE_VERIFY: the aggregates' checks)
  uint32_t cnt[CNT_WORDS];
  if (read_counters(s, L, cnt) != TBG_OK) return TBG_E_DEVICE;
  uint32_t ng = L.rlc_group ? (L.n_duties + L.rlc_group - 1) / L.rlc_group : 0;
  out4[0] = ng;
  out4[1] = cnt[CNT_DUTIES];
  out4[2] = cnt[CNT_PARTIALS];
  out4[3] = L.rlc_group;
  return TBG_OK;
}

int tbg_fetch_fallback(tbg_ctx* c, tbg_ticket t, uint32_t* out8) {
  if (!c || !out8) return TBG_E_INVALID_ARG;
  Collected k(c, t);
  if (k.rc != TBG_OK) return k.rc;
  Slot* s = k.s;
  const DevBatch L = checked_batch(s->last);  // (TBG_OP_AGGREGATE_VERIFY: the aggregates' checks)
  uint32_t cnt[CNT_WORDS];
  if (read_counters(s, L, cnt) != TBG_OK) return TBG_E_DEVICE;
  out8[0] = L.rlc_group ? (L.n_duties + L.rlc_group - 1) / L.rlc_group : 0;
  out8[1] = cnt[CNT_GID];
  out8[2] = cnt[CNT_CHUNKS];
  out8[3] = cnt[CNT_CID];
  out8[4] = cnt[CNT_DUTIES];
  out8[5] = cnt[CNT_PARTIALS];
  out8[6] = L.rlc_group;
  out8[7] = s->L.dims.op == TBG_OP_AGGREGATE || !L.rlc_batch ? (uint32_t)TBG_L0_NOT_RUN
            : cnt[CNT_L0_OK]                              ? (uint32_t)TBG_L0_PASSED
                                                          : (uint32_t)TBG_L0_FAILED;
  return TBG_OK;
}

int tbg_fetch_shape(tbg_ctx* c, tbg_ticket t, uint32_t* out4) {
  if (!c || !out4) return TBG_E_INVALID_ARG;
  Collected k(c, t);
  if (k.rc != TBG_OK) return k.rc;
  Slot* s = k.s;
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
  Collected k(c, t);
  if (k.rc != TBG_OK) return k.rc;
  Slot* s = k.s;
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
  Collected k(c, t);
  if (k.rc != TBG_OK) return k.rc;
  Slot* s = k.s;
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
  Collected k(c, t);
  if (k.rc != TBG_OK) return k.rc;
  Slot* s = k.s;
  *device_bytes = (uint64_t)s->d_in_cap + (uint64_t)s->d_work_cap;
  *pinned_bytes = (uint64_t)s->h_in_cap + (uint64_t)s->h_out_cap;
  return TBG_OK;
}

int tbg_fetch_level0_msgs(tbg_ctx* c, tbg_ticket t, uint32_t* out2) {
  if (!c || !out2) return TBG_E_INVALID_ARG;
  Collected k(c, t);
  if (k.rc != TBG_OK) return k.rc;
  Slot* s = k.s;
  // (the launch's own fields: launch_rlc_check took its path from the same ones)
  const DevBatch B = checked_batch(s->last);  // (TBG_OP_AGGREGATE_VERIFY: never by message)
  out2[0] = out2[1] = 0;
  if (s->L.dims.op == TBG_OP_AGGREGATE || !B.rlc_batch || !B.rlc_group || !B.n_duties) return TBG_OK;
  const bool by_msg = l0_by_msg(B);
  const uint32_t n = by_msg ? B.n_msgs : B.n_duties;
  out2[0] = by_msg ? 1u : 0u;
  out2[1] = ((n + B.rlc_group - 1) / B.rlc_group) * ((B.rlc_group + B.rlc_chunk - 1) / B.rlc_chunk);
  return TBG_OK;
}

int tbg_fetch_level0(tbg_ctx* c, tbg_ticket t, int32_t* state) {
  if (!c || !state) return TBG_E_INVALID_ARG;
  Collected k(c, t);
  if (k.rc != TBG_OK) return k.rc;
  Slot* s = k.s;
  *state = TBG_L0_NOT_RUN;
  const DevBatch L = checked_batch(s->last);  // (TBG_OP_AGGREGATE_VERIFY: the aggregates' checks)
  if (s->L.dims.op == TBG_OP_AGGREGATE || !L.rlc_batch) return TBG_OK;
  uint32_t cnt[CNT_WORDS];
  if (read_counters(s, L, cnt) != TBG_OK) return TBG_E_DEVICE;
  *state = cnt[CNT_L0_OK] ? TBG_L0_PASSED : TBG_L0_FAILED;
  return TBG_OK;
}

int tbg_last_timings(const tbg_ctx* c, float* ms8) {
  if (!c || !ms8) return TBG_E_INVALID_ARG;
  memcpy(ms8, c->last_ms, sizeof(c->last_ms));
  return TBG_OK;
}

}  // extern "C"

// ---- the calls that run to completion inside themselves ----------------------
// Each describes its workspace once (tbls_work.h), owns it through one scope
// and, once it has enqueued anything, leaves only through that scope.
namespace {

// The single device allocation of one such call.  Whatever way the call ends,
// the call's stream is drained first -- copies out of the call's own host
// vectors may still be queued -- and the memory freed after.
struct CallScope {
  hipStream_t st;
  uint8_t* d_base = nullptr;
  explicit CallScope(hipStream_t stream) : st(stream) {}
  CallScope(const CallScope&) = delete;
  ~CallScope() {
    (void)hipStreamSynchronize(st);
    if (d_base) (void)hipFree(d_base);
  }
  // Sizes w's workspace by one walk of its sections, allocates, binds w's pointers by a second.
  template <class W>
  int open(W& w) {
    const WorkWalk sized = work_size(w);
    if (hipMalloc(&d_base, sized.bytes()) != hipSuccess) {
      d_base = nullptr;
      return TBG_E_OOM;
    }
    work_bind(w, sized, d_base);
    return TBG_OK;
  }
  // The call's return code once its outputs have arrived: rc, or TBG_E_DEVICE if the stream failed.
  int drain(int rc) { return hipStreamSynchronize(st) != hipSuccess ? TBG_E_DEVICE : rc; }
};

// A signer's messages, their offsets and the items' message indices, into its workspace.
int upload_sign_inputs(const SignWork& w, const uint8_t* msgs, const uint32_t* msg_off, const uint32_t* item_msg,
                       hipStream_t st) {
  if ((w.msg_bytes && hipMemcpyAsync(w.msgs, msgs, w.msg_bytes, hipMemcpyHostToDevice, st) != hipSuccess) ||
      hipMemcpyAsync(w.msg_off, msg_off, 4ull * (w.n_msgs + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(w.item_msg, item_msg, 4ull * w.n, hipMemcpyHostToDevice, st) != hipSuccess)
    return TBG_E_DEVICE;
  return TBG_OK;
}

// H(m) of the call's messages into w.h_aff / w.h_status.
void hash_call_msgs(const SignWork& w, hipStream_t st) {
  DevBatch B{};
  memset(&B, 0, sizeof(B));
  B.n_msgs = (uint32_t)w.n_msgs;
  B.msgs = w.msgs;
  B.msg_off = w.msg_off;
  B.h_aff = w.h_aff;
  B.h_status = w.h_status;
  B.h_jac = w.h_jac;
  launch_hash_msgs(B, st);
}

}  // namespace

extern "C" {

int tbg_sk_to_pk(tbg_ctx* c, const uint8_t* sk32, uint32_t n, uint8_t* pk48) {
  if (!c || (n && (!sk32 || !pk48))) return TBG_E_INVALID_ARG;
  if (n == 0) return TBG_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  SkToPkWork w;
  w.n = n;
  CallScope cs(c->stream);
  int rc = cs.open(w);
  if (rc != TBG_OK) return rc;
  hipStream_t st = c->stream;
  if (hipMemcpyAsync(w.sk, sk32, 32ull * n, hipMemcpyHostToDevice, st) != hipSuccess) rc = TBG_E_DEVICE;
  if (rc == TBG_OK) {
    launch_sk_to_pk(w.sk, n, w.pk, st);
    if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  }
  if (rc == TBG_OK && hipMemcpyAsync(pk48, w.pk, 48ull * n, hipMemcpyDeviceToHost, st) != hipSuccess) rc = TBG_E_DEVICE;
  return cs.drain(rc);
}

int tbg_sign(tbg_ctx* c, const uint8_t* sk32, uint32_t n, const uint8_t* msgs, const uint32_t* msg_off, uint32_t n_msgs,
             const uint32_t* item_msg, uint8_t* sig96) {
  if (!c || (n && (!sk32 || !sig96 || !item_msg)) || n_msgs == 0 || !offsets_ok(msg_off, n_msgs)) return TBG_E_INVALID_ARG;
  for (uint32_t i = 0; i < n; ++i)
    if (item_msg[i] >= n_msgs) return TBG_E_INVALID_ARG;
  if (n == 0) return TBG_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  SignWork w;
  w.n = n;
  w.n_msgs = n_msgs;
  w.msg_bytes = msg_off[n_msgs];
  CallScope cs(c->stream);
  int rc = cs.open(w);
  if (rc != TBG_OK) return rc;
  hipStream_t st = c->stream;
  if (hipMemcpyAsync(w.sk, sk32, 32ull * n, hipMemcpyHostToDevice, st) != hipSuccess) rc = TBG_E_DEVICE;
  if (rc == TBG_OK) rc = upload_sign_inputs(w, msgs, msg_off, item_msg, st);
  if (rc == TBG_OK) {
    hash_call_msgs(w, st);
    launch_sign(w.sk, w.item_msg, n, w.h_aff, w.h_status, w.sig, st);
    if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  }
  if (rc == TBG_OK && hipMemcpyAsync(sig96, w.sig, 96ull * n, hipMemcpyDeviceToHost, st) != hipSuccess) rc = TBG_E_DEVICE;
  return cs.drain(rc);
}

}  // extern "C"

// ---- the hardened signer (k_keyed.hip, bls_ctmul.h) ------------------------
namespace {

// TBG_KS_* of a 32-byte big-endian key: zero, or a word-wise compare against
// r -- every word is read and subtracted whatever the earlier ones were.
// (zero_code / range_code: the caller's codes for the two refusals)
int32_t range_status(const uint8_t* b, int32_t zero_code, int32_t range_code) {
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
  return (zero_code & zero) | (range_code & ge & ~zero);
}
int32_t keyed_status(const uint8_t* b) { return range_status(b, TBG_KS_ZERO, TBG_KS_RANGE); }

// all ones iff v != 0
inline int32_t nz_mask(int32_t v) { return 0 - (int32_t)(((uint32_t)v | (0u - (uint32_t)v)) >> 31); }

void keyed_wipe(void* p, size_t n) {
  volatile uint8_t* v = (volatile uint8_t*)p;
  for (size_t i = 0; i < n; ++i) v[i] = 0;
}

// 32 bytes into the staging: k itself (keep = 0xff) or the scalar 1 (keep = 0), by masks
inline void stage_scalar(uint8_t* dst, const uint8_t* k, uint8_t keep) {
  for (int j = 0; j < 32; ++j) dst[j] = (uint8_t)((k[j] & keep) | ((j == 31 ? 1 : 0) & ~keep));
}

// The scope of a call that holds secrets: CallScope and everything that held
// secret bytes -- the device sections the call's workspace names in secrets()
// and every pinned staging buffer the call took from stage().  Whatever way
// the call ends, the device bytes are zeroed ON THE STREAM (behind the kernels
// and copies that use them), the stream is drained, the staging is zeroed, and
// only then is either released (the workspace by ~CallScope, which runs after
// this destructor).
struct KeyedScope : CallScope {
  struct Region {
    uint8_t* p;
    size_t bytes;
  };
  static constexpr uint32_t kMaxRegions = 8;
  Region dev[kMaxRegions] = {};   // inside the workspace
  Region pin[kMaxRegions] = {};   // pinned (hipHostMalloc)
  uint32_t n_dev = 0, n_pin = 0;
  using CallScope::CallScope;
  ~KeyedScope() {
    for (uint32_t i = 0; i < n_dev; ++i)
      if (dev[i].bytes) (void)hipMemsetAsync(dev[i].p, 0, dev[i].bytes, st);
    (void)hipStreamSynchronize(st);
    for (uint32_t i = 0; i < n_pin; ++i) {
      keyed_wipe(pin[i].p, pin[i].bytes);
      (void)hipHostFree(pin[i].p);
    }
  }
  // w's workspace; the sections w.secrets() names become the scope's to wipe
  template <class W>
  int open(W& w) {
    const int rc = CallScope::open(w);
    if (rc != TBG_OK) return rc;
    auto take = [&](const char*, uint8_t*& p, size_t count, size_t = 0) {
      plan_check(n_dev < kMaxRegions, "more secret sections than KeyedScope::kMaxRegions");
      dev[n_dev++] = Region{p, count};
    };
    w.secrets(take);
    return TBG_OK;
  }
  // a pinned staging buffer of the scope (zero-filled); null when the host cannot pin it
  uint8_t* stage(size_t bytes) {
    uint8_t* h = nullptr;
    if (n_pin >= kMaxRegions || hipHostMalloc((void**)&h, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    pin[n_pin++] = Region{h, bytes};
    memset(h, 0, bytes);
    return h;
  }
  // the hardened signer's: w's workspace and the keys' staging; the keys go into the staging
  // with every rejected one replaced by 1 (masks, no branch on a key byte), their codes into kst.
  template <class W>
  int open(W& w, const uint8_t* sk32, uint32_t n, std::vector<int32_t>& kst) {
    const int rc = open(w);
    if (rc != TBG_OK) return rc;
    uint8_t* h_sk = stage(32ull * n);
    if (!h_sk) return TBG_E_OOM;
    kst.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
      const uint8_t* k = sk32 + 32ull * i;
      kst[i] = keyed_status(k);
      stage_scalar(h_sk + 32ull * i, k, (uint8_t)~nz_mask(kst[i]));  // 0xff: accepted
    }
    return hipMemcpyAsync(w.sk, h_sk, 32ull * n, hipMemcpyHostToDevice, st) == hipSuccess ? TBG_OK : TBG_E_DEVICE;
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
  SkToPkCtWork w;
  w.n = n;
  w.tab_words = ct_tab_words_g1();
  std::vector<int32_t> kst;
  KeyedScope ks(c->stream);
  int rc = ks.open(w, sk32, n, kst);
  if (rc != TBG_OK) return rc;
  hipStream_t st = c->stream;
  launch_ct_table_g1(w.tab, st);
  launch_sk_to_pk_ct(w.sk, n, w.tab, w.pk, w.status, st);
  if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  if (rc == TBG_OK && (hipMemcpyAsync(pk48, w.pk, 48ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
                       hipMemcpyAsync(status, w.status, 4ull * n, hipMemcpyDeviceToHost, st) != hipSuccess))
    rc = TBG_E_DEVICE;
  rc = ks.drain(rc);
  if (rc == TBG_OK) keyed_mask(kst, pk48, 48, status);
  return rc;
}

int tbg_sign_ct(tbg_ctx* c, const uint8_t* sk32, uint32_t n, const uint8_t* msgs, const uint32_t* msg_off, uint32_t n_msgs,
                const uint32_t* item_msg, uint8_t* sig96, int32_t* status) {
  if (!c || (n && (!sk32 || !sig96 || !item_msg || !status)) || n_msgs == 0 || !offsets_ok(msg_off, n_msgs))
    return TBG_E_INVALID_ARG;
  for (uint32_t i = 0; i < n; ++i)
    if (item_msg[i] >= n_msgs) return TBG_E_INVALID_ARG;
  if (n == 0) return TBG_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  SignCtWork w;
  w.n = n;
  w.n_msgs = n_msgs;
  w.msg_bytes = msg_off[n_msgs];
  w.tab_words = ct_tab_words_g2(n_msgs);
  std::vector<int32_t> kst;
  KeyedScope ks(c->stream);
  int rc = ks.open(w, sk32, n, kst);
  if (rc != TBG_OK) return rc;
  hipStream_t st = c->stream;
  rc = upload_sign_inputs(w, msgs, msg_off, item_msg, st);
  if (rc == TBG_OK) {
    hash_call_msgs(w, st);
    launch_ct_table_g2(w.h_aff, w.h_status, n_msgs, w.tab, st);
    launch_sign_ct(w.sk, w.item_msg, n, n_msgs, w.tab, w.h_status, w.sig, w.status, st);
    if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  }
  if (rc == TBG_OK && (hipMemcpyAsync(sig96, w.sig, 96ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
                       hipMemcpyAsync(status, w.status, 4ull * n, hipMemcpyDeviceToHost, st) != hipSuccess))
    rc = TBG_E_DEVICE;
  rc = ks.drain(rc);
  if (rc == TBG_OK) keyed_mask(kst, sig96, 96, status);
  return rc;
}

// ---- shares on a fixed schedule (k_shares.hip, bls_frct.h) -----------------
// tbls/tss.go:256-290 (SplitSecret), :120-139 (GenerateTSS), :220-253
// (CombineShares).  The secret arithmetic in Fr runs on the device; the
// commitments and pubshares are the hardened signer's ladder over the
// coefficient section and the ladder-scalar section.  Secret outputs come back
// through the scope's pinned staging, never straight into caller memory.
int tbg_split_secret_ct(tbg_ctx* c, const uint8_t* coef32, const uint32_t* poly_first, uint32_t n_polys,
                        uint32_t n_shares, uint8_t* share32, uint8_t* commit48, uint8_t* pubshare48, int32_t* status) {
  if (!c || n_shares < 1 || n_shares > 255) return TBG_E_INVALID_ARG;
  if (n_polys == 0) return TBG_OK;
  if (!coef32 || !poly_first || !share32 || !commit48 || !status || poly_first[0] != 0) return TBG_E_INVALID_ARG;
  if ((uint64_t)n_polys * n_shares > 0x7fffffffull) return TBG_E_INVALID_ARG;
  for (uint32_t p = 0; p < n_polys; ++p) {
    if (poly_first[p + 1] < poly_first[p]) return TBG_E_INVALID_ARG;
    const uint32_t t = poly_first[p + 1] - poly_first[p];
    if (t < 2 || t > n_shares) return TBG_E_INVALID_ARG;  // (NewFeldman: 2 <= t <= n)
  }
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t nc = poly_first[n_polys], ne = n_polys * n_shares;
  SplitSecretCtWork w;
  w.n_coefs = nc;
  w.n_polys = n_polys;
  w.n_evals = ne;
  w.tab_words = ct_tab_words_g1();
  std::vector<int32_t> pst(n_polys);
  std::vector<uint32_t> zf(ne);
  KeyedScope ks(c->stream);
  int rc = ks.open(w);
  if (rc != TBG_OK) return rc;
  uint8_t* h_coef = ks.stage(32ull * nc);
  uint8_t* h_share = ks.stage(32ull * ne);
  if (!h_coef || !h_share) return TBG_E_OOM;
  // every coefficient's code is formed; the first one by index is the polynomial's, and a
  // refused polynomial goes up as all ones (masks, no branch on a coefficient byte)
  for (uint32_t p = 0; p < n_polys; ++p) {
    int32_t code = 0;
    for (uint32_t j = poly_first[p]; j < poly_first[p + 1]; ++j)
      code |= range_status(coef32 + 32ull * j, TBG_SH_COEF_ZERO, TBG_SH_COEF_RANGE) & ~nz_mask(code);
    pst[p] = code;
    for (uint32_t j = poly_first[p]; j < poly_first[p + 1]; ++j)
      stage_scalar(h_coef + 32ull * j, coef32 + 32ull * j, (uint8_t)~nz_mask(code));
  }
  hipStream_t st = c->stream;
  if (hipMemcpyAsync(w.coef, h_coef, 32ull * nc, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(w.poly_first, poly_first, 4ull * (n_polys + 1), hipMemcpyHostToDevice, st) != hipSuccess)
    rc = TBG_E_DEVICE;
  if (rc == TBG_OK) {
    launch_split_ct(w.coef, nc, w.poly_first, n_polys, n_shares, w.share, w.ladder, w.share_zero, st);
    launch_ct_table_g1(w.tab, st);
    launch_sk_to_pk_ct(w.coef, nc, w.tab, w.commit, w.ks_status, st);
    if (pubshare48) launch_sk_to_pk_ct(w.ladder, ne, w.tab, w.pubshare, w.ks_status, st);
    if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  }
  if (rc == TBG_OK &&
      (hipMemcpyAsync(h_share, w.share, 32ull * ne, hipMemcpyDeviceToHost, st) != hipSuccess ||
       hipMemcpyAsync(zf.data(), w.share_zero, 4ull * ne, hipMemcpyDeviceToHost, st) != hipSuccess ||
       hipMemcpyAsync(commit48, w.commit, 48ull * nc, hipMemcpyDeviceToHost, st) != hipSuccess ||
       (pubshare48 && hipMemcpyAsync(pubshare48, w.pubshare, 48ull * ne, hipMemcpyDeviceToHost, st) != hipSuccess)))
    rc = TBG_E_DEVICE;
  rc = ks.drain(rc);
  if (rc != TBG_OK) return rc;
  for (uint32_t p = 0; p < n_polys; ++p) {
    const size_t e0 = (size_t)p * n_shares, c0 = poly_first[p], t = poly_first[p + 1] - poly_first[p];
    uint32_t any_zero = 0;
    for (uint32_t i = 0; i < n_shares; ++i) any_zero |= zf[e0 + i];
    const int32_t code = pst[p] != TBG_SH_OK ? pst[p] : any_zero ? TBG_SH_SHARE_ZERO : TBG_SH_OK;  // (the code is public)
    status[p] = code;
    if (code == TBG_SH_OK) {
      memcpy(share32 + 32 * e0, h_share + 32 * e0, 32ull * n_shares);
    } else {
      memset(share32 + 32 * e0, 0, 32ull * n_shares);
      memset(commit48 + 48 * c0, 0, 48 * t);
      if (pubshare48) memset(pubshare48 + 48 * e0, 0, 48ull * n_shares);
    }
  }
  return TBG_OK;
}

int tbg_combine_shares_ct(tbg_ctx* c, const uint8_t* share32, const uint8_t* share_id, const uint32_t* set_first,
                          uint32_t n_sets, uint8_t* secret32, int32_t* status) {
  if (!c) return TBG_E_INVALID_ARG;
  if (n_sets == 0) return TBG_OK;
  if (!set_first || !secret32 || !status || set_first[0] != 0) return TBG_E_INVALID_ARG;
  for (uint32_t k = 0; k < n_sets; ++k)
    if (set_first[k + 1] < set_first[k]) return TBG_E_INVALID_ARG;
  const uint32_t nv = set_first[n_sets];
  if (nv && (!share32 || !share_id)) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  CombineSharesCtWork w;
  w.n_values = nv;
  w.n_sets = n_sets;
  std::vector<int32_t> sst(n_sets);
  std::vector<uint32_t> ok(n_sets), zf(n_sets);
  KeyedScope ks(c->stream);
  int rc = ks.open(w);
  if (rc != TBG_OK) return rc;
  uint8_t* h_value = ks.stage(32ull * nv);
  uint8_t* h_secret = ks.stage(32ull * n_sets);
  if (!h_value || !h_secret) return TBG_E_OOM;
  for (uint32_t k = 0; k < n_sets; ++k) {
    const uint32_t first = set_first[k], last = set_first[k + 1];
    // the public reasons (sizes and identifiers are public), in their precedence
    int32_t code = TBG_SH_OK;
    bool seen[256] = {}, id_zero = false, dup = false;
    for (uint32_t i = first; i < last; ++i) {
      id_zero |= share_id[i] == 0;
      dup |= seen[share_id[i]];
      seen[share_id[i]] = true;
    }
    if (last - first < 2) code = TBG_SH_TOO_FEW;
    else if (id_zero) code = TBG_SH_ID;
    else if (dup) code = TBG_SH_DUPLICATE_ID;
    // then the values: every one's code is formed, the first by index counts (masks)
    int32_t vcode = 0;
    for (uint32_t i = first; i < last; ++i)
      vcode |= range_status(share32 + 32ull * i, TBG_SH_VALUE_ZERO, TBG_SH_VALUE_RANGE) & ~nz_mask(vcode);
    code |= vcode & ~nz_mask(code);
    sst[k] = code;
    ok[k] = (uint32_t)~nz_mask(code) & 1u;
    for (uint32_t i = first; i < last; ++i)
      stage_scalar(h_value + 32ull * i, share32 + 32ull * i, (uint8_t)~nz_mask(code));
  }
  hipStream_t st = c->stream;
  if ((nv && (hipMemcpyAsync(w.value, h_value, 32ull * nv, hipMemcpyHostToDevice, st) != hipSuccess ||
              hipMemcpyAsync(w.share_id, share_id, nv, hipMemcpyHostToDevice, st) != hipSuccess)) ||
      hipMemcpyAsync(w.set_first, set_first, 4ull * (n_sets + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(w.set_ok, ok.data(), 4ull * n_sets, hipMemcpyHostToDevice, st) != hipSuccess)
    rc = TBG_E_DEVICE;
  if (rc == TBG_OK) {
    launch_combine_ct(w.value, w.share_id, nv, w.set_first, w.set_ok, n_sets, w.secret, w.secret_zero, st);
    if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  }
  if (rc == TBG_OK && (hipMemcpyAsync(h_secret, w.secret, 32ull * n_sets, hipMemcpyDeviceToHost, st) != hipSuccess ||
                       hipMemcpyAsync(zf.data(), w.secret_zero, 4ull * n_sets, hipMemcpyDeviceToHost, st) != hipSuccess))
    rc = TBG_E_DEVICE;
  rc = ks.drain(rc);
  if (rc != TBG_OK) return rc;
  for (uint32_t k = 0; k < n_sets; ++k) {
    const int32_t code = sst[k] != TBG_SH_OK ? sst[k] : zf[k] ? TBG_SH_SECRET_ZERO : TBG_SH_OK;  // (public)
    status[k] = code;
    if (code == TBG_SH_OK) memcpy(secret32 + 32ull * k, h_secret + 32ull * k, 32);
    else memset(secret32 + 32ull * k, 0, 32);
  }
  return TBG_OK;
}

// ---- plain sums and FastAggregateVerify (k_sum.hip) -----------------------
// dkg/dkg.go:466-476 (AggregateSignatures / AggregatePublicKeys of the lock
// hash), cluster/lock.go:155-177 (FastAggregateVerify over every pubshare).

}  // extern "C"

namespace {

// Host half of a sum plan; its device half is the head of the call's workspace (SumWork).
struct SumHost {
  std::vector<uint32_t> chunk_first, chunk_set;
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
  // the counts of the plan's device half, part_elem bytes per chunk sum (before the workspace is opened)
  void describe(SumWork& w, uint32_t n_sets, size_t part_elem) const {
    w.n_sets = n_sets;
    w.n_chunks = n_chunks();
    w.part_elem = part_elem;
  }
  int upload(const SumWork& w, const uint32_t* off, hipStream_t st, tbg::SumPlan& p) const {
    const uint32_t n_sets = (uint32_t)w.n_sets;
    p.n_sets = n_sets;
    p.n_chunks = n_chunks();
    p.off = w.off;
    p.chunk_first = w.chunk_first;
    p.chunk_set = w.chunk_set;
    p.part = w.part;
    p.set_bad = w.set_bad;
    if (hipMemcpyAsync(w.off, off, 4ull * (n_sets + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(w.chunk_first, chunk_first.data(), 4ull * (n_sets + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
        (n_chunks() &&
         hipMemcpyAsync(w.chunk_set, chunk_set.data(), 4ull * n_chunks(), hipMemcpyHostToDevice, st) != hipSuccess) ||
        hipMemsetAsync(w.set_bad, 0, 4ull * n_sets, st) != hipSuccess)
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
  const SumHost h(off, n_sets);  // (outlives the scope: its vectors are copied from on the stream)
  SumPubkeysWork w;
  h.describe(w, n_sets, sizeof(G1J));
  w.n_items = ni;
  CallScope cs(c->stream);
  int rc = cs.open(w);
  if (rc != TBG_OK) return rc;
  hipStream_t st = c->stream;
  tbg::SumPlan p;
  rc = h.upload(w, off, st, p);
  if (rc == TBG_OK && ni && hipMemcpyAsync(w.ids, pubkey_ids, 4ull * ni, hipMemcpyHostToDevice, st) != hipSuccess)
    rc = TBG_E_DEVICE;
  if (rc == TBG_OK) {
    tbg::launch_sum_g1(c->d_pk, c->d_pk_status, c->n_pk, w.ids, p, w.out, w.status, st);
    if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  }
  if (rc == TBG_OK && (hipMemcpyAsync(out48, w.out, 48ull * n_sets, hipMemcpyDeviceToHost, st) != hipSuccess ||
                       hipMemcpyAsync(status, w.status, 4ull * n_sets, hipMemcpyDeviceToHost, st) != hipSuccess))
    rc = TBG_E_DEVICE;
  return cs.drain(rc);
}

int tbg_sum_sigs(tbg_ctx* c, const uint8_t* sigs96, const uint32_t* off, uint32_t n_sets, uint8_t* out96,
                 int32_t* status, int32_t* sig_status) {
  if (!c || !n_sets || !out96 || !status || !offsets_ok(off, n_sets)) return TBG_E_INVALID_ARG;
  const uint32_t ni = off[n_sets];
  if (ni && !sigs96) return TBG_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const SumHost h(off, n_sets);  // (outlives the scope: its vectors are copied from on the stream)
  SumSigsWork w;
  h.describe(w, n_sets, sizeof(G2J));
  w.n_items = ni;
  CallScope cs(c->stream);
  int rc = cs.open(w);
  if (rc != TBG_OK) return rc;
  hipStream_t st = c->stream;
  tbg::SumPlan p;
  rc = h.upload(w, off, st, p);
  if (rc == TBG_OK && ni && hipMemcpyAsync(w.sigs, sigs96, 96ull * ni, hipMemcpyHostToDevice, st) != hipSuccess)
    rc = TBG_E_DEVICE;
  if (rc == TBG_OK) {
    tbg::launch_sum_g2(w.sigs, p, w.out, w.status, w.sig_status, st);
    if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  }
  if (rc == TBG_OK &&
      (hipMemcpyAsync(out96, w.out, 96ull * n_sets, hipMemcpyDeviceToHost, st) != hipSuccess ||
       hipMemcpyAsync(status, w.status, 4ull * n_sets, hipMemcpyDeviceToHost, st) != hipSuccess ||
       (sig_status && ni && hipMemcpyAsync(sig_status, w.sig_status, 4ull * ni, hipMemcpyDeviceToHost, st) != hipSuccess)))
    rc = TBG_E_DEVICE;
  return cs.drain(rc);
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
  // (both outlive the scope: they are copied from on the stream)
  const SumHost h(key_off, n);
  std::vector<uint32_t> iota(n + 1);
  for (uint32_t i = 0; i <= n; ++i) iota[i] = i;
  FastAggVerifyWork w;
  h.describe(w, n, sizeof(G1J));
  w.n_keys = nk;
  w.msg_bytes = mb;
  CallScope cs(c->stream);
  int rc = cs.open(w);
  if (rc != TBG_OK) return rc;
  hipStream_t st = c->stream;
  // 1. the key sums, compressed, then decoded into a table of their own
  tbg::SumPlan p;
  rc = h.upload(w, key_off, st, p);
  if (rc == TBG_OK && nk && hipMemcpyAsync(w.ids, pubkey_ids, 4ull * nk, hipMemcpyHostToDevice, st) != hipSuccess)
    rc = TBG_E_DEVICE;
  if (rc == TBG_OK) {
    tbg::launch_sum_g1(c->d_pk, c->d_pk_status, c->n_pk, w.ids, p, w.pk48, w.key_status, st);
    tbg::launch_decode_pubkeys(w.pk48, n, w.t_pk, w.t_xpk, w.t_pk_status, st);  // a failed / identity sum: not DEC_OK
  }
  // 2. one CoreVerify per set against that table (the per-item schedule)
  DevBatch B{};
  memset(&B, 0, sizeof(B));
  B.op = TBG_OP_VERIFY;
  B.n_duties = B.n_partials = B.n_msgs = n;
  B.msgs = w.msgs;
  B.msg_off = w.msg_off;
  B.duty_msg = B.duty_first = B.partial_duty = B.pubkey_ids = w.iota;
  B.duty_threshold = w.iota;  // unused by TBG_OP_VERIFY
  B.sigs = w.sigs;
  B.identifiers = w.identifiers;
  B.sig_aff = w.sig_aff;
  B.h_aff = w.h_aff;
  B.h_status = w.h_status;
  B.h_jac = w.h_jac;
  B.sig_lines = w.sig_lines;
  B.h_lines = w.h_lines;
  B.counters = w.counters;
  B.part_list = w.part_list;
  B.partial_status = w.partial_status;
  B.duty_status = w.duty_status;
  B.rlc_group = 0;
  B.fb_full = 0xFFFFFFFFu;
  if (rc == TBG_OK && ((mb && hipMemcpyAsync(w.msgs, msgs, mb, hipMemcpyHostToDevice, st) != hipSuccess) ||
                       hipMemcpyAsync(w.msg_off, msg_off, 4ull * (n + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
                       hipMemcpyAsync(w.iota, iota.data(), 4ull * (n + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
                       hipMemcpyAsync(w.sigs, sigs96, 96ull * n, hipMemcpyHostToDevice, st) != hipSuccess ||
                       hipMemsetAsync(w.identifiers, 0, n, st) != hipSuccess ||
                       hipMemsetAsync(w.counters, 0, 4 * tbg::CNT_WORDS, st) != hipSuccess))
    rc = TBG_E_DEVICE;
  if (rc == TBG_OK) {
    tbg::launch_decode_sigs(B, st);
    tbg::launch_hash_msgs(B, st);
    tbg::launch_h_lines(B, st);
    tbg::launch_rlc_prepare(B, w.t_pk, nullptr, w.t_pk_status, n, st);
    tbg::launch_rlc_check(B, w.t_pk, nullptr, w.t_pk_status, n, st);  // (per-item schedule: no key table)
    if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  }
  if (rc == TBG_OK && hipMemcpyAsync(status, w.partial_status, 4ull * n, hipMemcpyDeviceToHost, st) != hipSuccess)
    rc = TBG_E_DEVICE;
  return cs.drain(rc);
}

// ---- Feldman commitment polynomials (k_feldman.hip, bls_feldman.h) ---------
// tbls/tss.go:95-116 (NewTSS), :293-325 (getPubShare): the pubshares from the
// verifier alone; at one identifier, the public side of Feldman share verification.
int tbg_eval_commitments(tbg_ctx* c, const uint8_t* commit48, const uint32_t* poly_first, uint32_t n_polys,
                         const uint32_t* eval_poly, const uint32_t* eval_id, uint32_t n_evals, uint8_t* out48,
                         int32_t* eval_status, int32_t* commit_status) {
  if (!c) return TBG_E_INVALID_ARG;
  if (n_polys) {
    if (!commit48 || !poly_first || poly_first[0] != 0) return TBG_E_INVALID_ARG;
    for (uint32_t p = 0; p < n_polys; ++p)
      if (poly_first[p + 1] <= poly_first[p]) return TBG_E_INVALID_ARG;  // decreasing, or an empty polynomial
  }
  if (n_evals) {
    if (!eval_poly || !eval_id || !out48 || !eval_status) return TBG_E_INVALID_ARG;
    for (uint32_t e = 0; e < n_evals; ++e)
      if (eval_poly[e] >= n_polys) return TBG_E_INVALID_ARG;
  }
  if (n_polys == 0 || n_evals == 0) return TBG_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t nc = poly_first[n_polys];
  EvalCommitWork w;
  w.n_commits = nc;
  w.n_polys = n_polys;
  w.n_evals = n_evals;
  CallScope cs(c->stream);
  int rc = cs.open(w);
  if (rc != TBG_OK) return rc;
  hipStream_t st = c->stream;
  if (hipMemcpyAsync(w.commit48, commit48, 48ull * nc, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(w.poly_first, poly_first, 4ull * (n_polys + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(w.eval_poly, eval_poly, 4ull * n_evals, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(w.eval_id, eval_id, 4ull * n_evals, hipMemcpyHostToDevice, st) != hipSuccess)
    rc = TBG_E_DEVICE;
  if (rc == TBG_OK) {
    tbg::launch_decode_pubkeys(w.commit48, nc, w.t_c, w.t_xc, w.commit_status, st);
    tbg::launch_fv_eval(w.t_c, w.commit_status, nc, w.poly_first, n_polys, w.eval_poly, w.eval_id, n_evals, w.out48,
                        w.eval_status, st);
    if (hipGetLastError() != hipSuccess) rc = TBG_E_DEVICE;
  }
  if (rc == TBG_OK &&
      (hipMemcpyAsync(out48, w.out48, 48ull * n_evals, hipMemcpyDeviceToHost, st) != hipSuccess ||
       hipMemcpyAsync(eval_status, w.eval_status, 4ull * n_evals, hipMemcpyDeviceToHost, st) != hipSuccess ||
       (commit_status && hipMemcpyAsync(commit_status, w.commit_status, 4ull * nc, hipMemcpyDeviceToHost, st) != hipSuccess)))
    rc = TBG_E_DEVICE;
  return cs.drain(rc);
}

}  // extern "C"
