#include "tbls_launch.h"
#include "bls_ctmul.h"

namespace tbg {

// ---- the hardened signer (tbg_sk_to_pk_ct / tbg_sign_ct, include/tbls_gpu.h):
// tbls.Sign / PartialSign and SecretKey.GetPublicKey for keys that matter
// (reference cmd/createcluster.go:185-207, :487-515; dkg/dkg.go:480-542). ----
// One lane per key.  [sk]G1 and [sk]H(m) on the fixed schedule of
// bls_ctmul.h: no branch, loop bound or address below depends on sk.  What
// does vary from lane to lane is public: the lane's index, its message index
// and whether that message's H(m) could be formed.  The host has replaced
// every key outside (0, r) by 1 (tbls_engine.hip), so no product is the
// identity and the compressed encodings never take their infinity form.
namespace {

TBG_HD void ct_words_from_be32(const uint8_t* b, uint32_t (&w)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
    w[i] = ((uint32_t)b[31 - 4 * i]) | ((uint32_t)b[30 - 4 * i] << 8) | ((uint32_t)b[29 - 4 * i] << 16) |
           ((uint32_t)b[28 - 4 * i] << 24);
}

// the multiples 0..8 of the G1 generator: one table, one lane
__global__ void __launch_bounds__(64) k_ct_table_g1(uint32_t* tab) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const G1A g = {fp_from_const(G1_X), fp_from_const(G1_Y)};
  ct_build_table(g, [&](int e, const CtPoint<Fp>& p) { ct_tab_store(tab, 1, e, p); });
}

// the multiples 0..8 of every H(m): one lane per message.  A message whose
// H(m) failed gets a table of well-formed field elements; k_sign_ct zeroes
// the outputs of its items.
__global__ void __launch_bounds__(64) k_ct_table_g2(const G2A* h_aff, const int32_t* h_status, uint32_t n_msgs,
                                                     uint32_t* tab) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n_msgs) return;
  G2A h = {fp2_zero(), fp2_one()};
  if (h_status[m] == 0) h = h_aff[m];
  ct_build_table(h, [&](int e, const CtPoint<Fp2>& p) { ct_tab_store(tab + m, n_msgs, e, p); });
}

__global__ void __launch_bounds__(64) k_sk_to_pk_ct(const uint8_t* sk32, uint32_t n, const uint32_t* tab, uint8_t* pk48,
                                                     int32_t* status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  ct_words_from_be32(sk32 + 32ull * i, w);
  const CtTabMem<Fp> T = {tab, 1};
  const G1A a = ct_to_aff(ct_mul<Fp>(T, w));
  uint8_t enc[48];
  g1_compress(a, false, enc);
  for (int j = 0; j < 48; ++j) pk48[48ull * i + j] = enc[j];
  status[i] = TBG_KS_OK;
}

__global__ void __launch_bounds__(64) k_sign_ct(const uint8_t* sk32, const uint32_t* item_msg, uint32_t n, uint32_t n_msgs,
                                                 const uint32_t* tab, const int32_t* h_status, uint8_t* sig96,
                                                 int32_t* status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  ct_words_from_be32(sk32 + 32ull * i, w);
  const uint32_t m = item_msg[i];
  const CtTabMem<Fp2> T = {tab + m, n_msgs};
  const G2A a = ct_to_aff(ct_mul<Fp2>(T, w));
  uint8_t enc[96];
  g2_compress(a, false, enc);
  const bool msg_ok = h_status[m] == 0;  // (public)
  for (int j = 0; j < 96; ++j) sig96[96ull * i + j] = msg_ok ? enc[j] : (uint8_t)0;
  status[i] = msg_ok ? TBG_KS_OK : TBG_KS_MSG;
}

}  // namespace

size_t ct_tab_words_g1() { return ct_tab_words_per<Fp>(); }
size_t ct_tab_words_g2(uint32_t n_msgs) { return (size_t)ct_tab_words_per<Fp2>() * n_msgs; }

void launch_ct_table_g1(uint32_t* tab, hipStream_t st) { TBG_KLAUNCH(k_ct_table_g1, dim3(1), dim3(kBlock), st, tab); }
void launch_ct_table_g2(const G2A* h_aff, const int32_t* h_status, uint32_t n_msgs, uint32_t* tab, hipStream_t st) {
  if (n_msgs) TBG_KLAUNCH(k_ct_table_g2, grid_for(n_msgs), dim3(kBlock), st, h_aff, h_status, n_msgs, tab);
}
void launch_sk_to_pk_ct(const uint8_t* sk32, uint32_t n, const uint32_t* tab, uint8_t* pk48, int32_t* status,
                        hipStream_t st) {
  if (n) TBG_KLAUNCH(k_sk_to_pk_ct, grid_for(n), dim3(kBlock), st, sk32, n, tab, pk48, status);
}
void launch_sign_ct(const uint8_t* sk32, const uint32_t* item_msg, uint32_t n, uint32_t n_msgs, const uint32_t* tab,
                    const int32_t* h_status, uint8_t* sig96, int32_t* status, hipStream_t st) {
  if (n) TBG_KLAUNCH(k_sign_ct, grid_for(n), dim3(kBlock), st, sk32, item_msg, n, n_msgs, tab, h_status, sig96, status);
}

}  // namespace tbg
