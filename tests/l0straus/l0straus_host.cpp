// TEST TOOLING ONLY: host (CPU) twin of the fused level 0's per-duty key side
// (charon_amd/csrc/bls_rlc.h rlc_duty_keys_l0f, run by k_rlc_g1_l0 one lane
// per duty) for tests/test_l0_straus_host.py, with the value bound checks
// (TBG_BOUNDS_CHECK) switched on.  Modelled on tests/sgbpair.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../charon_amd/csrc/bls_pairing.h"
#include "../../charon_amd/csrc/bls_h2c.h"
#include "../../charon_amd/csrc/bls_rlc.h"
#include "../../charon_amd/csrc/bls_pair.h"

extern "C" unsigned long long tbg_mad_count = 0;

using namespace tbg;

namespace {

constexpr int MAX_N = 64;

struct Keys {
  std::vector<G1A> tab;  // PK_TAB_W2 entries per key, built entry by entry as k_pubkey_tables does
  bool load(const uint8_t* pk48, int n_keys) {
    tab.resize((size_t)PK_TAB_W2 * n_keys);
    for (int j = 0; j < n_keys; ++j) {
      G1A pk, xpk;
      if (g1_decompress(pk48 + 48 * j, pk) != DEC_OK) return false;
      if (!jac_to_aff(jac_neg(jac_mul_xabs(jac_from_aff(pk))), xpk)) return false;
      for (int k = 0; k < (int)PK_TAB_W2; ++k)
        if (!jac_to_aff(rlc_key_table_w2_entry(pk, xpk, k), tab[(size_t)PK_TAB_W2 * j + k])) return false;
    }
    return true;
  }
};

int put(const G1J& p, uint8_t* out48) {
  G1A a{fp_zero(), fp_zero()};
  const bool fin = jac_to_aff(p, a);
  g1_compress(a, !fin, out48);
  return fin ? 0 : 1;
}

}  // namespace

extern "C" {

// fused digits u_j of n digit vectors c (18 each): l0f_digits
void ls_digits(const int32_t* c18, uint32_t n, uint32_t* u4) {
  for (uint32_t i = 0; i < n; ++i) {
    int32_t c[18];
    uint32_t u[4];
    for (int k = 0; k < 18; ++k) c[k] = c18[18ull * i + k];
    l0f_digits(c, u);
    for (int j = 0; j < 4; ++j) u4[4ull * i + j] = u[j];
  }
}

// P_d of a duty of n partials by rlc_duty_keys_l0f, as k_rlc_g1_l0 calls it:
// partial k is a candidate when cand[k] != 0, its key is pid[k] (an index
// into the n_keys compressed keys), its digits u4[4 k ..].  complete = 0 is
// the control: the mixed addition without the doubling branch (jac_add_aff_x)
// in place of the complete one; *exc then says whether an addition met equal
// operands.  out48: P_d compressed.  Returns 0, 1 when P_d is the point at
// infinity (the kernel's RLC_EACH), or a negative error.
int ls_duty(const uint8_t* pk48, int n_keys, const uint32_t* pid, const uint32_t* u4, const uint8_t* cand, int n,
            int complete, int* exc, uint8_t* out48) {
  if (n < 0 || n > MAX_N || n_keys <= 0) return -1;
  Keys keys;
  if (!keys.load(pk48, n_keys)) return -2;
  for (int k = 0; k < n; ++k)
    if (pid[k] >= (uint32_t)n_keys) return -1;
  auto get = [&](uint32_t k, const G1A*& t, uint32_t (&u)[4]) {
    if (!cand[k]) return false;
    t = keys.tab.data() + (size_t)PK_TAB_W2 * pid[k];
    for (int j = 0; j < 4; ++j) u[j] = u4[4ull * k + j];
    return true;
  };
  bool met = false;
  const Fp beta = fp_from_const(G1_BETA);
  const G1J P = complete ? rlc_duty_keys_l0f<Fp>((uint32_t)n, beta, get)
                         : rlc_duty_keys_l0f<Fp>((uint32_t)n, beta, get, [&](const G1J& p, const G1A& q) {
                             return jac_add_aff_x(p, q, met);
                           });
  if (exc) *exc = met ? 1 : 0;
  return put(P, out48);
}

// The expectation: sum over the candidates of rlc_mul_key_l0f(tab_i, beta,
// u_i) -- the per-partial kernel's product -- added with the complete
// Jacobian addition (jac_add: doubling and infinity cases included).
int ls_reference(const uint8_t* pk48, int n_keys, const uint32_t* pid, const uint32_t* u4, const uint8_t* cand, int n,
                 uint8_t* out48) {
  if (n < 0 || n > MAX_N || n_keys <= 0) return -1;
  Keys keys;
  if (!keys.load(pk48, n_keys)) return -2;
  G1J P = jac_inf<Fp>();
  for (int k = 0; k < n; ++k) {
    if (!cand[k]) continue;
    if (pid[k] >= (uint32_t)n_keys) return -1;
    const uint32_t u[4] = {u4[4ull * k], u4[4ull * k + 1], u4[4ull * k + 2], u4[4ull * k + 3]};
    P = jac_add(P, rlc_mul_key_l0f(keys.tab.data() + (size_t)PK_TAB_W2 * pid[k], fp_from_const(G1_BETA), u));
  }
  return put(P, out48);
}

// Work-model probe (tools/count_work.py builds this file with TBG_COUNT_OPS):
// the multiply-adds of one duty's P_d, Jacobian (the conversion is counted
// with the batched inversion's share elsewhere).
unsigned long long ls_count_get(void) { return tbg_mad_count; }
void ls_count_reset(void) { tbg_mad_count = 0; }
static Keys g_keys;
int ls_probe_setup(const uint8_t* pk48, int n_keys) { return g_keys.load(pk48, n_keys) ? 0 : -2; }
// the per-partial form's same work: n products and their sum (k_rlc_duty_sum's additions)
int ls_probe_partials(const uint32_t* pid, const uint32_t* u4, int n) {
  const Keys& keys = g_keys;
  G1J P = jac_inf<Fp>();
  for (int k = 0; k < n; ++k) {
    const uint32_t u[4] = {u4[4ull * k], u4[4ull * k + 1], u4[4ull * k + 2], u4[4ull * k + 3]};
    P = jac_add_in<Fp, true>(P, rlc_mul_key_l0f(keys.tab.data() + (size_t)PK_TAB_W2 * pid[k], fp_from_const(G1_BETA), u));
  }
  return jac_is_inf(P) ? 1 : 0;
}
int ls_probe_duty(const uint32_t* pid, const uint32_t* u4, int n) {
  const Keys& keys = g_keys;
  const G1J P = rlc_duty_keys_l0f<Fp>((uint32_t)n, fp_from_const(G1_BETA), [&](uint32_t k, const G1A*& t, uint32_t (&u)[4]) {
    t = keys.tab.data() + (size_t)PK_TAB_W2 * pid[k];
    for (int j = 0; j < 4; ++j) u[j] = u4[4ull * k + j];
    return true;
  });
  return jac_is_inf(P) ? 1 : 0;
}

}  // extern "C"
