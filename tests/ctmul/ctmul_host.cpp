// TEST TOOLING ONLY: host (CPU) build of the hardened signer's ladder
// (charon_amd/csrc/bls_ctmul.h) for tests/test_ctmul_host.py, with the value
// bound checks (TBG_BOUNDS_CHECK) switched on.  The template runs three times:
// over Fp (G1), over Fp2 (G2, through the device's table layout) and over a
// counting field type that defines no f_is_zero and no f_eq -- that it
// compiles shows the ladder tests no field value.  Modelled on tests/l0tail.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../charon_amd/csrc/bls_ctmul.h"

namespace tbg {

// ---- the counting field type: Fp underneath, every overload the ladder may
// call counted.  (No f_is_zero, no f_eq, no f_inv.)
enum CtCount : int { C_MUL, C_SQR, C_ADD, C_SUB, C_REDUCE, C_SMALL, C_B3, C_SELECT, C_CNEG, C_N };
static uint64_t g_count[C_N];
struct CFp { Fp v; };
inline CFp f_mul(const CFp& a, const CFp& b) { ++g_count[C_MUL]; return {fp_mul(a.v, b.v)}; }
inline CFp f_sqr(const CFp& a) { ++g_count[C_SQR]; return {fp_sqr(a.v)}; }
inline CFp f_add(const CFp& a, const CFp& b) { ++g_count[C_ADD]; return {fp_add(a.v, b.v)}; }
inline CFp f_add_l(const CFp& a, const CFp& b) { ++g_count[C_ADD]; return {fp_add_l(a.v, b.v)}; }
inline CFp f_sub_l(const CFp& a, const CFp& b) { ++g_count[C_SUB]; return {fp_sub_l(a.v, b.v)}; }
inline CFp f_reduce(const CFp& a) { ++g_count[C_REDUCE]; return {fp_reduce(a.v)}; }
inline CFp f_small(const CFp& a, uint32_t k) { ++g_count[C_SMALL]; return {fp_mul_small(a.v, k)}; }
inline CFp f_mul_b3(const CFp& a) { ++g_count[C_B3]; return {f_mul_b3(a.v)}; }
inline CFp f_select(uint32_t m, const CFp& a, const CFp& b) { ++g_count[C_SELECT]; return {f_select(m, a.v, b.v)}; }
inline CFp f_cneg(uint32_t m, const CFp& a) { ++g_count[C_CNEG]; return {f_cneg(m, a.v)}; }
template <> inline CFp f_zero<CFp>() { return {fp_zero()}; }
template <> inline CFp f_one<CFp>() { return {fp_one()}; }

}  // namespace tbg

using namespace tbg;

namespace {

template <class F> struct HostTab {
  CtPoint<F> e[CT_ENTRIES];
  F coord(int en, int c) const { return c == 0 ? e[en].X : c == 1 ? e[en].Y : e[en].Z; }
};

void words_from_be32(const uint8_t* b, uint32_t (&w)[8]) {
  for (int i = 0; i < 8; ++i)
    w[i] = ((uint32_t)b[31 - 4 * i]) | ((uint32_t)b[30 - 4 * i] << 8) | ((uint32_t)b[29 - 4 * i] << 16) |
           ((uint32_t)b[28 - 4 * i] << 24);
}

// compressed (identity encoding included) <-> projective, for the law checks
bool g1_in(const uint8_t* b, CtPoint<Fp>& p) {
  G1A a;
  const int32_t st = g1_decompress(b, a);
  if (st == DEC_IDENTITY) { p = ct_inf<Fp>(); return true; }
  if (st != DEC_OK) return false;
  p = ct_from_aff(a);
  return true;
}
bool g2_in(const uint8_t* b, CtPoint<Fp2>& p) {
  G2A a;
  const int32_t st = g2_decompress(b, a);
  if (st == DEC_IDENTITY) { p = ct_inf<Fp2>(); return true; }
  if (st != DEC_OK) return false;
  p = ct_from_aff(a);
  return true;
}
// (the harness may test Z; the ladder may not)
void g1_out(const CtPoint<Fp>& p, uint8_t* out) {
  const bool inf = fp_is_zero(p.Z);
  G1A a{};
  if (!inf) a = ct_to_aff(p);
  g1_compress(a, inf, out);
}
void g2_out(const CtPoint<Fp2>& p, uint8_t* out) {
  const bool inf = fp2_is_zero(p.Z);
  G2A a{};
  if (!inf) a = ct_to_aff(p);
  g2_compress(a, inf, out);
}

}  // namespace

extern "C" {

// [k_i] G1 for n 32-byte big-endian scalars: out48[n][48]
int ctm_g1_mul(const uint8_t* sk32, uint32_t n, uint8_t* out48) {
  const G1A g = {fp_from_const(G1_X), fp_from_const(G1_Y)};
  HostTab<Fp> T;
  ct_build_table(g, [&](int e, const CtPoint<Fp>& p) { T.e[e] = p; });
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t w[8];
    words_from_be32(sk32 + 32ull * i, w);
    g1_out(ct_mul<Fp>(T, w), out48 + 48ull * i);
  }
  return 0;
}

// [k_i] Q for the compressed G2 point base96, through the device's table
// layout: Q's table is table `slot` of `n_tab` (the others hold another
// point's multiples, so a wrong stride or index changes the result).
int ctm_g2_mul(const uint8_t* base96, const uint8_t* other96, uint32_t n_tab, uint32_t slot, const uint8_t* sk32, uint32_t n,
               uint8_t* out96) {
  G2A q, o;
  if (g2_decompress(base96, q) != DEC_OK || g2_decompress(other96, o) != DEC_OK || slot >= n_tab) return -1;
  std::vector<uint32_t> tab((size_t)ct_tab_words_per<Fp2>() * n_tab);
  for (uint32_t m = 0; m < n_tab; ++m)
    ct_build_table(m == slot ? q : o, [&](int e, const CtPoint<Fp2>& p) { ct_tab_store(tab.data() + m, n_tab, e, p); });
  const CtTabMem<Fp2> T = {tab.data() + slot, n_tab};
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t w[8];
    words_from_be32(sk32 + 32ull * i, w);
    g2_out(ct_mul<Fp2>(T, w), out96 + 96ull * i);
  }
  return 0;
}

// the laws on compressed points (the identity encoding is a valid input):
// sum = P + Q, dbl = 2 P
int ctm_g1_law(const uint8_t* p48, const uint8_t* q48, uint8_t* sum48, uint8_t* dbl48) {
  CtPoint<Fp> p, q;
  if (!g1_in(p48, p) || !g1_in(q48, q)) return -1;
  g1_out(ct_add(p, q), sum48);
  g1_out(ct_dbl(p), dbl48);
  return 0;
}
int ctm_g2_law(const uint8_t* p96, const uint8_t* q96, uint8_t* sum96, uint8_t* dbl96) {
  CtPoint<Fp2> p, q;
  if (!g2_in(p96, p) || !g2_in(q96, q)) return -1;
  g2_out(ct_add(p, q), sum96);
  g2_out(ct_dbl(p), dbl96);
  return 0;
}

// the recoding: digits[64] of k, least significant first
void ctm_digits(const uint8_t* sk32, int32_t* digits) {
  uint32_t w[8], e[8];
  words_from_be32(sk32, w);
  ct_recode(w, e);
  for (int i = 0; i < 64; ++i) digits[i] = (int32_t)((e[i >> 3] >> (4 * (i & 7))) & 15u) - 7;
}

uint32_t ctm_count_kinds() { return C_N; }

// the ladder over the counting type on the G1 generator: counts[n][C_N] of
// the ladder alone (the table is built before the counters are zeroed), and
// the products themselves (out48), which must equal ctm_g1_mul's
int ctm_count(const uint8_t* sk32, uint32_t n, uint64_t* counts, uint8_t* out48) {
  const Aff<CFp> g = {{fp_from_const(G1_X)}, {fp_from_const(G1_Y)}};
  HostTab<CFp> T;
  ct_build_table(g, [&](int e, const CtPoint<CFp>& p) { T.e[e] = p; });
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t w[8];
    words_from_be32(sk32 + 32ull * i, w);
    memset(g_count, 0, sizeof(g_count));
    const CtPoint<CFp> r = ct_mul<CFp>(T, w);
    memcpy(counts + (size_t)C_N * i, g_count, sizeof(g_count));
    g1_out(CtPoint<Fp>{r.X.v, r.Y.v, r.Z.v}, out48 + 48ull * i);
  }
  return 0;
}

}  // extern "C"
