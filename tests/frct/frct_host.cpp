// TEST TOOLING ONLY: host (CPU) build of the fixed-schedule Fr arithmetic
// (charon_amd/csrc/bls_frct.h) for tests/test_frct_host.py, with the value
// bound checks (TBG_BOUNDS_CHECK) switched on.  The header is instantiated
// twice: over uint32_t, as the kernels of k_shares.hip do, and over a counting
// word type that defines NO comparison, NO operator bool and NO conversion to
// an integer -- that the second instantiation compiles shows the header tests
// no value.  Modelled on tests/ctmul.  frct_main.cpp includes this file and
// adds a main() for the stand-alone sanitizer run.
#include <cstdint>
#include <cstring>
#include "../../charon_amd/csrc/bls_frct.h"

namespace tbg {

// ---- the counting word types: uint32_t / uint64_t underneath, every operator
// the header may use counted by kind.  Construction from a public constant or
// a loaded byte, and the explicit conversions between the two widths, are the
// only ways in; the harness reads .v, the header cannot.
enum FrCount : int { K_ADD, K_SUB, K_MUL, K_AND, K_OR, K_XOR, K_NOT, K_SHL, K_SHR, K_WIDEN, K_NARROW, K_N };
static uint64_t g_count[K_N];
struct CW64;
struct CW {
  uint32_t v;
  CW() = default;
  explicit CW(uint32_t x) : v(x) {}
  explicit CW(const CW64& w);
};
struct CW64 {
  uint64_t v;
  CW64() = default;
  explicit CW64(const CW& w) : v(w.v) { ++g_count[K_WIDEN]; }
};
inline CW::CW(const CW64& w) : v((uint32_t)w.v) { ++g_count[K_NARROW]; }
template <> struct FrctWide<CW> { using type = CW64; };

#define FRCT_BINOP(T, op, kind) \
  inline T operator op(const T& a, const T& b) { ++g_count[kind]; T r; r.v = a.v op b.v; return r; }
FRCT_BINOP(CW, +, K_ADD)
FRCT_BINOP(CW, -, K_SUB)
FRCT_BINOP(CW, *, K_MUL)
FRCT_BINOP(CW, &, K_AND)
FRCT_BINOP(CW, |, K_OR)
FRCT_BINOP(CW, ^, K_XOR)
FRCT_BINOP(CW64, +, K_ADD)
FRCT_BINOP(CW64, *, K_MUL)
#undef FRCT_BINOP
inline CW operator~(const CW& a) { ++g_count[K_NOT]; CW r; r.v = ~a.v; return r; }
inline CW operator<<(const CW& a, int s) { ++g_count[K_SHL]; CW r; r.v = a.v << s; return r; }
inline CW operator>>(const CW& a, int s) { ++g_count[K_SHR]; CW r; r.v = a.v >> s; return r; }
inline CW64 operator>>(const CW64& a, int s) { ++g_count[K_SHR]; CW64 r; r.v = a.v >> s; return r; }

}  // namespace tbg

using namespace tbg;

namespace {

template <class W> W word_in(uint8_t b);
template <> uint32_t word_in<uint32_t>(uint8_t b) { return b; }
template <> CW word_in<CW>(uint8_t b) { return CW((uint32_t)b); }
inline uint8_t byte_out(uint32_t w) { return (uint8_t)w; }
inline uint8_t byte_out(const CW& w) { return (uint8_t)w.v; }  // (the harness may; the header may not)
inline uint32_t raw(uint32_t w) { return w; }
inline uint32_t raw(const CW& w) { return w.v; }

template <class W> FrCt<W> in32(const uint8_t* p) {
  W b[32];
  for (int j = 0; j < 32; ++j) b[j] = word_in<W>(p[j]);
  return frct_from_be32(b);
}
template <class W> void out32(const FrCt<W>& a, uint8_t* p) {
  W b[32];
  frct_to_be32(a, b);
  for (int j = 0; j < 32; ++j) p[j] = byte_out(b[j]);
}

enum Op : int { OP_ADD = 0, OP_SUB = 1, OP_MUL = 2, OP_ROUND = 3, OP_SELECT_A = 4, OP_SELECT_B = 5, OP_ZERO_MASK = 6 };

template <class W> int run_op(int op, const uint8_t* a32, const uint8_t* b32, uint8_t* out) {
  const FrCt<W> a = in32<W>(a32), b = in32<W>(b32);
  switch (op) {
    case OP_ADD: out32(frct_add(a, b), out); return 0;
    case OP_SUB: out32(frct_sub(a, b), out); return 0;
    case OP_MUL: out32(frct_mul(a, b), out); return 0;  // (a R)(b R) / R = a b R: the field product
    case OP_ROUND: out32(a, out); return 0;
    case OP_SELECT_A: out32(frct_select(W(0u) - W(1u), a, b), out); return 0;
    case OP_SELECT_B: out32(frct_select(W(0u), a, b), out); return 0;
    case OP_ZERO_MASK: {
      const uint32_t m = raw(frct_zero_mask(a));
      memset(out, 0, 32);
      for (int j = 0; j < 4; ++j) out[28 + j] = (uint8_t)(m >> (24 - 8 * j));
      return 0;
    }
  }
  return -1;
}

template <class W> void run_horner(const uint8_t* coef32, uint32_t t, uint32_t id, uint8_t* share32, uint8_t* ladder32,
                                   uint32_t* zero) {
  const FrCt<W> s = frct_horner<W>(fr_from_u32(id), t, [&](uint32_t j, W(&b)[32]) {
    for (int k = 0; k < 32; ++k) b[k] = word_in<W>(coef32[32ull * j + k]);
  });
  // what k_split_ct writes: the share, the ladder's scalar, the flag
  const W zm = frct_zero_mask(s);
  out32(s, share32);
  out32(frct_select(zm, frct_pub<W>(fr_from_limbs(R_ONE_M)), s), ladder32);
  *zero = raw(zm & W(1u));
}

template <class W> void run_combine(const uint8_t* value32, const uint8_t* ids, uint32_t m, uint8_t* secret32, uint32_t* zero) {
  const FrCt<W> acc = frct_interpolate_at_zero<W>(ids, m, [&](uint32_t i, W(&b)[32]) {
    for (int k = 0; k < 32; ++k) b[k] = word_in<W>(value32[32ull * i + k]);
  });
  out32(acc, secret32);
  *zero = raw(frct_zero_mask(acc) & W(1u));
}

}  // namespace

extern "C" {

// out32[i] = op(a32[i], b32[i]) for n operand pairs (32 bytes big-endian each, all < r)
int frh_ops(int op, const uint8_t* a32, const uint8_t* b32, uint32_t n, uint8_t* out) {
  for (uint32_t i = 0; i < n; ++i)
    if (run_op<uint32_t>(op, a32 + 32ull * i, b32 + 32ull * i, out + 32ull * i) != 0) return -1;
  return 0;
}

// f(id) by Horner's rule over t coefficients, lowest first, as k_split_ct forms it
int frh_horner(const uint8_t* coef32, uint32_t t, uint32_t id, uint8_t* share32, uint8_t* ladder32, uint32_t* zero) {
  if (t == 0) return -1;
  run_horner<uint32_t>(coef32, t, id, share32, ladder32, zero);
  return 0;
}

// the interpolation at 0 over m shares, as k_combine_ct forms it
int frh_combine(const uint8_t* value32, const uint8_t* ids, uint32_t m, uint8_t* secret32, uint32_t* zero) {
  run_combine<uint32_t>(value32, ids, m, secret32, zero);
  return 0;
}

uint32_t frh_count_kinds() { return K_N; }

// the same three over the counting type: counts[K_N] of the whole computation, and the result,
// which must equal the uint32_t instantiation's
int frh_count_op(int op, const uint8_t* a32, const uint8_t* b32, uint64_t* counts, uint8_t* out) {
  memset(g_count, 0, sizeof(g_count));
  const int rc = run_op<CW>(op, a32, b32, out);
  memcpy(counts, g_count, sizeof(g_count));
  return rc;
}
int frh_count_horner(const uint8_t* coef32, uint32_t t, uint32_t id, uint64_t* counts, uint8_t* share32, uint8_t* ladder32,
                     uint32_t* zero) {
  if (t == 0) return -1;
  memset(g_count, 0, sizeof(g_count));
  run_horner<CW>(coef32, t, id, share32, ladder32, zero);
  memcpy(counts, g_count, sizeof(g_count));
  return 0;
}
int frh_count_combine(const uint8_t* value32, const uint8_t* ids, uint32_t m, uint64_t* counts, uint8_t* secret32,
                      uint32_t* zero) {
  memset(g_count, 0, sizeof(g_count));
  run_combine<CW>(value32, ids, m, secret32, zero);
  memcpy(counts, g_count, sizeof(g_count));
  return 0;
}

}  // extern "C"
