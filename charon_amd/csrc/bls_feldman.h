// Evaluation of a Feldman commitment polynomial in G1 (tbls.NewTSS /
// getPubShare, reference tbls/tss.go:95-116, :293-325; kryptology
// FeldmanVerifier.Verify): for the t commitments C_j = [a_j] G1 of one
// polynomial and a public identifier id,
//
//   E(id) = C_0 + [id] C_1 + [id^2] C_2 + ... + [id^(t-1)] C_(t-1)
//
// by Horner's rule from the top coefficient down: acc = C_(t-1), then
// acc = [id] acc + C_j for j = t-2 .. 0.  [id] acc is a left-to-right
// double-and-add over the bits of id; with b the bit length of id and w its
// weight one Horner step is b - 1 doublings, w - 1 additions and one mixed
// addition, so an evaluation costs (t - 1) (b + w - 1) group operations
// (3-of-4 at id 4: 6; 7-of-10 at id 7: 30; a 256-bit ladder: 256 + 64).
//
// Everything here is public data: the schedule depends on id and on which
// commitments are the identity, and the additions are the complete ones of
// bls_curve.h -- equal operands ([id] acc == C_j), opposite operands
// ([id] acc == -C_j) and infinity in mid-chain all occur for crafted (and for
// some honest) polynomials, tests/edge_feldman.py.
#pragma once
#include "bls_curve.h"

namespace tbg {

// per-evaluation status (TBG_FV_* of include/tbls_gpu.h), in this precedence
constexpr int32_t FV_OK = 0;
constexpr int32_t FV_ID = -50;            // id == 0
constexpr int32_t FV_COMMIT = -51;        // a commitment of the polynomial failed to decode
constexpr int32_t FV_KEY_IDENTITY = -52;  // C_0 is the identity: no group key
constexpr int32_t FV_IDENTITY = -53;      // E(id) is the identity

// [k] p: left-to-right double-and-add over the bits of k (k = 1: p itself).
TBG_NI G1J fv_mul_u32(const G1J& p, uint32_t k) {
  if (k == 0) return jac_inf<Fp>();
  if (jac_is_inf(p)) return p;
  int top = 31;
  while (!((k >> top) & 1)) --top;
  G1J acc = p;
  for (int i = top - 1; i >= 0; --i) {
    acc = jac_dbl(acc);
    if ((k >> i) & 1) acc = jac_add(acc, p);
  }
  return acc;
}

// One evaluation: c[0..t) the decoded commitments of the polynomial, lowest
// coefficient first, st[0..t) their decode statuses (DEC_OK, DEC_IDENTITY or
// an error).  Returns the status; `out` holds E(id) for FV_OK (and infinity
// for every other status).
TBG_NI int32_t fv_eval(const G1A* c, const int32_t* st, uint32_t t, uint32_t id, G1J& out) {
  out = jac_inf<Fp>();
  if (id == 0) return FV_ID;
  for (uint32_t j = 0; j < t; ++j)
    if (st[j] != DEC_OK && st[j] != DEC_IDENTITY) return FV_COMMIT;
  if (st[0] == DEC_IDENTITY) return FV_KEY_IDENTITY;
  G1J acc = st[t - 1] == DEC_OK ? jac_from_aff(c[t - 1]) : jac_inf<Fp>();
  for (uint32_t j = t - 1; j-- > 0;) {
    acc = fv_mul_u32(acc, id);
    if (st[j] == DEC_OK) acc = jac_add_aff(acc, c[j]);
  }
  if (jac_is_inf(acc)) return FV_IDENTITY;
  out = acc;
  return FV_OK;
}

}  // namespace tbg
