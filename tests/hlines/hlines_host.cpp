// TEST TOOLING ONLY: host (CPU) twin of the H(m)-lines kernel's projective
// Miller steps (charon_amd/csrc/bls_pair.h hline_dbl_s / hline_add_s,
// k_lines_h through px_h_lines) for tests/test_hlines_host.py, in the
// single-lane Fp2 form and with the lane pairs emulated (Fp2p), with the
// value bound checks (TBG_BOUNDS_CHECK) switched on.  Built with
// TBG_COUNT_OPS instead it is tools/count_work.py's probe of the kernel's
// work.  Modelled on tests/hostcheck and tests/sgbpair.
#include <cstdint>
#include <cstring>
#include "../../charon_amd/csrc/bls_pairing.h"
#include "../../charon_amd/csrc/bls_h2c.h"
#include "../../charon_amd/csrc/bls_pair.h"

extern "C" unsigned long long tbg_mad_count = 0;

using namespace tbg;

namespace {

Fp from_be(const uint8_t* b) {
  bool lt;
  return fp_to_mont(fp_limbs_from_be48(b, &lt));
}
void to_be(const Fp& a, uint8_t* b) { fp_limbs_to_be48(fp_from_mont(a), b); }
void f2_out(const Fp2& a, uint8_t* b) {
  to_be(a.c0, b);
  to_be(a.c1, b + 48);
}
G2A aff_in(const uint8_t* b) { return {{from_be(b), from_be(b + 48)}, {from_be(b + 96), from_be(b + 144)}}; }
void f12_out(const Fp12& f, uint8_t* b) {
  const Fp2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
  for (int i = 0; i < 6; ++i) f2_out(*c[i], b + 96 * i);
}

Fp2 plain(const Fp2& a) { return a; }
Fp2 plain(const Fp2p& a) { return pp_to(a); }
template <class F> F lift(const Fp2& a);
template <> Fp2 lift<Fp2>(const Fp2& a) { return a; }
template <> Fp2p lift<Fp2p>(const Fp2& a) { return pp_from(a); }

// the 68 lines of q by the projective steps in representation F, as Line
// structs in loop order; *end (may be null) receives the point after the loop
template <class F>
void new_lines(const G2A& q, Line* out, Prj<F>* end) {
  const Aff<F> Q{lift<F>(q.x), lift<F>(q.y)};
  Prj<F> T = prj_from_aff(Q);
  int idx = 0;
  auto put = [&](const LineG<F>& l) { out[idx++] = Line{plain(l.l0), plain(l.l1), plain(l.l4)}; };
  for (int i = 62; i >= 0; --i) {
    put(hline_dbl_g(T));
    if ((X_ABS >> i) & 1) put(hline_add_g(T, Q));
  }
  if (end) *end = T;
}

// the Miller value of (P, Q) from 68 UNEVALUATED lines: l1 (-x_P), l4 y_P
// folded in here, as the kernels that read h_lines do
Fp12 miller_from_lines(const Line* ls, const G1A& P) {
  const Fp nx = fp_reduce(fp_neg(P.x));
  Fp12 f = fp12_one();
  int idx = 0;
  for (int i = 62; i >= 0; --i) {
    if (i != 62) f = fp12_sqr(f);
    for (int k = 0; k < 1 + (int)((X_ABS >> i) & 1); ++k) {
      const Line& l = ls[idx++];
      f = fp12_mul_by_014(f, l.l0, fp2_mul_fp(l.l1, nx), fp2_mul_fp(l.l4, P.y));
    }
  }
  return fp12_conj(f);
}

void pinned_lines(const G2A& q, const Fp& nx, const Fp& y, Line* out) {
  static uint32_t w[LINES_WORDS];
  g2_lines(q, nx, y, w);
  for (int i = 0; i < N_LINES; ++i) out[i] = line_load(w + LINE_WORDS * i);
}

}  // namespace

extern "C" {

unsigned long long hl_count_get(void) { return tbg_mad_count; }
void hl_count_reset(void) { tbg_mad_count = 0; }

// H(m) in affine form (x.c0, x.c1, y.c0, y.c1; 48 canonical big-endian bytes each); 0, or -1 for infinity
int hl_hash(const uint8_t* msg, uint32_t len, uint8_t* aff192) {
  G2A a;
  if (!jac_to_aff(hash_to_g2(msg, len), a)) return -1;
  f2_out(a.x, aff192);
  f2_out(a.y, aff192 + 96);
  return 0;
}

// The 68 steps on q (affine, as hl_hash writes it): form 0 = Fp2, 1 = the
// emulated lane pair.  new288 / ref288: per step (l0, l1, l4) of the new
// steps and of g2_lines(q, one, one), 3 x 96 canonical bytes each; end192:
// the point after the loop made affine (X / Z, Y / Z).  Returns 0, -1 for a
// bad form, -2 when the loop ends at infinity.
int hl_steps(const uint8_t* q192, int form, uint8_t* new288, uint8_t* ref288, uint8_t* end192) {
  const G2A q = aff_in(q192);
  Line nl[N_LINES], rl[N_LINES];
  Fp2 X, Y, Z;
  if (form == 0) {
    Prj<Fp2> T;
    new_lines<Fp2>(q, nl, &T);
    X = T.X, Y = T.Y, Z = T.Z;
  } else if (form == 1) {
    Prj<Fp2p> T;
    new_lines<Fp2p>(q, nl, &T);
    X = pp_to(T.X), Y = pp_to(T.Y), Z = pp_to(T.Z);
  } else {
    return -1;
  }
  pinned_lines(q, fp_one(), fp_one(), rl);
  for (int i = 0; i < N_LINES; ++i) {
    const Fp2* n[3] = {&nl[i].l0, &nl[i].l1, &nl[i].l4};
    const Fp2* r[3] = {&rl[i].l0, &rl[i].l1, &rl[i].l4};
    for (int k = 0; k < 3; ++k) {
      f2_out(*n[k], new288 + 288 * i + 96 * k);
      f2_out(*r[k], ref288 + 288 * i + 96 * k);
    }
  }
  if (fp2_is_zero(Z)) return -2;
  const Fp2 zi = fp2_inv(Z);
  f2_out(fp2_mul(X, zi), end192);
  f2_out(fp2_mul(Y, zi), end192 + 96);
  return 0;
}

// The words k_lines_h stores for q: the emulated pair's lines in the engine's
// layout (LINES_WORDS words; Montgomery form, < 2p, 28-bit limbs).
void hl_words(const uint8_t* q192, uint32_t* out) {
  Line nl[N_LINES];
  new_lines<Fp2p>(aff_in(q192), nl, nullptr);
  for (int i = 0; i < N_LINES; ++i) line_store(out + LINE_WORDS * i, nl[i]);
}

// final_exp of the Miller value of (p, q) from q's stored lines evaluated at
// p (p96: x, y): which = 0 the new lines (pair form), 1 the pinned ones
// (g2_lines with P left out), 2 the new lines with l1 NEGATED (the control).
int hl_pairing(const uint8_t* p96, const uint8_t* q192, int which, uint8_t* out576) {
  const G1A P{from_be(p96), from_be(p96 + 48)};
  const G2A q = aff_in(q192);
  Line ls[N_LINES];
  if (which == 1) {
    pinned_lines(q, fp_one(), fp_one(), ls);
  } else if (which == 0 || which == 2) {
    new_lines<Fp2p>(q, ls, nullptr);
    if (which == 2)
      for (auto& l : ls) l.l1 = fp2_reduce(fp2_neg(l.l1));
  } else {
    return -1;
  }
  f12_out(final_exp(miller_from_lines(ls, P)), out576);
  return 0;
}

// e(pk, H(m)) e(-g1, sig) == 1 with H(m)'s lines from the new steps and the
// signature's from the pinned form with -g1 folded in (k_l0_lines /
// k_lines_fold keep it): 1 true, 0 false, < 0 decode error.
int hl_verify(const uint8_t* pk48, const uint8_t* msg, uint32_t len, const uint8_t* sig96) {
  G1A pk;
  G2A sig, h;
  if (g1_decompress(pk48, pk) != DEC_OK) return -1;
  if (g2_decompress(sig96, sig) != DEC_OK) return -2;
  if (!jac_to_aff(hash_to_g2(msg, len), h)) return -3;
  Line hl[N_LINES], sl[N_LINES];
  new_lines<Fp2p>(h, hl, nullptr);
  pinned_lines(sig, fp_reduce(fp_neg(fp_from_const(G1_X))), fp_from_const(G1_NEG_Y), sl);
  // the folded lines again "evaluated" at (x, y) = (-1, 1): l1, l4 unchanged
  const G1A unit{fp_reduce(fp_neg(fp_one())), fp_one()};
  const Fp12 f = fp12_mul(miller_from_lines(hl, pk), miller_from_lines(sl, unit));
  return fp12_is_one(final_exp(f)) ? 1 : 0;
}

// tools/count_work.py: the work of one k_lines_h item (both lanes of the pair)
void hl_probe_lines(const uint8_t* q192) {
  Line nl[N_LINES];
  new_lines<Fp2p>(aff_in(q192), nl, nullptr);
}

}  // extern "C"
