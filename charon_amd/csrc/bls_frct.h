// Fr on a fixed schedule, for SECRET operands (k_shares.hip: tbg_split_secret_ct
// / tbg_combine_shares_ct -- polynomial coefficients, shares, share values and
// combined secrets).  bls_fr.h serves public data: its fr_sub branches on the
// borrow and its fr_csub returns one of two values by a test.  This sibling
// keeps the representation (10 limbs of 28 bits, Montgomery R = 2^280, the
// constants of bls_constants.h) and tests nothing.
//
// Written once over the limb word type W and its double-width partner
// FrctWide<W>::type, through the operators + - * & | ^ ~ << >> alone and mask
// selects: no value is compared, none is converted to bool or to an integer,
// nothing is indexed by a value (every index and shift count below is a loop
// counter or a constant).  The only conversions are the explicit ones between
// W and its wide partner and from public constants into W.  tests/frct
// instantiates the header a second time over a counting word type that
// defines no comparison, no operator bool and no integer conversion: that it
// compiles shows the header tests no value.
//
// Public multipliers (an identifier, a Lagrange coefficient) are ordinary Fr
// of bls_fr.h and enter through frct_pub.  Every FrCt that leaves a function
// below is canonical: normalised limbs, value < r.
#pragma once
#include "bls_fr.h"

namespace tbg {

template <class W> struct FrctWide;
template <> struct FrctWide<uint32_t> { using type = uint64_t; };

template <class W> struct FrCt { W l[NLR]; };

template <class W> TBG_HD FrCt<W> frct_zero() {
  FrCt<W> r;
#pragma unroll
  for (int i = 0; i < NLR; ++i) r.l[i] = W(0u);
  return r;
}
// a public Fr (Montgomery form stays Montgomery form)
template <class W> TBG_HD FrCt<W> frct_pub(const Fr& a) {
  FrCt<W> r;
#pragma unroll
  for (int i = 0; i < NLR; ++i) r.l[i] = W(a.l[i]);
  return r;
}

// mask: all ones (take a) or zero (take b)
template <class W> TBG_HD FrCt<W> frct_select(W mask, const FrCt<W>& a, const FrCt<W>& b) {
  FrCt<W> r;
#pragma unroll
  for (int i = 0; i < NLR; ++i) r.l[i] = b.l[i] ^ ((a.l[i] ^ b.l[i]) & mask);
  return r;
}

// all ones iff a == 0 (a canonical)
template <class W> TBG_HD W frct_zero_mask(const FrCt<W>& a) {
  W o = W(0u);
#pragma unroll
  for (int i = 0; i < NLR; ++i) o = o | a.l[i];
  return ((o | (W(0u) - o)) >> 31) - W(1u);
}

// a - r if a >= r, else a (a < 2r, normalised limbs): the difference is always
// formed and the borrow out of the top limb chooses by mask.
template <class W> TBG_HD FrCt<W> frct_csub(const FrCt<W>& a) {
  FrCt<W> d;
  W borrow = W(0u);
#pragma unroll
  for (int i = 0; i < NLR; ++i) {
    const W s = a.l[i] - W(R_L[i]) - borrow;  // wraps below zero: bit 31 is the borrow
    d.l[i] = s & W(LMASK);
    borrow = s >> 31;
  }
  return frct_select(W(0u) - borrow, a, d);
}

// a + b mod r
template <class W> TBG_HD FrCt<W> frct_add(const FrCt<W>& a, const FrCt<W>& b) {
  FrCt<W> s;
  W carry = W(0u);
#pragma unroll
  for (int i = 0; i < NLR; ++i) {
    const W t = a.l[i] + b.l[i] + carry;
    s.l[i] = t & W(LMASK);
    carry = t >> 28;
  }
  return frct_csub(s);  // (a + b < 2r < 2^256: nothing is carried out of limb 9)
}

// a - b mod r: the difference, then r & mask added whatever the borrow was
template <class W> TBG_HD FrCt<W> frct_sub(const FrCt<W>& a, const FrCt<W>& b) {
  FrCt<W> d;
  W borrow = W(0u);
#pragma unroll
  for (int i = 0; i < NLR; ++i) {
    const W s = a.l[i] - b.l[i] - borrow;
    d.l[i] = s & W(LMASK);
    borrow = s >> 31;
  }
  const W mask = W(0u) - borrow;
  W carry = W(0u);
#pragma unroll
  for (int i = 0; i < NLR; ++i) {
    const W t = d.l[i] + (W(R_L[i]) & mask) + carry;
    d.l[i] = t & W(LMASK);  // (the carry out of limb 9 cancels the borrow)
    carry = t >> 28;
  }
  return d;
}

// Montgomery product a b / R mod r (fr_mul's schedule), masked final correction
template <class W> TBG_HD FrCt<W> frct_mul(const FrCt<W>& a, const FrCt<W>& b) {
  using D = typename FrctWide<W>::type;
  W m[NLR];
  FrCt<W> r;
  D acc = D(W(0u));
#pragma unroll
  for (int k = 0; k < NLR; ++k) {
    D s = acc;
#pragma unroll
    for (int i = 0; i <= k; ++i) s = s + D(a.l[i]) * D(b.l[k - i]);
#pragma unroll
    for (int i = 0; i < k; ++i) s = s + D(m[i]) * D(W(R_L[k - i]));
    m[k] = (W(s) * W(RNINV)) & W(LMASK);
    s = s + D(m[k]) * D(W(R_L[0]));
    acc = s >> 28;
  }
#pragma unroll
  for (int k = NLR; k < 2 * NLR - 1; ++k) {
    D s = acc;
#pragma unroll
    for (int i = k - NLR + 1; i < NLR; ++i) s = s + D(a.l[i]) * D(b.l[k - i]) + D(m[i]) * D(W(R_L[k - i]));
    r.l[k - NLR] = W(s) & W(LMASK);
    acc = s >> 28;
  }
  r.l[NLR - 1] = W(acc);
  return frct_csub(r);  // (a b + m r) / R < 2r for a, b < r
}

// 32 big-endian bytes, one per word (each < 256), of a value ALREADY KNOWN to
// be below r -> Montgomery form.  Limb i is bits [28 i, 28 i + 28).
template <class W> TBG_HD FrCt<W> frct_from_be32(const W (&b)[32]) {
  W w[8];  // little-endian 32-bit words
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = b[31 - 4 * i] | (b[30 - 4 * i] << 8) | (b[29 - 4 * i] << 16) | (b[28 - 4 * i] << 24);
  FrCt<W> a;
#pragma unroll
  for (int i = 0; i < NLR; ++i) {
    const int bit = 28 * i, q = bit >> 5, s = bit & 31;
    W v = w[q] >> s;
    if (s > 4 && q + 1 < 8) v = v | (w[q + 1] << (32 - s));  // (s, q: constants of the unrolled loop)
    a.l[i] = v & W(LMASK);
  }
  return frct_mul(a, frct_pub<W>(fr_from_limbs(R_R2_M)));
}

// Montgomery form -> 32 big-endian bytes, one per word
template <class W> TBG_HD void frct_to_be32(const FrCt<W>& a, W (&b)[32]) {
  FrCt<W> one = frct_zero<W>();
  one.l[0] = W(1u);
  const FrCt<W> c = frct_mul(a, one);
  W w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = W(0u);
#pragma unroll
  for (int i = 0; i < NLR; ++i) {
    const int bit = 28 * i, q = bit >> 5, s = bit & 31;
    w[q] = w[q] | (c.l[i] << s);
    if (s > 4 && q + 1 < 8) w[q + 1] = w[q + 1] | (c.l[i] >> (32 - s));
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    b[31 - 4 * i] = w[i] & W(0xffu);
    b[30 - 4 * i] = (w[i] >> 8) & W(0xffu);
    b[29 - 4 * i] = (w[i] >> 16) & W(0xffu);
    b[28 - 4 * i] = w[i] >> 24;
  }
}

// Horner's rule at the public point x (Montgomery form) over t coefficients
// given as big-endian bytes, lowest first: coef(j, bytes) hands out
// coefficient j.  acc = a_(t-1), then acc = acc x + a_j for j = t-2 .. 0.  The
// trip count t is public.
template <class W, class Coef> TBG_HD FrCt<W> frct_horner(const Fr& x, uint32_t t, Coef&& coef) {
  const FrCt<W> xm = frct_pub<W>(x);
  W b[32];
  coef(t - 1, b);
  FrCt<W> acc = frct_from_be32(b);
  for (uint32_t j = t - 1; j-- > 0;) {
    coef(j, b);
    acc = frct_add(frct_mul(acc, xm), frct_from_be32(b));
  }
  return acc;
}

// lambda_i(0) = prod_(j != i) id_j / (id_j - id_i) mod r of PUBLIC identifiers, in Montgomery
// form (bls_tss.h's lagrange_at_zero_words without the conversion to words; bls_fr.h, variable
// time).  Colliding identifiers give 0 (fr_inv(0) = 0): the caller refuses such a set.
TBG_HD Fr fr_lagrange_at_zero(const uint8_t* ids, uint32_t m, uint32_t i) {
  const Fr one = fr_from_limbs(R_ONE_M);
  Fr num = one, den = one;
  const Fr xi = fr_from_u32(ids[i]);
  for (uint32_t j = 0; j < m; ++j) {
    if (j == i) continue;
    const Fr xj = fr_from_u32(ids[j]);
    num = fr_mul(num, xj);
    den = fr_mul(den, fr_sub(xj, xi));
  }
  return fr_mul(num, fr_inv(den));
}

// sum_i lambda_i(0) s_i mod r over the m shares of one set: value(i, bytes) hands out s_i as
// big-endian bytes.  The lambda_i are public; the products with s_i and the sum are masked.
template <class W, class Val> TBG_HD FrCt<W> frct_interpolate_at_zero(const uint8_t* ids, uint32_t m, Val&& value) {
  FrCt<W> acc = frct_zero<W>();
  W b[32];
  for (uint32_t i = 0; i < m; ++i) {
    value(i, b);
    acc = frct_add(acc, frct_mul(frct_from_be32(b), frct_pub<W>(fr_lagrange_at_zero(ids, m, i))));
  }
  return acc;
}

}  // namespace tbg
