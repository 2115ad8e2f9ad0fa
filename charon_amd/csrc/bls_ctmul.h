// Fixed-schedule scalar multiplication [k] P for a SECRET k and a public base
// point P (the hardened signer: k_keyed.hip, tbg_sk_to_pk_ct / tbg_sign_ct).
//
// Written once over the field type F (Fp for G1, Fp2 for G2) through the f_*
// overload set alone; tests/ctmul instantiates it a second time over a
// counting field type that defines no f_is_zero and no f_eq, so the template
// cannot test a field value.
//
// What makes the schedule independent of k:
//   * the group law is the complete one of Renes, Costello and Batina
//     ("Complete addition formulas for prime order elliptic curves", 2016;
//     Algorithms 7 and 9, a = 0) in homogeneous projective coordinates with
//     O = (0 : 1 : 0) -- no exceptional case, hence no test of a coordinate;
//   * k + 0x77..7 (one 256-bit addition) written in base 16 has the nibbles
//     e_i = d_i + 7 of the signed digits d_i in [-7, 8] with k = sum d_i 16^i:
//     the carry out of nibble i of that addition is exactly the recoding's
//     carry (n_i + c_i > 8).  For 0 < k < r the top nibble of k is at most 7,
//     so nothing is carried out of the top;
//   * per window: 4 doublings, a scan of ALL nine table entries |d| = 0..8
//     with a mask per entry, a masked negation and one addition: 64 windows,
//     256 doublings and 64 additions for every k;
//   * the digits stay in eight registers that are shifted by one nibble per
//     window: nothing is indexed by a digit, neither memory nor registers.
// The table (multiples 0..8 of P, projective) is public and comes from a
// reader object: coord(e, c) is coordinate c of entry e.
//
// Value bounds (bls_field.h): every coordinate that enters or leaves ct_add /
// ct_dbl is reduced (< 2p, normalised limbs).  The second operand of every
// product is normalised and at most 16p (fp2_mul negates its c1).
#pragma once
#include "bls_curve.h"

namespace tbg {

// ---- the overloads the ladder needs beyond bls_curve.h's set ----
// mask: all ones (take a) or zero (take b)
TBG_HD Fp f_select(uint32_t mask, const Fp& a, const Fp& b) {
  Fp r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = b.l[i] ^ ((a.l[i] ^ b.l[i]) & mask);
  return r;
}
TBG_HD Fp2 f_select(uint32_t mask, const Fp2& a, const Fp2& b) {
  return {f_select(mask, a.c0, b.c0), f_select(mask, a.c1, b.c1)};
}
// mask ? -a : a (a reduced; the result is reduced)
TBG_HD Fp f_cneg(uint32_t mask, const Fp& a) { return f_select(mask, fp_reduce(fp_neg(a)), a); }
TBG_HD Fp2 f_cneg(uint32_t mask, const Fp2& a) { return f_select(mask, fp2_reduce(fp2_neg(a)), a); }
// b3 a for b3 = 3b: 12 on E1, 12 (1 + u) on E2.  a reduced; the result is
// normalised and below 216p: the caller reduces it.
TBG_HD Fp f_mul_b3(const Fp& a) { return fp_mul_small(a, 12); }
TBG_HD Fp2 f_mul_b3(const Fp2& a) { return fp2_mul_small(fp2_mul_xi(a), 12); }

template <class F> struct CtPoint { F X, Y, Z; };

template <class F> TBG_HD CtPoint<F> ct_inf() { return {f_zero<F>(), f_one<F>(), f_zero<F>()}; }
template <class F> TBG_HD CtPoint<F> ct_from_aff(const Aff<F>& a) { return {a.x, a.y, f_one<F>()}; }

// P + Q, complete (Algorithm 7): 12 products, 2 products by b3.
template <class F> TBG_HD CtPoint<F> ct_add_in(const CtPoint<F>& p, const CtPoint<F>& q) {
  F t0 = f_mul(p.X, q.X);
  F t1 = f_mul(p.Y, q.Y);
  F t2 = f_mul(p.Z, q.Z);
  const F t3 = f_reduce(f_sub_l(f_mul(f_add_l(p.X, p.Y), f_add(q.X, q.Y)), f_add(t0, t1)));
  const F t4 = f_reduce(f_sub_l(f_mul(f_add_l(p.Y, p.Z), f_add(q.Y, q.Z)), f_add(t1, t2)));
  F Y3 = f_reduce(f_sub_l(f_mul(f_add_l(p.X, p.Z), f_add(q.X, q.Z)), f_add(t0, t2)));
  t0 = f_small(t0, 3);                     // < 6p
  t2 = f_reduce(f_mul_b3(t2));
  F Z3 = f_add(t1, t2);                    // < 4p
  t1 = f_reduce(f_sub_l(t1, t2));
  Y3 = f_reduce(f_mul_b3(Y3));
  const F X3 = f_reduce(f_sub_l(f_mul(t3, t1), f_mul(t4, Y3)));
  Y3 = f_reduce(f_add_l(f_mul(t1, Z3), f_mul(Y3, t0)));
  Z3 = f_reduce(f_add_l(f_mul(Z3, t4), f_mul(t3, t0)));
  return {X3, Y3, Z3};
}

// 2 P, complete (Algorithm 9): 6 products, 2 squarings, 1 product by b3.
template <class F> TBG_HD CtPoint<F> ct_dbl_in(const CtPoint<F>& p) {
  F t0 = f_sqr(p.Y);
  F Z3 = f_small(t0, 8);                   // < 16p
  const F t1 = f_mul(p.Y, p.Z);
  F t2 = f_reduce(f_mul_b3(f_sqr(p.Z)));
  F X3 = f_mul(t2, Z3);
  F Y3 = f_add(t0, t2);                    // < 4p
  Z3 = f_mul(t1, Z3);
  t2 = f_small(t2, 3);                     // < 6p
  t0 = f_reduce(f_sub_l(t0, t2));
  Y3 = f_reduce(f_add_l(f_mul(t0, Y3), X3));
  X3 = f_mul(f_add_l(t0, t0), f_mul(p.X, p.Y));
  return {X3, Y3, Z3};
}

// One copy of each law per kernel (TBG_NI, bls_field.h): the operands travel
// through the scratch stack, at addresses the compiler chose.
template <class F> TBG_NI CtPoint<F> ct_add(const CtPoint<F>& p, const CtPoint<F>& q) { return ct_add_in(p, q); }
template <class F> TBG_NI CtPoint<F> ct_dbl(const CtPoint<F>& p) { return ct_dbl_in(p); }

constexpr int CT_WINDOWS = 64;   // 4-bit windows of a 256-bit scalar
constexpr int CT_ENTRIES = 9;    // table entries: the multiples 0..8
constexpr uint32_t CT_BIAS = 0x77777777u;

// k (eight little-endian words, 0 < k < r) -> the words of k + 0x77..7, whose
// nibble i is d_i + 7.
TBG_HD void ct_recode(const uint32_t (&k)[8], uint32_t (&e)[8]) {
  uint64_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t s = (uint64_t)k[i] + CT_BIAS + carry;
    e[i] = (uint32_t)s;
    carry = s >> 32;
  }
}

// The multiples 0..8 of an affine base point, handed to store(e, point).
template <class F, class Store> TBG_HD void ct_build_table(const Aff<F>& base, Store&& store) {
  const CtPoint<F> b = ct_from_aff(base);
  CtPoint<F> acc = ct_inf<F>();
  for (int e = 0; e < CT_ENTRIES; ++e) {
    store(e, acc);
    acc = ct_add(acc, b);
  }
}

// [k] P.  tab.coord(e, c): coordinate c (0: X, 1: Y, 2: Z) of [e] P.
template <class F, class Tab> TBG_HD CtPoint<F> ct_mul(const Tab& tab, const uint32_t (&k)[8]) {
  uint32_t e[8];
  ct_recode(k, e);
  CtPoint<F> acc = ct_inf<F>();
  for (int w = 0; w < CT_WINDOWS; ++w) {
    for (int j = 0; j < 4; ++j) acc = ct_dbl(acc);
    // the window's digit: the top nibble, then the words move up one nibble
    const int32_t d = (int32_t)(e[7] >> 28) - 7;
#pragma unroll
    for (int i = 7; i > 0; --i) e[i] = (e[i] << 4) | (e[i - 1] >> 28);
    e[0] <<= 4;
    const uint32_t neg = (uint32_t)(d >> 31);            // all ones: d < 0
    const uint32_t mag = ((uint32_t)d ^ neg) - neg;      // |d|
    CtPoint<F> t = {f_zero<F>(), f_zero<F>(), f_zero<F>()};
    for (uint32_t en = 0; en < (uint32_t)CT_ENTRIES; ++en) {
      const uint32_t x = en ^ mag;                       // 0 only for the digit's entry
      const uint32_t m = ((x | (0u - x)) >> 31) - 1u;    // all ones there, else 0
      t.X = f_select(m, tab.coord((int)en, 0), t.X);
      t.Y = f_select(m, tab.coord((int)en, 1), t.Y);
      t.Z = f_select(m, tab.coord((int)en, 2), t.Z);
    }
    t.Y = f_cneg(neg, t.Y);
    acc = ct_add(acc, t);
  }
  return acc;
}

// ---- to affine, Z inverted by Fermat (its value depends on k) ----
// Z != 0: [k] P is not the identity for 0 < k < r and P of order r.
TBG_HD G1A ct_to_aff(const CtPoint<Fp>& p) {
  const Fp zi = fp_inv_fermat(p.Z);
  return {fp_mul(p.X, zi), fp_mul(p.Y, zi)};
}
TBG_HD G2A ct_to_aff(const CtPoint<Fp2>& p) {
  // 1 / (a + bu) = (a - bu) / (a^2 + b^2), the norm inverted by Fermat
  const Fp t = fp_inv_fermat(fp_mul2(p.Z.c0, p.Z.c0, p.Z.c1, p.Z.c1));
  const Fp2 zi = {fp_mul(p.Z.c0, t), fp_mul(fp_neg(p.Z.c1), t)};
  return {fp2_mul(p.X, zi), fp2_mul(p.Y, zi)};
}

// ---- the table in device memory ----
// Word w of entry e of table m is at (e * W + w) * n_tab + m, W = 3
// coordinates of F: the lanes of a wave that hold neighbouring messages read
// neighbouring words, and lanes that share a message (one table: the G1
// generator; one signing root for a whole ceremony) read one address.  The
// index m is public (item_msg); e runs over every entry.
template <class F> struct CtWords;
template <> struct CtWords<Fp> { static constexpr uint32_t N = NL; };
template <> struct CtWords<Fp2> { static constexpr uint32_t N = 2 * NL; };
template <class F> constexpr uint32_t ct_tab_words_per() { return (uint32_t)CT_ENTRIES * 3u * CtWords<F>::N; }

TBG_HD void ct_load(const uint32_t* p, size_t stride, Fp& out) {
#pragma unroll
  for (int i = 0; i < NL; ++i) out.l[i] = p[stride * (size_t)i];
}
TBG_HD void ct_load(const uint32_t* p, size_t stride, Fp2& out) {
  ct_load(p, stride, out.c0);
  ct_load(p + stride * (size_t)NL, stride, out.c1);
}
TBG_HD void ct_store(uint32_t* p, size_t stride, const Fp& v) {
#pragma unroll
  for (int i = 0; i < NL; ++i) p[stride * (size_t)i] = v.l[i];
}
TBG_HD void ct_store(uint32_t* p, size_t stride, const Fp2& v) {
  ct_store(p, stride, v.c0);
  ct_store(p + stride * (size_t)NL, stride, v.c1);
}

template <class F> struct CtTabMem {
  const uint32_t* base;  // table m's first word
  size_t n_tab;
  TBG_HD F coord(int e, int c) const {
    F v;
    ct_load(base + ((size_t)e * 3u + (size_t)c) * CtWords<F>::N * n_tab, n_tab, v);
    return v;
  }
};
template <class F> TBG_HD void ct_tab_store(uint32_t* base, size_t n_tab, int e, const CtPoint<F>& p) {
  const size_t cw = (size_t)CtWords<F>::N * n_tab;
  ct_store(base + ((size_t)e * 3u + 0u) * cw, n_tab, p.X);
  ct_store(base + ((size_t)e * 3u + 1u) * cw, n_tab, p.Y);
  ct_store(base + ((size_t)e * 3u + 2u) * cw, n_tab, p.Z);
}

}  // namespace tbg
