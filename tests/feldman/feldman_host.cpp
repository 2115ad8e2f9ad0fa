// TEST TOOLING ONLY: host (CPU) build of the Feldman commitment evaluation
// (charon_amd/csrc/bls_feldman.h) for tests/test_feldman_host.py, with the
// value bound checks (TBG_BOUNDS_CHECK) switched on.  fvh_eval takes the
// arguments of tbg_eval_commitments and does what its two kernels do, one
// evaluation after the other: g1_decompress of every commitment, fv_eval,
// to-affine (a plain inversion here), g1_compress.  Modelled on tests/ctmul.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../charon_amd/csrc/bls_feldman.h"

using namespace tbg;

extern "C" {

int fvh_eval(const uint8_t* commit48, const uint32_t* poly_first, uint32_t n_polys, const uint32_t* eval_poly,
             const uint32_t* eval_id, uint32_t n_evals, uint8_t* out48, int32_t* eval_status, int32_t* commit_status) {
  const uint32_t nc = n_polys ? poly_first[n_polys] : 0;
  std::vector<G1A> tab(nc);
  std::vector<int32_t> st(nc);
  for (uint32_t i = 0; i < nc; ++i) {
    G1A a{fp_zero(), fp_zero()};
    st[i] = g1_decompress(commit48 + 48ull * i, a);
    if (st[i] != DEC_OK) a = G1A{fp_zero(), fp_zero()};
    tab[i] = a;
    commit_status[i] = st[i];
  }
  for (uint32_t e = 0; e < n_evals; ++e) {
    if (eval_poly[e] >= n_polys) return -1;
    const uint32_t first = poly_first[eval_poly[e]], t = poly_first[eval_poly[e] + 1] - first;
    G1J acc;
    const int32_t s = fv_eval(tab.data() + first, st.data() + first, t, eval_id[e], acc);
    uint8_t* out = out48 + 48ull * e;
    if (s == FV_OK || s == FV_IDENTITY) {
      G1A a{fp_zero(), fp_zero()};
      const bool aff = jac_to_aff(acc, a);
      g1_compress(a, !aff, out);
    } else {
      memset(out, 0, 48);
    }
    eval_status[e] = s;
  }
  return 0;
}

// [k] P for a compressed point (fv_mul_u32 alone): out48, -1 when P does not decode
int fvh_mul(const uint8_t* p48, uint32_t k, uint8_t* out48) {
  G1A a{fp_zero(), fp_zero()};
  const int32_t st = g1_decompress(p48, a);
  if ((st != DEC_OK && st != DEC_IDENTITY) || k == 0) return -1;
  const G1J r = fv_mul_u32(st == DEC_OK ? jac_from_aff(a) : jac_inf<Fp>(), k);
  G1A o{fp_zero(), fp_zero()};
  const bool aff = jac_to_aff(r, o);
  g1_compress(o, !aff, out48);
  return 0;
}

}  // extern "C"
