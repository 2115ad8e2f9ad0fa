// TEST TOOLING ONLY: the stand-alone sanitizer run of the fixed-schedule Fr
// arithmetic.  frct_host.cpp with a main() of its own, compiled
// -fsanitize=address,undefined by tests/frct and run as a subprocess by
// tests/test_frct_host.py: nothing is loaded into Python.  argv[1] is a file
// of 32-byte big-endian operands, all below r.  Every ordered pair goes
// through every operation in both instantiations; beyond the sanitizers'
// verdict the run checks that the two agree and a few identities, and exits
// non-zero on the first miss.
#include <cstdio>
#include <vector>
#include "frct_host.cpp"

static int fail(const char* what, size_t i, size_t j) {
  fprintf(stderr, "frct_main: %s at operands %zu, %zu\n", what, i, j);
  return 1;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> v;
  uint8_t buf[32];
  while (fread(buf, 1, 32, f) == 32) v.insert(v.end(), buf, buf + 32);
  fclose(f);
  const size_t n = v.size() / 32;
  if (n < 8) return 2;
  uint8_t one[32] = {}, zero[32] = {};
  one[31] = 1;
  uint64_t counts[K_N], first_counts[K_N];
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j) {
      const uint8_t *a = &v[32 * i], *b = &v[32 * j];
      uint8_t x[32], y[32];
      for (int op = OP_ADD; op <= OP_ZERO_MASK; ++op) {
        if (frh_ops(op, a, b, 1, x) != 0 || frh_count_op(op, a, b, counts, y) != 0) return fail("an operation failed", i, j);
        if (memcmp(x, y, 32) != 0) return fail("the two instantiations differ", i, j);
      }
      frh_ops(OP_ADD, a, b, 1, x);
      frh_ops(OP_SUB, x, b, 1, y);
      if (memcmp(y, a, 32) != 0) return fail("(a + b) - b != a", i, j);
      frh_ops(OP_SUB, a, a, 1, x);
      if (memcmp(x, zero, 32) != 0) return fail("a - a != 0", i, j);
      frh_ops(OP_MUL, a, one, 1, x);
      if (memcmp(x, a, 32) != 0) return fail("a * 1 != a", i, j);
    }
  // Horner and the interpolation over windows of the operands: a split of threshold t at the
  // identifiers 1..t recombines to coefficient 0, with the same counts whatever the operands
  const uint32_t ts[] = {2, 3, 7};
  for (uint32_t t : ts) {
    for (size_t w = 0; w + t <= n; ++w) {
      const uint8_t* coef = &v[32 * w];
      std::vector<uint8_t> shares(32 * t), ids(t);
      uint8_t ladder[32], secret[32], s2[32], l2[32];
      uint32_t z, z2;
      for (uint32_t id = 1; id <= t; ++id) {
        ids[id - 1] = (uint8_t)id;
        if (frh_horner(coef, t, id, &shares[32 * (id - 1)], ladder, &z) != 0) return fail("horner failed", w, id);
        if (frh_count_horner(coef, t, id, counts, s2, l2, &z2) != 0) return fail("counting horner failed", w, id);
        if (memcmp(s2, &shares[32 * (id - 1)], 32) != 0 || memcmp(l2, ladder, 32) != 0 || z != z2)
          return fail("horner: the two instantiations differ", w, id);
        if (z ? memcmp(ladder, one, 32) != 0 : memcmp(ladder, s2, 32) != 0) return fail("the ladder scalar is wrong", w, id);
      }
      frh_combine(shares.data(), ids.data(), t, secret, &z);
      frh_count_combine(shares.data(), ids.data(), t, counts, s2, &z2);
      if (memcmp(secret, s2, 32) != 0 || z != z2) return fail("combine: the two instantiations differ", w, t);
      if (memcmp(secret, coef, 32) != 0) return fail("the shares do not recombine to the secret", w, t);
      if (w == 0) memcpy(first_counts, counts, sizeof(counts));
      else if (memcmp(first_counts, counts, sizeof(counts)) != 0) return fail("operation counts depend on the operands", w, t);
    }
  }
  printf("frct_main ok: %zu operands\n", n);
  return 0;
}
