// The cofactor-clearing half of tests/devcheck's hash-to-G2 harness
// (devcheck_h2c.hip): this source #includes charon_amd/csrc/k_hash_clear.hip
// itself and is compiled with the flags charon_amd/_native.py gives that
// unit, so k_hash_clear_x1 / _x2 / _fin and launch_hash_clear are the
// product's own text as the product builds it.  TEST TOOLING ONLY.
#include "../../charon_amd/csrc/k_hash_clear.hip"

using namespace tbg;

// stage 0 / 1 / 2: k_hash_clear_x1 / _x2 / _fin alone, with launch_hash_clear's grid
void dc_h2c_clear_stage(int stage, const DevBatch& B, hipStream_t st) {
  if (!B.n_msgs) return;
  const dim3 grid = grid_for(2 * B.n_msgs);
  if (stage == 0) TBG_KLAUNCH(k_hash_clear_x1, grid, dim3(kBlock), st, B);
  else if (stage == 1) TBG_KLAUNCH(k_hash_clear_x2, grid, dim3(kBlock), st, B);
  else if (stage == 2) TBG_KLAUNCH(k_hash_clear_fin, grid, dim3(kBlock), st, B);
}
