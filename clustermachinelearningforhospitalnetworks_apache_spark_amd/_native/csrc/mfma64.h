// Device helpers shared by the kernels on v_mfma_f64_16x16x4_f64 (K13t, K27 .. K32).
//
// The f64 MFMA computes D[16][16] += A[16][4] B[4][16] per wave, one f64 of each operand and four of D per lane:
//   lane l holds A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15];
//   register r of the result on lane l is D[row (l >> 4) + 4 r][col l & 15].
// This is the f64 form, not the bf16 C/D map. The kernels call c = lane & 15 and g = lane >> 4 ("lane group"), so a
// lane's four results are rows g, g + 4, g + 8, g + 12 of column c. Where a kernel feeds one product's result to
// the next product as the B operand, K-step r takes register r, and the k index it stands for is g + 4 r: hence
// the lane -> unit map below.
#pragma once
#include "common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));  // the accumulator of one 16 x 16 block

// Exact bf16 -> f64: the 16 bits sit in the high half of the word (low half zero).
__device__ __forceinline__ double bf16hi_to_f64(unsigned bits16_in_high_half) {
  return (double)__uint_as_float(bits16_in_high_half);
}

// Column index of an f64 LDS image row `unit`, XORed so that a ds_read_b64 of a half wave falls on 32 distinct
// doubles mod 32 both with lanes along columns and lane groups along units, and the other way round (lda.hip has
// the argument). The caller adds unit * pitch.
__device__ __forceinline__ int unit_swizzle(int unit, int col) {
  return col ^ ((2 * (unit & 15)) ^ (16 * (unit & 1)));
}

// The contiguous run [t0, t1) of `ntiles` tiles that belongs to this workgroup: the grid cuts them into equal runs.
__device__ __forceinline__ void tile_run(long long ntiles, long long& t0, long long& t1) {
  t0 = ntiles * blockIdx.x / gridDim.x;
  t1 = ntiles * (blockIdx.x + 1) / gridDim.x;
}
// ... that belongs to part `index` of `count`, where a workgroup is not a part (gram's slabs).
__device__ __forceinline__ void tile_run(long long ntiles, int index, int count, long long& t0, long long& t1) {
  t0 = ntiles * index / count;
  t1 = ntiles * (index + 1) / count;
}

// The unit (row of a 16 T-row operand) behind index i of the 4 T values a lane of group g holds.
__device__ __forceinline__ int unit_of_lane(int i, int g) { return 16 * (i >> 2) + g + 4 * (i & 3); }

// Sum over the four lane groups (lanes c, c + 16, c + 32, c + 48); every lane gets the sum. The argument comes by
// reference: by value the compiler allocates the callers' registers in another order.
__device__ __forceinline__ double lane_groups_sum(const double& x) {
  double v = x;
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
