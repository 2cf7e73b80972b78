// K31: the Gram matrix [X 1 z]^T W [X 1 z] of bf16 rows with 31 <= d <= 512 feature columns (gfx950).
//
// With a_r = [x_r[:d], 1, z_r], m = d + 2 and w_r = 1 without a weight: G[i][j] = sum_r a_ri (w_r a_rj), all f64
// after the exact bf16 -> f64 widening; z and w are f64 and never pass through bf16. The weight goes on one side
// (no sqrt). Only the upper triangle is computed; gram_fold_kernel mirrors it, so G is exactly symmetric.
//
// The output is a grid of 16 x 16 f64 blocks: NT = ceil(d / 16) column tiles of X and one augmented tile
// U = [1, z, 0, ..]. The X tiles are grouped in panels of 8 (128 columns, at most 4 panels). A workgroup of 256
// threads (4 waves) owns one panel pair (p <= q) for a contiguous run (slab) of 64-row tiles:
//   off-diagonal pair  64 blocks, wave v the 4 x 4 arrangement of row tiles 4 (v >> 1) .. + 3 of panel p and
//                      column tiles 4 (v & 1) .. + 3 of panel q: a 4-row K-step reads 4 A and 4 B operands for
//                      16 MFMAs into 128 accumulator VGPRs.
//   diagonal pair      waves 0, 1, 3 the same arrangement restricted to tile i <= tile j (10 + 16 + 10 blocks);
//                      wave 2, whose 4 x 4 arrangement lies below the diagonal, takes the 8 (tile, U) blocks of
//                      the panel and (U, U) instead. The fold reads (U, U) from pair (0, 0).
//   Blocks whose tiles lie past NT are skipped (wave-uniform masks), so a narrow d costs what it needs.
// Per 64-row tile: the rows of the one or two panels go to LDS as bf16, once; columns >= d and rows >= n are
// stored as 0, rows >= n get w = 0 and z = 0, so that pad columns (which may hold NaN bits) and rows past the
// view never reach a product. z and w of the tile are staged as f64 side arrays. The global loads of a tile are
// issued one tile ahead and wait in registers while the previous tile is computed (K30's scheme).
// Operands follow the f64 MFMA layout of v_mfma_f64_16x16x4_f64 (mfma64.h): for block (ti, tj) and K-step s both
// operands are read at LDS row 4 s + (l >> 4), column 16 t + (l & 15); the B side is multiplied by w[row] in
// f64 after the widening. The LDS pitch is 128 + 16 bf16 = 72 dwords, so the four row groups of a wave read
// banks 8 dwords apart (16 lanes of a group cover 8 dwords): no conflict.
// At the end of its run a workgroup writes its 64 block slots (16 per wave, [row][col]) to part[slab][pair];
// gram_fold_kernel adds the slabs in slab order and writes the mirrored (m, m) matrix. No atomics, the grid
// depends on (n, d, CUs) only, every loop is bounded by n: two calls give the same bits.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): gram_pass_kernel
// 216 VGPRs (of them 128 accumulators) at __launch_bounds__(256, 2), no scratch, 37 888 B LDS (two panels
// 2 * 64 * 144 * 2 B + z and w 2 * 64 * 8 B): two workgroups per CU. gram_fold_kernel: no LDS, no scratch.
#include "mfma64.h"

namespace {

constexpr int kGrThreads = 256;
constexpr int kGrTile = 64;            // rows per tile
constexpr int kGrPanel = 128;          // columns per panel: 8 tiles of 16
constexpr int kGrXP = kGrPanel + 16;   // bf16 pitch of a staged row
constexpr int kGrSlots = 64;           // block slots of a workgroup: 16 per wave
constexpr int kGrMaxD = 512;
constexpr int kGrMinD = 31;

__host__ __device__ constexpr int gr_tiles(int d) { return (d + 15) / 16; }
__host__ __device__ constexpr int gr_panels(int d) { return (gr_tiles(d) + 7) / 8; }
__host__ __device__ constexpr int gr_pairs(int d) { return gr_panels(d) * (gr_panels(d) + 1) / 2; }
// index of panel pair (p <= q) among np panels, rows of the upper triangle in order
__host__ __device__ constexpr int gr_pair_index(int p, int q, int np) { return p * np - p * (p - 1) / 2 + (q - p); }

__global__ __launch_bounds__(kGrThreads, 2) void gram_pass_kernel(
    const u16* __restrict__ X, long long n, long long ldx, int wc, int d, const double* __restrict__ z,
    const double* __restrict__ w, double* __restrict__ part, int npairs) {
  __shared__ __align__(16) u16 Xs[2][kGrTile][kGrXP];
  __shared__ double zs[kGrTile];
  __shared__ double ws[kGrTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int nt = gr_tiles(d), np = gr_panels(d);
  const int pair = blockIdx.x % npairs, slab = blockIdx.x / npairs, nslabs = gridDim.x / npairs;
  int p = 0, q = 0;
  for (int i = 0, pp = 0; pp < np; ++pp)
    for (int qq = pp; qq < np; ++qq, ++i)
      if (i == pair) {
        p = pp;
        q = qq;
      }
  const bool diag = p == q;
  const int nslot = diag ? 1 : 2;   // staged panels
  const int sb = diag ? 0 : 1;      // LDS slot of the B side
  const bool uwave = diag && wave == 2;
  const int ai = wave >> 1, bj = wave & 1;
  // live blocks of this wave: bit 4 i + j of the 4 x 4 arrangement, or bit t of the (tile, U) blocks and bit 8 (U, U)
  unsigned live = 0;
  if (uwave) {
    for (int t = 0; t < 8; ++t)
      if (8 * p + t < nt) live |= 1u << t;
    live |= 1u << 8;
  } else {
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        const int ti = 8 * p + 4 * ai + i, tj = 8 * q + 4 * bj + j;
        if (ti < nt && tj < nt && ti <= tj) live |= 1u << (4 * i + j);
      }
  }

  f64x4 acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = (f64x4)0.0;

  const long long ntiles = (n + kGrTile - 1) / kGrTile;
  long long t0, t1;
  tile_run(ntiles, slab, nslabs, t0, t1);

  // One item = 8 bf16 of one row (16 bytes); a thread holds its 4 items per panel of a tile in registers. The loads
  // of tile + 1 are issued before the products of tile. wc is a multiple of 8, so a chunk is inside the row or not.
  uint4 pf[2][4];
  double pz = 0.0, pw = 0.0;
  auto fetch = [&](long long tile) {
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
      const int col0 = kGrPanel * (sl == 0 ? p : q);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int it = tid + kGrThreads * k, row = it >> 4, col = col0 + 8 * (it & 15);
        const long long r = tile * kGrTile + row;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (sl < nslot && r < n && col < wc && col < d)
          v = *reinterpret_cast<const uint4*>(X + r * ldx + col);
        pf[sl][k] = v;
      }
    }
    if (tid < kGrTile) {
      const long long r = tile * kGrTile + tid;
      const bool in = r < n;
      pz = in ? z[r] : 0.0;
      pw = in ? (w != nullptr ? w[r] : 1.0) : 0.0;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
      if (sl < nslot) {
        const int col0 = kGrPanel * (sl == 0 ? p : q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int it = tid + kGrThreads * k, row = it >> 4, cc = it & 15;
          const int nv = d - (col0 + 8 * cc);  // live columns of this chunk (<= 0: none, >= 8: all)
          auto mk = [nv](int e) { return (2 * e < nv ? 0x0000ffffu : 0u) | (2 * e + 1 < nv ? 0xffff0000u : 0u); };
          uint4 v = pf[sl][k];
          v.x &= mk(0);
          v.y &= mk(1);
          v.z &= mk(2);
          v.w &= mk(3);
          *reinterpret_cast<uint4*>(&Xs[sl][row][8 * cc]) = v;
        }
      }
    }
    if (tid < kGrTile) {
      zs[tid] = pz;
      ws[tid] = pw;
    }
  };

  if (t0 < t1) fetch(t0);
  for (long long tile = t0; tile < t1; ++tile) {
    stage();
    __syncthreads();
    if (tile + 1 < t1) fetch(tile + 1);
    if (uwave) {
#pragma unroll 2
      for (int s = 0; s < kGrTile / 4; ++s) {
        const int row = 4 * s + g;
        const double u = c == 0 ? 1.0 : (c == 1 ? zs[row] : 0.0);
        const double ub = ws[row] * u;
#pragma unroll
        for (int t = 0; t < 8; ++t)
          if (live & (1u << t))
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)bf16_to_f32(Xs[0][row][16 * t + c]), ub, acc[t], 0, 0, 0);
        acc[8] = __builtin_amdgcn_mfma_f64_16x16x4f64(u, ub, acc[8], 0, 0, 0);
      }
    } else if (live) {
#pragma unroll 2
      for (int s = 0; s < kGrTile / 4; ++s) {
        const int row = 4 * s + g;
        const double wv = ws[row];
        double a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[i] = (double)bf16_to_f32(Xs[0][row][16 * (4 * ai + i) + c]);
          b[i] = wv * (double)bf16_to_f32(Xs[sb][row][16 * (4 * bj + i) + c]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (live & (1u << (4 * i + j)))
              acc[4 * i + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[4 * i + j], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // slot 16 wave + k, [row][col]: register r of a lane is row (lane >> 4) + 4 r, column lane & 15
  double* pu = part + ((long long)slab * npairs + pair) * (kGrSlots * 256) + (long long)wave * 16 * 256;
#pragma unroll
  for (int k = 0; k < 16; ++k)
#pragma unroll
    for (int r = 0; r < 4; ++r) pu[k * 256 + (g + 4 * r) * 16 + c] = acc[k][r];
}

// G[i][j] for every (i, j) of the (m, m) output: the entry (min, max) of the upper triangle, summed over the slabs in
// slab order.
__global__ __launch_bounds__(256) void gram_fold_kernel(const double* __restrict__ part, int nslabs, int npairs, int d,
                                                        double* __restrict__ out) {
  const int m = d + 2;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)m * m) return;
  const int i = (int)(e / m), j = (int)(e % m);
  const int a = i < j ? i : j, b = i < j ? j : i;
  const int np = gr_panels(d);
  int pair, slot, row, col;
  if (b < d) {
    const int ta = a >> 4, tb = b >> 4, p = ta >> 3, q = tb >> 3, li = ta & 7, lj = tb & 7;
    pair = gr_pair_index(p, q, np);
    slot = 16 * (2 * (li >> 2) + (lj >> 2)) + 4 * (li & 3) + (lj & 3);
    row = a & 15;
    col = b & 15;
  } else if (a < d) {
    const int ta = a >> 4, p = ta >> 3;
    pair = gr_pair_index(p, p, np);
    slot = 16 * 2 + (ta & 7);
    row = a & 15;
    col = b - d;
  } else {
    pair = 0;
    slot = 16 * 2 + 8;
    row = a - d;
    col = b - d;
  }
  const long long off = (long long)pair * (kGrSlots * 256) + slot * 256 + row * 16 + col;
  const long long ps = (long long)npairs * (kGrSlots * 256);
  double s = 0.0;
  for (int k = 0; k < nslabs; ++k) s += part[k * ps + off];
  out[e] = s;
}

}  // namespace

// Row slabs of a launch: a function of (n, d, CUs) only; two workgroups per CU over the panel pairs, at most one
// slab per 64-row tile. 0 = unsupported width or no row.
CML_API int cml_gram_mfma_slabs(long long n, int d, int ncu) {
  if (d < kGrMinD || d > kGrMaxD || n <= 0) return 0;
  const long long tiles = (n + kGrTile - 1) / kGrTile;
  long long cap = 2LL * (ncu > 0 ? ncu : 256) / gr_pairs(d);
  if (cap < 1) cap = 1;
  return (int)(tiles < cap ? tiles : cap);
}

// Doubles of the partial buffer per slab.
CML_API long long cml_gram_mfma_part(int d) {
  if (d < kGrMinD || d > kGrMaxD) return 0;
  return (long long)gr_pairs(d) * kGrSlots * 256;
}

// X: bf16 [n, >= d] rows of pitch ldx elements (16-byte pitch and base), wc >= d readable columns of a row (a multiple
// of 8, so that every 8-column chunk is inside the row or outside it); z: f64 [n]; w: f64 [n] or null;
// part: f64 [slabs * cml_gram_mfma_part(d)] scratch; out: f64 [(d + 2)^2].
CML_API int cml_gram_mfma(const void* X, long long n, long long ldx, int wc, int d, const double* z, const double* w,
                          double* part, int slabs, double* out, int ncu, void* stream) {
  if (d < kGrMinD || d > kGrMaxD || n <= 0 || X == nullptr || z == nullptr || part == nullptr || out == nullptr ||
      (reinterpret_cast<size_t>(X) & 15) != 0 || (ldx & 7) != 0 || (wc & 7) != 0 || wc < d || ldx < wc ||
      slabs != cml_gram_mfma_slabs(n, d, ncu))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int npairs = gr_pairs(d);
  hipLaunchKernelGGL(gram_pass_kernel, dim3((unsigned)(slabs * npairs)), dim3(kGrThreads), 0, st, (const u16*)X, n, ldx,
                     wc, d, z, w, part, npairs);
  const int rc = cml_status();
  if (rc != 0) return rc;
  return cml_launch_fold(gram_fold_kernel, (long long)(d + 2) * (d + 2), st, part, slabs, npairs, d, out);
}
