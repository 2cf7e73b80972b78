// K32: loss and gradient (and the scores) of the second-order factorisation machine on bf16 rows (gfx950).
//
// Parameters b, w [d], V [d, f]. Per row x with label y, all f64 after the exact bf16 -> f64 widening:
//   t_u = sum_i x_i V_iu,  sv_i = sum_u V_iu^2,  s = b + sum_i w_i x_i + 1/2 (sum_u t_u^2 - sum_i x_i^2 sv_i)
//   squared:  l = 1/2 (s - y)^2,  r = s - y;   logistic:  l = softplus(s) - y s,  r = sigmoid(s) - y
//   db = sum_rows r,  dw_i = sum_rows r x_i,  u_i = sum_rows r x_i^2,  dV_iu = sum_rows x_i (r t_u) - V_iu u_i
// The sums are not divided by the number of rows. The scores form (fit = 0) writes s [n] and nothing else.
//
// The parameter image P = [V^T ; w ; 0 ..] has HP = 16 T rows ("units", T = 1 for f <= 15, 2 for f <= 31): unit
// u < f is factor u, unit f is the linear term. A persistent workgroup of 256 threads (4 waves, one per SIMD) keeps
// P [HP][DPT] in LDS as f64 for the whole launch, computes sv [dp] from it once, and walks a contiguous run of
// 64-row tiles. Per tile:
//   stage     the rows (through the row list where there is one) go to LDS as bf16, once; pad columns (>= d), rows
//             past the end and listed rows outside the matrix are stored as 0. Inside a 16-column block position
//             4 g + r holds column g + 4 r, so that lane group g reads its four values with one 8-byte load (K29's
//             order). The global loads of a tile are issued one tile ahead and wait in registers while the
//             previous tile is computed.
//   forward   a wave owns 16 rows, row = lane & 15, lane group g = lane >> 4, transposed on
//             v_mfma_f64_16x16x4_f64 (operand layout: mfma64.h): T^T[unit][row] = P[unit][k] X^T[k][row]. The x^2
//             sv term is one multiply and
//             one FMA per K-step on the operand the lane already holds; it, sum_u t_u^2 and the linear unit are
//             summed over the four lane groups. s, l and r are f64 VALU; rows past the end get r = 0 and no loss.
//             Column blocks go in pairs on two accumulation chains, and the LDS operands of a pair (x, P, sv) are
//             read while the pair before it is multiplied.
//   backward  D^T = [r t_u ; r ; 0 ..] of the tile goes to the staging buffer [HP][66], and after a barrier the wave
//             that owns a 16 x 16 block of dP for the whole launch adds sum_rows D^T[unit][row] X[row][col] to its
//             accumulator registers, 4 rows of depth per MFMA, with the staged bf16 rows as the B operand. Block
//             (t, tb) belongs to wave (tb T + t) & 3; the owner of (0, tb) also adds r x^2 to u of its column from
//             the same operand, r read from the staging buffer. A wave's blocks share their unit tile, so its A
//             operands and r are read once per tile; a block's rows are read while the block before it is
//             multiplied. db and the loss are per-lane sums.
// At the end a workgroup writes its partial [dP | u | db | loss]; fm_fold_kernel adds the partials in workgroup
// order, subtracts V_iu u_i and writes the flat layout [db | dw | dV (d x f, row-major) | loss]. No atomics, nothing
// of size n in global memory in the fit form, the grid depends on (rows, CUs) only, every loop is bounded.
//
// LDS reads of a half wave fall on 32 distinct doubles mod 32: the image uses K29's XOR of the column index with
// f(unit) = 2 (unit & 15) ^ 16 (unit & 1); the staging buffer has pitch 66 (2 c + g).
#include "mfma64.h"

namespace {

constexpr int kFmThreads = 256;
constexpr int kFmTile = 64;   // rows per tile: 16 per wave
constexpr int kFmSP = 66;     // f64 pitch of a staging row (64 rows of a tile)

__host__ __device__ constexpr int fm_dpt(int dp) { return dp < 64 ? 64 : dp; }  // compiled width class

// LDS bytes: the image HP DPT, sv DPT, the staging buffer HP 66, the fold of db and the loss 4 * 2 (all f64), the
// rows 64 (DPT + 8) bf16.
__host__ __device__ constexpr long long fm_lds_bytes(int dpt, int t) {
  const int hp = 16 * t;
  return 8LL * ((long long)hp * dpt + dpt + hp * kFmSP + 8) + 2LL * kFmTile * (dpt + 8);
}

__host__ __device__ constexpr bool fm_supported(int dp, int t) {
  if (dp < 16 || dp > 512 || (dp & (dp - 1)) != 0 || t < 1 || t > 2) return false;
  return fm_lds_bytes(fm_dpt(dp), t) <= kLdsPerCu;
}

__host__ __device__ constexpr long long fm_part_len(int dp, int t) { return (long long)16 * t * dp + dp + 2; }

template <int DPT, int T>
__global__ __launch_bounds__(kFmThreads, 1) void fm_pass_kernel(
    const u16* __restrict__ X, long long n, int dp, int d, int f, const long long* __restrict__ rows, long long B,
    const double* __restrict__ y, const double* __restrict__ wp, double* __restrict__ part,
    double* __restrict__ sout, int fit, int logistic) {
  constexpr int HP = 16 * T;
  constexpr int NI = 4 * T;             // units per lane: index i <-> unit 16 (i >> 2) + g + 4 (i & 3)
  constexpr int BP = DPT;
  constexpr int SP = kFmSP;
  constexpr int XP = DPT + 8;           // bf16 pitch of a staged row (K29's: pitch / 4 = 2 mod 4 doubles)
  constexpr int NBW = (T * (DPT / 16) + 3) / 4;  // blocks of dP per wave
  constexpr int NIT = DPT / 64;         // 16-column blocks of a tile per thread
  extern __shared__ __align__(16) unsigned char fm_smem[];
  double* Ps = reinterpret_cast<double*>(fm_smem);    // [HP][BP], column index swizzled by the unit
  double* svs = Ps + HP * BP;                         // [DPT]
  double* DS = svs + DPT;                             // [HP][SP]: D^T of the tile
  double* red = DS + HP * SP;                         // [4][2]
  u16* Xs = reinterpret_cast<u16*>(red + 8);          // [64][XP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int nb = dp >> 4;               // 16-column blocks of a row

  auto psw = [](int unit, int col) { return unit * BP + unit_swizzle(unit, col); };

  for (int i = tid; i < HP * dp; i += kFmThreads) Ps[psw(i / dp, i % dp)] = wp[i];
  const double bias = wp[(long long)HP * dp];
  __syncthreads();
  for (int i = tid; i < dp; i += kFmThreads) {
    double sv = 0.0;
    for (int u = 0; u < f; ++u) {
      const double v = Ps[psw(u, i)];
      sv += v * v;
    }
    svs[i] = sv;
  }

  int unit_of[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) unit_of[i] = unit_of_lane(i, g);

  f64x4 gp[NBW];
  double uacc[NBW];
#pragma unroll
  for (int s = 0; s < NBW; ++s) {
    gp[s] = (f64x4)0.0;
    uacc[s] = 0.0;
  }
  double dbacc = 0.0, lossacc = 0.0;

  const long long ntiles = (B + kFmTile - 1) / kFmTile;
  long long t0, t1;
  tile_run(ntiles, t0, t1);

  // The row of the matrix behind row ri of the walk; -1 = none (past the end, or a listed index outside [0, n)).
  auto source = [&](long long ri) -> long long {
    if (ri >= B) return -1;
    const long long src = rows ? rows[ri] : ri;
    return src >= 0 && src < n ? src : -1;
  };

  // One item = one 16-column block of one row (32 bytes); a thread holds its NIT items of a tile in registers.
  // The loads of tile + 1 are issued before the products of tile, so that no tile waits for HBM.
  uint4 pf[NIT][2];
  const int lnb = __ffs(nb) - 1;  // nb is a power of two
  auto fetch = [&](long long tile) {
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const int item = tid + kFmThreads * j;
      pf[j][0] = make_uint4(0u, 0u, 0u, 0u);
      pf[j][1] = pf[j][0];
      if (item < kFmTile * nb) {
        const long long src = source(tile * kFmTile + (item >> lnb));
        if (src >= 0) {
          const uint4* p = reinterpret_cast<const uint4*>(X + src * dp + 16 * (item & (nb - 1)));
          pf[j][0] = p[0];
          pf[j][1] = p[1];
        }
      }
    }
  };
  if (t0 < t1) fetch(t0);

  for (long long tile = t0; tile < t1; ++tile) {
    const long long base = tile * kFmTile;
    // ---- stage the fetched tile
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const int item = tid + kFmThreads * j;
      if (item < kFmTile * nb) {
        const int row = item >> lnb, tb = item & (nb - 1);
        // the same block as in lda.hip and mlp.hip: as a shared function it compiles to other machine code
        const unsigned w[8] = {pf[j][0].x, pf[j][0].y, pf[j][0].z, pf[j][0].w,
                               pf[j][1].x, pf[j][1].y, pf[j][1].z, pf[j][1].w};
        unsigned v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const unsigned b = (u & 1) ? (w[u >> 1] >> 16) : (w[u >> 1] & 0xffffu);
          v[u] = 16 * tb + u < d ? b : 0u;  // the pad columns are masked by d, not trusted
        }
        uint2* out = reinterpret_cast<uint2*>(Xs + row * XP + 16 * tb);
#pragma unroll
        for (int gg = 0; gg < 4; ++gg)
          out[gg] = make_uint2(v[gg] | (v[gg + 4] << 16), v[gg + 8] | (v[gg + 12] << 16));
      }
    }
    __syncthreads();  // also orders the sv stores before the first tile's reads

    // ---- forward: this wave's 16 rows
    const long long ri = base + wave * 16 + c;
    const long long src = source(ri);
    const bool valid = src >= 0;
    const double yv = fit && valid ? y[src] : 0.0;
    if (tile + 1 < t1) fetch(tile + 1);
    double cur[NI], q;
    {
      f64x4 z[2][T];  // two chains of column blocks
      double qq[2] = {0.0, 0.0};
#pragma unroll
      for (int t = 0; t < T; ++t) {
        z[0][t] = (f64x4)0.0;
        z[1][t] = (f64x4)0.0;
      }
      const u16* xrow = Xs + (wave * 16 + c) * XP + 4 * g;
      // The LDS operands of a pair of column blocks (chain 0: the even block, chain 1: the odd one). A pair's
      // operands are read while the pair before it is multiplied, so that no MFMA waits for its own LDS read.
      struct Pair {
        uint2 xv[2];
        double pv[2][T][4], sv[2][4];
      };
      auto read_pair = [&](int tb0, Pair& o, bool full) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int tb = tb0 + u;
          const bool in = full || tb < nb;  // past the width (dp < 64 only): zeros
          o.xv[u] = in ? *reinterpret_cast<const uint2*>(xrow + 16 * tb) : make_uint2(0u, 0u);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int t = 0; t < T; ++t) o.pv[u][t][s] = in ? Ps[psw(16 * t + c, 16 * tb + g + 4 * s)] : 0.0;
            o.sv[u][s] = in ? svs[16 * tb + g + 4 * s] : 0.0;
          }
        }
      };
      auto multiply = [&](const Pair& o) {
        double xs[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          xs[u][0] = bf16hi_to_f64(o.xv[u].x << 16);
          xs[u][1] = bf16hi_to_f64(o.xv[u].x & 0xffff0000u);
          xs[u][2] = bf16hi_to_f64(o.xv[u].y << 16);
          xs[u][3] = bf16hi_to_f64(o.xv[u].y & 0xffff0000u);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int t = 0; t < T; ++t)
              z[u][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.pv[u][t][s], xs[u][s], z[u][t], 0, 0, 0);
            qq[u] = fma(xs[u][s] * xs[u][s], o.sv[u][s], qq[u]);
          }
      };
      Pair pa, pb;
      if (DPT > 64 || nb == DPT / 16) {  // dp = DPT
        read_pair(0, pa, true);
#pragma unroll 2
        for (int tb0 = 0; tb0 < DPT / 16; tb0 += 4) {
          read_pair(tb0 + 2, pb, true);
          if constexpr (DPT > 64) __builtin_amdgcn_sched_barrier(0);  // one trip at width 64: the compiler's order
          multiply(pa);
          if (tb0 + 4 < DPT / 16) read_pair(tb0 + 4, pa, true);
          if constexpr (DPT > 64) __builtin_amdgcn_sched_barrier(0);  // one trip at width 64: the compiler's order
          multiply(pb);
        }
      } else {  // one or two column blocks
        read_pair(0, pa, false);
        multiply(pa);
      }
#pragma unroll
      for (int i = 0; i < NI; ++i) cur[i] = z[0][i >> 2][i & 3] + z[1][i >> 2][i & 3];
      q = qq[0] + qq[1];
    }
    // s = b + linear + 1/2 (sum_u t_u^2 - sum_i x_i^2 sv_i): this lane group's units and columns, then the four groups
    double s;
    {
      double sq = 0.0, lin = 0.0;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        sq += unit_of[i] < f ? cur[i] * cur[i] : 0.0;
        lin += unit_of[i] == f ? cur[i] : 0.0;
      }
      double h = lin + 0.5 * (sq - q);
      s = bias + lane_groups_sum(h);
    }

    if (!fit) {
      if (valid && g == 0) sout[ri] = s;
      __syncthreads();  // the row tile is free for the next tile
      continue;
    }

    // ---- loss and residual
    double r, l;
    if (logistic) {
      const double e = exp(-fabs(s));
      const double inv = 1.0 / (1.0 + e);
      r = (s >= 0.0 ? inv : e * inv) - yv;
      l = (fmax(s, 0.0) + log1p(e)) - yv * s;
    } else {
      r = s - yv;
      l = 0.5 * r * r;
    }
    r = valid ? r : 0.0;
    if (g == 0) {
      dbacc += r;
      lossacc += valid ? l : 0.0;
    }

    // ---- D^T = [r t_u ; r ; 0 ..] of the tile, then the blocks of dP and u
#pragma unroll
    for (int i = 0; i < NI; ++i)
      DS[unit_of[i] * SP + wave * 16 + c] = unit_of[i] < f ? r * cur[i] : (unit_of[i] == f ? r : 0.0);
    __syncthreads();
    {
      // A wave's blocks share their unit tile (4 % T == 0), so the A operands and r are read once per tile; the
      // rows of a block are read while the block before it is multiplied.
      const int tw = wave % T;
      double da[16], dr[16];
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) {
        da[s4] = DS[(16 * tw + c) * SP + g + 4 * s4];
        dr[s4] = DS[f * SP + g + 4 * s4];
      }
      const u16* xb = Xs + g * XP + 4 * (c & 3) + (c >> 2);
      unsigned xq[2][16];
      auto read_rows = [&](int slot, unsigned (&o)[16]) {
        const int tb = (4 * slot + wave) / T;
        if (tb < nb) {
#pragma unroll
          for (int s4 = 0; s4 < 16; ++s4) o[s4] = xb[16 * tb + 4 * s4 * XP];
        }
      };
      read_rows(0, xq[0]);
#pragma unroll
      for (int slot = 0; slot < NBW; ++slot) {
        if (slot + 1 < NBW) read_rows(slot + 1, xq[(slot + 1) & 1]);
        if constexpr (NBW > 1) __builtin_amdgcn_sched_barrier(0);
        if ((4 * slot + wave) / T < nb) {
#pragma unroll
          for (int s4 = 0; s4 < 16; ++s4) {
            const double xv = bf16hi_to_f64(xq[slot & 1][s4] << 16);
            gp[slot] = __builtin_amdgcn_mfma_f64_16x16x4f64(da[s4], xv, gp[slot], 0, 0, 0);
            if (tw == 0) uacc[slot] = fma(dr[s4], xv * xv, uacc[slot]);
          }
        }
        if constexpr (NBW > 1) __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();  // the staging buffer and the row tile are free
  }

  if (fit) {
    double* pp = part + (long long)blockIdx.x * fm_part_len(dp, T);
    double* pu = pp + (long long)HP * dp;
#pragma unroll
    for (int slot = 0; slot < NBW; ++slot) {
      const int qb = 4 * slot + wave, t = qb % T, tb = qb / T;
      if (tb < nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) pp[(long long)(16 * t + g + 4 * r) * dp + 16 * tb + c] = gp[slot][r];
        if (t == 0) {
          const double v = lane_groups_sum(uacc[slot]);
          if (g == 0) pu[16 * tb + c] = v;
        }
      }
    }
    {
      double v = dbacc, w = lossacc;  // zero outside lane group 0
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        v += __shfl_xor(v, o, 16);
        w += __shfl_xor(w, o, 16);
      }
      if (lane == 0) {
        red[2 * wave] = v;
        red[2 * wave + 1] = w;
      }
    }
    __syncthreads();
    if (tid < 2) pu[dp + tid] = ((red[tid] + red[2 + tid]) + red[4 + tid]) + red[6 + tid];
  }
}

// out = [db | dw (d) | dV (d x f, row-major) | loss]: the sum of the partials' entries in workgroup order, and
// dV_iu = sum - V_iu u_i with V from the parameter image.
__global__ __launch_bounds__(256) void fm_fold_kernel(const double* __restrict__ part, int nparts, int hp, int dp, int d,
                                                      int f, const double* __restrict__ wp,
                                                      double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long ps = (long long)hp * dp + dp + 2, ub = (long long)hp * dp;
  const long long nv = (long long)d * f;
  long long src, usrc = -1;
  if (e == 0) {
    src = ub + dp;
  } else if (e <= d) {
    src = (long long)f * dp + (e - 1);
  } else if (e <= d + nv) {
    const long long i = (e - 1 - d) / f, u = (e - 1 - d) % f;
    src = u * dp + i;
    usrc = ub + i;
  } else if (e == d + nv + 1) {
    src = ub + dp + 1;
  } else {
    return;
  }
  double s = 0.0, us = 0.0;
  for (int b = 0; b < nparts; ++b) s += part[(long long)b * ps + src];
  if (usrc >= 0) {
    for (int b = 0; b < nparts; ++b) us += part[(long long)b * ps + usrc];
    s -= wp[src] * us;
  }
  out[e] = s;
}

template <int DPT, int T>
int fm_launch(int grid, hipStream_t st, const void* X, long long n, int dp, int d, int f, const long long* rows,
              long long B, const double* y, const double* wp, double* part, double* out, int fit, int logistic) {
  if constexpr (!fm_supported(DPT, T)) {
    return (int)hipErrorInvalidValue;
  } else {
    return cml_launch_lds(fm_pass_kernel<DPT, T>, grid, kFmThreads, fm_lds_bytes(DPT, T), st, (const u16*)X, n, dp, d, f,
                          rows, B, y, wp, part, out, fit, logistic);
  }
}

template <int DPT, typename... Args>
int fm_launch_shape(int t, Args... a) {
  if (t == 1) return fm_launch<DPT, 1>(a...);
  if (t == 2) return fm_launch<DPT, 2>(a...);
  return (int)hipErrorInvalidValue;
}

__host__ constexpr int fm_tiles_of(int f) { return f <= 15 ? 1 : 2; }

}  // namespace

// LDS bytes of K32 at this padded width and factor size; 0 = outside the limits.
CML_API long long cml_fm_lds(int dp, int f) {
  if (f < 1 || f > 31) return 0;
  const int t = fm_tiles_of(f);
  return fm_supported(dp, t) ? fm_lds_bytes(fm_dpt(dp), t) : 0;
}

// Workgroups of a launch over B rows: a function of (B, CUs) only for a supported shape, one per CU. 0 = unsupported
// or no row.
CML_API int cml_fm_grid(long long B, int dp, int f, int ncu) {
  if (cml_fm_lds(dp, f) == 0 || B <= 0) return 0;
  return (int)cml_grid_cap((B + kFmTile - 1) / kFmTile, ncu, 1);
}

// X: bf16 [n, dp] contiguous; rows: i64 [B] (indices into X; one outside [0, n) counts as no row) or null for the
// first B rows; y: f64 [n], indexed by the row of X (fit form); wp: f64 [HP dp + 1] with HP = 16 (f <= 15) or 32:
// rows 0 .. f - 1 = V^T, row f = w, zero padded, then b. fit != 0: part f64 [grid][HP dp + dp + 2] scratch and out f64
// [2 + d + d f] = [db | dw | dV | loss]; logistic selects the loss. fit == 0: rows must be null, out f64 [B] = s.
CML_API int cml_fm_pass(const void* X, long long n, int dp, int d, int f, const long long* rows, long long B,
                        const double* y, const double* wp, double* part, int grid, double* out, int fit, int logistic,
                        int ncu, void* stream) {
  if (cml_fm_lds(dp, f) == 0 || d < 1 || d > dp || n < 0 || B <= 0 || (rows == nullptr && B > n) || wp == nullptr ||
      out == nullptr || X == nullptr || (reinterpret_cast<size_t>(X) & 15) != 0 || grid != cml_fm_grid(B, dp, f, ncu) ||
      (fit ? (part == nullptr || y == nullptr) : rows != nullptr))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int t = fm_tiles_of(f);
  int rc = (int)hipErrorInvalidValue;
  switch (fm_dpt(dp)) {
    case 64: rc = fm_launch_shape<64>(t, grid, st, X, n, dp, d, f, rows, B, y, wp, part, out, fit, logistic); break;
    case 128: rc = fm_launch_shape<128>(t, grid, st, X, n, dp, d, f, rows, B, y, wp, part, out, fit, logistic); break;
    case 256: rc = fm_launch_shape<256>(t, grid, st, X, n, dp, d, f, rows, B, y, wp, part, out, fit, logistic); break;
    case 512: rc = fm_launch_shape<512>(t, grid, st, X, n, dp, d, f, rows, B, y, wp, part, out, fit, logistic); break;
  }
  if (rc != 0 || !fit) return rc;
  const long long ne = 2 + d + (long long)d * f;
  return cml_launch_fold(fm_fold_kernel, ne, st, part, grid, 16 * t, dp, d, f, wp, out);
}
