// K30: loss and gradient (and the forward pass) of the multilayer perceptron classifier on bf16 rows (gfx950).
//
// layers = [d, h_1, .., C] with NL = 2 or 3 weight layers. Per row x with label y, all f64 after the exact
// bf16 -> f64 widening:
//   a_0 = x,  z_l = W_l a_{l-1} + b_l,  a_l = 1 / (1 + exp(-z_l)) for l < NL
//   loss = logsumexp(z_NL) - z_NL[y]  (the row maximum subtracted inside),  delta_NL = softmax(z_NL) - onehot(y)
//   delta_l = (W_{l+1}^T delta_{l+1}) a_l (1 - a_l),  dW_l = sum_rows delta_l a_{l-1}^T,  db_l = sum_rows delta_l
// The sums are not divided by n. The forward-only form (fit = 0) writes z_NL [n, C] and nothing else.
//
// Every non-input layer is padded with zero weights and biases to HP = 16 T units (T = 1 or 2, one value for the
// whole network). A persistent workgroup of 256 threads (4 waves, one per SIMD) keeps every layer in LDS as f64
// for the whole launch and walks a contiguous run of 64-row tiles. Per tile:
//   stage     the rows go to LDS as bf16, once; pad columns (>= d) and rows past n are stored as 0. Inside a
//             16-column block position 4 g + r holds column g + 4 r, so that lane group g reads its four values
//             with one 8-byte load (K29's order). The global loads of a tile are issued one tile ahead and wait
//             in registers while the previous tile is computed.
//   forward   a wave owns 16 rows, row = lane & 15, lane group g = lane >> 4, transposed on
//             v_mfma_f64_16x16x4_f64 (operand layout: mfma64.h): Z^T[unit][row] = W[unit][k] A^T[k][row].
//             Accumulator register r of unit tile
//             t holds unit 16 t + g + 4 r, which is the B operand of K-step (t, r) of the next layer. Sigmoid, exp
//             and log are f64 VALU; the softmax sums over a row's classes are sums over the four lane groups; pad
//             classes are left out of it; rows past n get delta = 0 and no loss.
//   backward  delta_l^T = W_{l+1}^T delta_{l+1}^T the same way, from a transposed LDS copy of W_{l+1}.
//   gradients from the last layer to the first: delta_l^T and a_{l-1}^T of the tile go to the staging buffers
//             [unit][row], and after a barrier the wave that owns a 16 x 16 block of dW_l for the whole launch adds
//             sum_rows delta_l[unit][row] a_{l-1}[j][row] to its accumulator registers, 4 rows of depth per MFMA;
//             layer 1 takes the staged bf16 rows as its B operand. Block (t, tb) of dW_1 belongs to wave
//             (tb T + t) & 3; the T^2 blocks of an upper layer to waves 0 .. T^2 - 1.
// At the end a workgroup writes its partial [dW | db | loss] in the padded layout; mlp_fold_kernel adds the
// partials in workgroup order into Spark's flat layout (per layer W out x in column-major, then b). No atomics,
// nothing of size n in global memory, the grid depends on (n, CUs) only, every loop is bounded by n.
//
// LDS reads of a half wave fall on 32 distinct doubles mod 32: the W_1 image [HP][DPT] uses K29's XOR of the
// column index with f(unit) = 2 (unit & 15) ^ 16 (unit & 1) (lanes along units with lane groups along columns is
// the only pattern it is read in; the swizzle also serves lanes along columns); the upper layers have pitch
// HP + 2 (2 c + g), in both orientations; the staging buffers have pitch 66 (2 c + g).
#include "mfma64.h"

namespace {

constexpr int kMlThreads = 256;
constexpr int kMlTile = 64;   // rows per tile: 16 per wave
constexpr int kMlSP = 66;     // f64 pitch of a staging row (64 rows of a tile)

__host__ __device__ constexpr int ml_dpt(int dp) { return dp < 64 ? 64 : dp; }  // compiled width class

// LDS bytes: W_1 HP DPT, the upper layers in both orientations 2 (NL - 1) HP (HP + 2), the biases NL HP, the two
// staging buffers 2 HP 66, the fold of db and the loss 4 (NL HP + 1) (all f64), the rows 64 (DPT + 8) bf16.
__host__ __device__ constexpr long long ml_lds_bytes(int dpt, int t, int nl) {
  const int hp = 16 * t;
  return 8LL * ((long long)hp * dpt + 2 * (nl - 1) * hp * (hp + 2) + nl * hp + 2 * hp * kMlSP + 4 * (nl * hp + 1)) +
         2LL * kMlTile * (dpt + 8);
}

__host__ __device__ constexpr bool ml_supported(int dp, int t, int nl) {
  if (dp < 16 || dp > 512 || (dp & (dp - 1)) != 0 || t < 1 || t > 2 || nl < 2 || nl > 3) return false;
  return ml_lds_bytes(ml_dpt(dp), t, nl) <= kLdsPerCu;
}

__host__ __device__ constexpr long long ml_part_len(int dp, int t, int nl) {
  const int hp = 16 * t;
  return (long long)hp * dp + (nl - 1) * hp * hp + nl * hp + 1;
}

template <int DPT, int T, int NL>
__global__ __launch_bounds__(kMlThreads, 1) void mlp_pass_kernel(
    const u16* __restrict__ X, long long n, int dp, int d, int C, const int* __restrict__ y,
    const double* __restrict__ wp, double* __restrict__ part, double* __restrict__ zout, int fit) {
  constexpr int HP = 16 * T;
  constexpr int NI = 4 * T;             // units per lane: index i <-> unit 16 (i >> 2) + g + 4 (i & 3)
  constexpr int BP = DPT;
  constexpr int WP = HP + 2;
  constexpr int SP = kMlSP;
  constexpr int XP = DPT + 8;           // bf16 pitch of a staged row (K29's: pitch / 4 = 2 mod 4 doubles)
  constexpr int NBW = (T * (DPT / 16) + 3) / 4;  // blocks of dW_1 per wave
  constexpr int RP = NL * HP + 1;
  constexpr int NIT = DPT / 64;         // 16-column blocks of a tile per thread
  extern __shared__ __align__(16) unsigned char ml_smem[];
  double* W1s = reinterpret_cast<double*>(ml_smem);   // [HP][BP], column index swizzled by the unit
  double* Wu = W1s + HP * BP;                         // [NL - 1][HP out][WP]
  double* WuT = Wu + (NL - 1) * HP * WP;              // [NL - 1][HP in][WP]
  double* bs = WuT + (NL - 1) * HP * WP;              // [NL][HP]
  double* DS = bs + NL * HP;                          // [HP][SP]: delta_l^T of the tile
  double* AS = DS + HP * SP;                          // [HP][SP]: a_{l-1}^T of the tile
  double* red = AS + HP * SP;                         // [4][RP]
  u16* Xs = reinterpret_cast<u16*>(red + 4 * RP);     // [64][XP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int nb = dp >> 4;               // 16-column blocks of a row

  auto wsw = [](int unit, int col) { return unit * BP + unit_swizzle(unit, col); };

  for (int i = tid; i < HP * dp; i += kMlThreads) W1s[wsw(i / dp, i % dp)] = wp[i];
  const double* wu_g = wp + (long long)HP * dp;
  for (int i = tid; i < (NL - 1) * HP * HP; i += kMlThreads) {
    const int l = i / (HP * HP), o = (i / HP) % HP, k = i % HP;
    const double v = wu_g[i];
    Wu[(l * HP + o) * WP + k] = v;
    WuT[(l * HP + k) * WP + o] = v;
  }
  for (int i = tid; i < NL * HP; i += kMlThreads) bs[i] = wu_g[(NL - 1) * HP * HP + i];

  int unit_of[NI];
  bool real[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    unit_of[i] = unit_of_lane(i, g);
    real[i] = unit_of[i] < C;
  }

  f64x4 g1[NBW];
#pragma unroll
  for (int s = 0; s < NBW; ++s) g1[s] = (f64x4)0.0;
  f64x4 gu[NL - 1];
#pragma unroll
  for (int l = 0; l < NL - 1; ++l) gu[l] = (f64x4)0.0;
  double dbacc[NL][NI];
#pragma unroll
  for (int l = 0; l < NL; ++l)
#pragma unroll
    for (int i = 0; i < NI; ++i) dbacc[l][i] = 0.0;
  double lossacc = 0.0;

  const long long ntiles = (n + kMlTile - 1) / kMlTile;
  long long t0, t1;
  tile_run(ntiles, t0, t1);

  // One item = one 16-column block of one row (32 bytes); a thread holds its NIT items of a tile in registers.
  // The loads of tile + 1 are issued before the products of tile, so that no tile waits for HBM.
  uint4 pf[NIT][2];
  const int lnb = __ffs(nb) - 1;  // nb is a power of two
  auto fetch = [&](long long tile) {
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const int item = tid + kMlThreads * j;
      const long long ri = tile * kMlTile + (item >> lnb);
      pf[j][0] = make_uint4(0u, 0u, 0u, 0u);
      pf[j][1] = pf[j][0];
      if (item < kMlTile * nb && ri < n) {
        const uint4* p = reinterpret_cast<const uint4*>(X + ri * dp + 16 * (item & (nb - 1)));
        pf[j][0] = p[0];
        pf[j][1] = p[1];
      }
    }
  };
  fetch(t0);

  for (long long tile = t0; tile < t1; ++tile) {
    const long long base = tile * kMlTile;
    // ---- stage the fetched tile
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const int item = tid + kMlThreads * j;
      if (item < kMlTile * nb) {
        const int row = item >> lnb, tb = item & (nb - 1);
        // the same block as in lda.hip and fm.hip: as a shared function it compiles to other machine code
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
    __syncthreads();  // also orders the weight stores before the first tile's reads

    // ---- forward: this wave's 16 rows
    const long long ri = base + wave * 16 + c;
    const bool valid = ri < n;
    const int yv = fit && valid ? y[ri] : -1;
    if (tile + 1 < t1) fetch(tile + 1);
    double act[NL - 1][NI], cur[NI];
    {
      f64x4 z[2][T];  // two chains of column blocks
#pragma unroll
      for (int t = 0; t < T; ++t) {
        z[1][t] = (f64x4)0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) z[0][t][r] = bs[16 * t + g + 4 * r];
      }
      const u16* xrow = Xs + (wave * 16 + c) * XP + 4 * g;
      auto block = [&](int tb, int u) {
        const uint2 xv = *reinterpret_cast<const uint2*>(xrow + 16 * tb);
        const double xs[4] = {bf16hi_to_f64(xv.x << 16), bf16hi_to_f64(xv.x & 0xffff0000u), bf16hi_to_f64(xv.y << 16),
                              bf16hi_to_f64(xv.y & 0xffff0000u)};
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int t = 0; t < T; ++t)
            z[u][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(W1s[wsw(16 * t + c, 16 * tb + g + 4 * s)], xs[s], z[u][t],
                                                           0, 0, 0);
      };
      if (DPT > 64 || nb == DPT / 16) {  // dp = DPT: up to eight column blocks per trip, their LDS reads ahead
#pragma unroll 4
        for (int tb0 = 0; tb0 < DPT / 16; tb0 += 2) {
          block(tb0, 0);
          block(tb0 + 1, 1);
        }
      } else {
#pragma unroll 1
        for (int tb0 = 0; tb0 < nb; tb0 += 2) {
          block(tb0, 0);
          if (tb0 + 1 < nb) block(tb0 + 1, 1);
        }
      }
#pragma unroll
      for (int i = 0; i < NI; ++i) cur[i] = z[0][i >> 2][i & 3] + z[1][i >> 2][i & 3];
    }
#pragma unroll
    for (int l = 1; l < NL; ++l) {
      f64x4 acc[T];
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = bs[l * HP + 16 * t + g + 4 * r];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        act[l - 1][i] = 1.0 / (1.0 + exp(-cur[i]));
#pragma unroll
        for (int t = 0; t < T; ++t)
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Wu[((l - 1) * HP + 16 * t + c) * WP + unit_of[i]],
                                                        act[l - 1][i], acc[t], 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < NI; ++i) cur[i] = acc[i >> 2][i & 3];
    }

    if (!fit) {
      if (valid) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
          if (real[i]) zout[ri * C + unit_of[i]] = cur[i];
      }
      __syncthreads();  // the row tile is free for the next tile
      continue;
    }

    // ---- softmax, loss and delta of the last layer
    double dl[NL][NI];
    {
      double m = -INFINITY;
#pragma unroll
      for (int i = 0; i < NI; ++i) m = real[i] ? fmax(m, cur[i]) : m;
      m = fmax(m, __shfl_xor(m, 16, 64));
      m = fmax(m, __shfl_xor(m, 32, 64));
      double e[NI], s = 0.0, zy = 0.0;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        e[i] = real[i] ? exp(cur[i] - m) : 0.0;
        s += e[i];
        zy += unit_of[i] == yv ? cur[i] : 0.0;
      }
      s = lane_groups_sum(s);
      zy = lane_groups_sum(zy);
      const double inv = 1.0 / s;
#pragma unroll
      for (int i = 0; i < NI; ++i)
        dl[NL - 1][i] = valid && real[i] ? e[i] * inv - (unit_of[i] == yv ? 1.0 : 0.0) : 0.0;
      lossacc += valid && g == 0 ? (m + log(s)) - zy : 0.0;
    }
    // ---- backward: delta of the hidden layers
#pragma unroll
    for (int l = NL - 1; l >= 1; --l) {
      f64x4 acc[T];
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] = (f64x4)0.0;
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int t = 0; t < T; ++t)
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(WuT[((l - 1) * HP + 16 * t + c) * WP + unit_of[i]], dl[l][i],
                                                        acc[t], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const double a = act[l - 1][i];
        dl[l - 1][i] = valid ? acc[i >> 2][i & 3] * (a * (1.0 - a)) : 0.0;
      }
    }
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
      for (int i = 0; i < NI; ++i) dbacc[l][i] += dl[l][i];

    // ---- gradients, from the last layer to the first, through the staging buffers
#pragma unroll
    for (int l = NL - 1; l >= 0; --l) {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        DS[unit_of[i] * SP + wave * 16 + c] = dl[l][i];
        if (l >= 1) AS[unit_of[i] * SP + wave * 16 + c] = act[l >= 1 ? l - 1 : 0][i];
      }
      __syncthreads();
      if (l >= 1) {
        if (wave < T * T) {
          const int to = wave / T, ti = wave % T;
          const double* da = DS + (16 * to + c) * SP + g;
          const double* ab = AS + (16 * ti + c) * SP + g;
#pragma unroll
          for (int s = 0; s < 16; ++s)
            gu[l >= 1 ? l - 1 : 0] =
                __builtin_amdgcn_mfma_f64_16x16x4f64(da[4 * s], ab[4 * s], gu[l >= 1 ? l - 1 : 0], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int slot = 0; slot < NBW; ++slot) {
          const int q = 4 * slot + wave, t = q % T, tb = q / T;
          if (tb < nb) {
            const double* da = DS + (16 * t + c) * SP + g;
            const u16* xb = Xs + g * XP + 16 * tb + 4 * (c & 3) + (c >> 2);
#pragma unroll
            for (int s = 0; s < 16; ++s)
              g1[slot] = __builtin_amdgcn_mfma_f64_16x16x4f64(da[4 * s], bf16hi_to_f64((unsigned)xb[4 * s * XP] << 16),
                                                              g1[slot], 0, 0, 0);
          }
        }
      }
      __syncthreads();  // the staging buffers (and after layer 1 the row tile) are free
    }
  }

  if (fit) {
    double* pp = part + (long long)blockIdx.x * ml_part_len(dp, T, NL);
#pragma unroll
    for (int slot = 0; slot < NBW; ++slot) {
      const int q = 4 * slot + wave, t = q % T, tb = q / T;
      if (tb < nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) pp[(long long)(16 * t + g + 4 * r) * dp + 16 * tb + c] = g1[slot][r];
      }
    }
    double* pu = pp + (long long)HP * dp;
    if (wave < T * T) {
      const int to = wave / T, ti = wave % T;
#pragma unroll
      for (int l = 0; l < NL - 1; ++l)
#pragma unroll
        for (int r = 0; r < 4; ++r) pu[(l * HP + 16 * to + g + 4 * r) * HP + 16 * ti + c] = gu[l][r];
    }
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        double v = dbacc[l][i];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
        if (c == 0) red[wave * RP + l * HP + unit_of[i]] = v;
      }
    {
      double v = lossacc;
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
      if (lane == 0) red[wave * RP + NL * HP] = v;
    }
    __syncthreads();
    if (tid < RP) pu[(NL - 1) * HP * HP + tid] = ((red[tid] + red[RP + tid]) + red[2 * RP + tid]) + red[3 * RP + tid];
  }
}

// out = [grad in Spark's flat layout | loss]: the sum of the partials' entries in workgroup order.
__global__ __launch_bounds__(256) void mlp_fold_kernel(const double* __restrict__ part, int nparts, int hp, int dp,
                                                       int nl, int s0, int s1, int s2, int s3,
                                                       double* __restrict__ out) {
  const int sz[4] = {s0, s1, s2, s3};
  long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long ps = (long long)hp * dp + (long long)(nl - 1) * hp * hp + nl * hp + 1;
  const long long ob = (long long)hp * dp + (long long)(nl - 1) * hp * hp;
  long long src = -1;
  long long r = e;
  for (int l = 0; l < nl; ++l) {
    const long long in = sz[l], o = sz[l + 1];
    if (r < in * o) {
      const long long i = r / o, u = r % o;
      src = l == 0 ? u * dp + i : (long long)hp * dp + ((long long)(l - 1) * hp + u) * hp + i;
      break;
    }
    r -= in * o;
    if (r < o) {
      src = ob + (long long)l * hp + r;
      break;
    }
    r -= o;
  }
  if (src < 0) {
    if (r != 0) return;  // past the loss
    src = ps - 1;
  }
  double s = 0.0;
  for (int b = 0; b < nparts; ++b) s += part[(long long)b * ps + src];
  out[e] = s;
}

template <int DPT, int T, int NL>
int ml_launch(int grid, hipStream_t st, const void* X, long long n, int dp, int d, int C, const int* y,
              const double* wp, double* part, double* zout, int fit) {
  if constexpr (!ml_supported(DPT, T, NL)) {
    return (int)hipErrorInvalidValue;
  } else {
    return cml_launch_lds(mlp_pass_kernel<DPT, T, NL>, grid, kMlThreads, ml_lds_bytes(DPT, T, NL), st, (const u16*)X, n,
                          dp, d, C, y, wp, part, zout, fit);
  }
}

template <int DPT, typename... Args>
int ml_launch_shape(int t, int nl, Args... a) {
  if (t == 1 && nl == 2) return ml_launch<DPT, 1, 2>(a...);
  if (t == 2 && nl == 2) return ml_launch<DPT, 2, 2>(a...);
  if (t == 1 && nl == 3) return ml_launch<DPT, 1, 3>(a...);
  if (t == 2 && nl == 3) return ml_launch<DPT, 2, 3>(a...);
  return (int)hipErrorInvalidValue;
}

__host__ constexpr int ml_tiles_of(int hmax) { return hmax <= 16 ? 1 : 2; }

}  // namespace

// LDS bytes of K30 at this padded width, widest non-input layer and number of weight layers; 0 = outside the limits.
CML_API long long cml_mlp_lds(int dp, int hmax, int nl) {
  if (hmax < 1 || hmax > 32) return 0;
  const int t = ml_tiles_of(hmax);
  return ml_supported(dp, t, nl) ? ml_lds_bytes(ml_dpt(dp), t, nl) : 0;
}

// Workgroups of a launch: a function of (n, CUs) only for a supported shape, one per CU. 0 = unsupported or no row.
CML_API int cml_mlp_grid(long long n, int dp, int hmax, int nl, int ncu) {
  if (cml_mlp_lds(dp, hmax, nl) == 0 || n <= 0) return 0;
  return (int)cml_grid_cap((n + kMlTile - 1) / kMlTile, ncu, 1);
}

// X: bf16 [n, dp] contiguous; layers = [d, s1, s2(, s3)] with nl = 2 or 3 weight layers (s3 = 0 at nl = 2); y: i32 [n]
// in [0, C) (fit form); wp: f64, HP = 16 or 32 by the widest non-input layer: W_1 [HP][dp], W_l [HP out][HP in] for
// l = 2 .. nl, b [nl][HP], all zero padded. fit != 0: part f64 [grid][HP dp + (nl - 1) HP^2 + nl HP + 1] scratch and
// out f64 [P + 1] = the gradient in Spark's flat layout, then the loss. fit == 0: out f64 [n, C] = z of the last layer.
CML_API int cml_mlp_pass(const void* X, long long n, int dp, int d, int nl, int s1, int s2, int s3, const int* y,
                         const double* wp, double* part, int grid, double* out, int fit, int ncu, void* stream) {
  if (nl < 2 || nl > 3 || s1 < 1 || s2 < 1 || (nl == 3 ? s3 < 1 : s3 != 0)) return (int)hipErrorInvalidValue;
  const int hmax = s1 > s2 ? (s1 > s3 ? s1 : s3) : (s2 > s3 ? s2 : s3);
  const int C = nl == 3 ? s3 : s2;
  if (cml_mlp_lds(dp, hmax, nl) == 0 || C < 2 || d < 1 || d > dp || n <= 0 || wp == nullptr || out == nullptr ||
      (reinterpret_cast<size_t>(X) & 15) != 0 || grid != cml_mlp_grid(n, dp, hmax, nl, ncu) ||
      (fit && (part == nullptr || y == nullptr)))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int t = ml_tiles_of(hmax);
  int rc = (int)hipErrorInvalidValue;
  switch (ml_dpt(dp)) {
    case 64: rc = ml_launch_shape<64>(t, nl, grid, st, X, n, dp, d, C, y, wp, part, out, fit); break;
    case 128: rc = ml_launch_shape<128>(t, nl, grid, st, X, n, dp, d, C, y, wp, part, out, fit); break;
    case 256: rc = ml_launch_shape<256>(t, nl, grid, st, X, n, dp, d, C, y, wp, part, out, fit); break;
    case 512: rc = ml_launch_shape<512>(t, nl, grid, st, X, n, dp, d, C, y, wp, part, out, fit); break;
  }
  if (rc != 0 || !fit) return rc;
  long long ne = 1;
  const int sz[4] = {d, s1, s2, s3};
  for (int l = 0; l < nl; ++l) ne += (long long)sz[l] * sz[l + 1] + sz[l + 1];
  return cml_launch_fold(mlp_fold_kernel, ne, st, part, grid, 16 * t, dp, nl, d, s1, s2, s3, out);
}
