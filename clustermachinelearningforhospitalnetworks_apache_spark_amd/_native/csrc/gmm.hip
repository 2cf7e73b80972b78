// K28: the E-step of a full-covariance Gaussian mixture on bf16 rows (gfx950), and the mixture model's transform.
//
// With A_j = L_j^-1 (L_j the Cholesky factor of component j's covariance) a row's log density under component j
// is lp_j = c_j - |A_j (x - mu_j)|^2 / 2; its responsibility is r_j = w exp(lp_j - lse) with lse the
// log-sum-exp over the components, and the M-step needs, per component, S0 = sum r, S1 = sum r x and
// S2 = sum r x x^T. Both the Mahalanobis terms and the second moments are small GEMMs and run on
// v_mfma_f64_16x16x4_f64 (operand layout: mfma64.h). Every value after the exact bf16 -> f64 widening is f64.
//
// A workgroup of 512 threads (8 waves) keeps the tables [A_j^T | mu | c] in LDS for the whole launch and walks a
// contiguous run of row tiles (TR = 2048 / DP rows: 128 at DP = 16, 64 at DP = 32). Per tile:
//   store    the prefetched rows are widened into the LDS row tile, pad columns (col >= d) and rows past n as 0
//   phase 1  item (16-row group g, component j) -> wave item mod 8: Z = (X_g - mu_j) A_j^T with the rows as the
//            A operand and A_j^T from LDS as B; at DP = 32 the zero upper block of A_j (columns 16.. of rows
//            ..15) is skipped. |z|^2 is a 16-lane sum; lp goes to the LDS tile R [TR][k].
//   lse      512 / TR lanes per row: max, log-sum-exp, r = w exp(lp - lse) back into R (predict: prob and the
//            label, the lowest index among the maxima, to global memory); w lse and w stay in registers.
//   phase 2  component j belongs to wave j mod 8 for the whole launch and keeps S2_j as 16x16 accumulator tiles
//            (1 at DP = 16; the 3 lower ones at DP = 32): S2 += (r_j o X)^T X, 4 rows of depth per MFMA. S1 and
//            S0 are VALU sums of the same A operand.
// At the end every workgroup writes its partial [k][1 + d + d*d] (the lower triangle of S2 mirrored, so S2 is
// symmetric bit for bit) and its two tail sums; gmm_fold_kernel adds the partials in workgroup order. No
// atomics, nothing of size n x k or n x d in global memory, and the grid depends on (n, DP, k, CUs) only.
#include "mfma64.h"

namespace {

constexpr int kGmThreads = 512;
constexpr int kGmWaves = 8;

__host__ __device__ constexpr int gm_rp(int k) { return k | 1; }  // odd f64 pitch of R: rows on distinct banks

// LDS doubles: tables k DP DP + k DP + k, row tile TR (DP + 1), R TR rp, weights TR.
__host__ __device__ constexpr long long gm_lds_doubles(int dp, int k) {
  const int tr = 2048 / dp;
  return (long long)k * dp * dp + (long long)k * dp + k + (long long)tr * (dp + 1) + (long long)tr * gm_rp(k) + tr;
}

template <int DP, bool PREDICT>
__global__ __launch_bounds__(kGmThreads) void gmm_estep_kernel(const u16* __restrict__ X, long long n, int d, int k,
                                                               const double* __restrict__ wts,
                                                               const double* __restrict__ tab,
                                                               double* __restrict__ part,
                                                               double* __restrict__ prob, int* __restrict__ label) {
  constexpr int TR = 2048 / DP;       // rows per tile: 4 values per thread
  constexpr int XP = DP + 1;          // f64 pitch of the row tile
  constexpr int NG = TR / 16;         // 16-row groups per tile
  constexpr int SUB = kGmThreads / TR;  // lanes per row in the lse step
  constexpr int CB = DP / 16;
  constexpr int MAXC = DP == 16 ? 4 : 2;  // components per wave at the limits (k <= 32 / 16)
  constexpr int NT = DP == 16 ? 1 : 3;    // lower 16x16 tiles of S2
  extern __shared__ __align__(16) unsigned char gm_smem[];
  double* Bt = reinterpret_cast<double*>(gm_smem);  // [k][CB][DP][16]: Bt[j][cb][t][c] = A_j[16 cb + c][t]
  double* mu = Bt + (long long)k * DP * DP;          // [k][DP]
  double* cc = mu + k * DP;                          // [k]
  double* Xs = cc + k;                               // [TR][XP]
  const int RP = gm_rp(k);
  double* R = Xs + TR * XP;                          // [TR][RP]
  double* wl = R + TR * RP;                          // [TR]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, kq = lane >> 4;

  const int ntab = k * DP * DP + k * DP + k;
  for (int i = tid; i < ntab; i += kGmThreads) Bt[i] = tab[i];

  const long long ntiles = (n + TR - 1) / TR;
  long long t0, t1;
  tile_run(ntiles, t0, t1);
  const int lrow = (4 * tid) / DP, lcol = (4 * tid) % DP;

  uint2 xq = make_uint2(0u, 0u);
  double wq = 0.0;
  auto load = [&](long long tile) {
    const long long row = tile * TR + lrow;
    xq = row < n ? *reinterpret_cast<const uint2*>(X + row * DP + lcol) : make_uint2(0u, 0u);
    if (tid < TR) {
      const long long wr = tile * TR + tid;
      wq = wr < n ? (wts ? wts[wr] : 1.0) : 0.0;
    }
  };

  f64x4 S2[MAXC][NT];
  double s1[MAXC][CB], s0[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
#pragma unroll
    for (int t = 0; t < NT; ++t) S2[c][t] = (f64x4)0.0;
#pragma unroll
    for (int b = 0; b < CB; ++b) s1[c][b] = 0.0;
    s0[c] = 0.0;
  }
  double tl = 0.0, tw = 0.0;

  if (t0 < t1) load(t0);
  for (long long tile = t0; tile < t1; ++tile) {
    // ---- store: widen the prefetched values; the pad columns are masked by d, not trusted
    {
      const unsigned wv[2] = {xq.x, xq.y};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double v = bf16hi_to_f64((e & 1) ? (wv[e >> 1] & 0xffff0000u) : (wv[e >> 1] << 16));
        Xs[lrow * XP + lcol + e] = lcol + e < d ? v : 0.0;
      }
      if (tid < TR) wl[tid] = wq;
    }
    __syncthreads();
    if (tile + 1 < t1) load(tile + 1);

    // ---- phase 1: lp[row][j] = c_j - |A_j (x - mu_j)|^2 / 2
    for (int item = wave; item < NG * k; item += kGmWaves) {
      const int g = item % NG, j = item / NG;
      const double* xs = Xs + (g * 16 + r16) * XP;
      const double* mj = mu + j * DP;
      const double* bt = Bt + (long long)j * DP * DP + r16;
      f64x4 D[CB];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) D[cb] = (f64x4)0.0;
#pragma unroll
      for (int s = 0; s < DP / 4; ++s) {
        const int t = 4 * s + kq;
        const double a = xs[t] - mj[t];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          if (4 * s < 16 * (cb + 1))  // A_j is lower triangular: columns past the block's last row are zero
            D[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bt[(cb * DP + t) * 16], D[cb], 0, 0, 0);
        }
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        double q = 0.0;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) q += D[cb][reg] * D[cb][reg];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) q += __shfl_xor(q, o, 16);
        if (r16 == 0) R[(g * 16 + kq + 4 * reg) * RP + j] = cc[j] - 0.5 * q;
      }
    }
    __syncthreads();

    // ---- lse: SUB adjacent lanes per row
    {
      const int row = tid / SUB, sub = tid % SUB;
      const long long grow = tile * TR + row;
      double* rr = R + row * RP;
      double m = -__builtin_huge_val();
      int am = 0x7fffffff;
      for (int j = sub; j < k; j += SUB) {
        const double v = rr[j];
        if (v > m) {
          m = v;
          am = j;
        }
      }
#pragma unroll
      for (int o = SUB / 2; o > 0; o >>= 1) {
        const double om = __shfl_xor(m, o, SUB);
        const int oa = __shfl_xor(am, o, SUB);
        if (om > m || (om == m && oa < am)) {
          m = om;
          am = oa;
        }
      }
      double se = 0.0;
      for (int j = sub; j < k; j += SUB) se += exp(rr[j] - m);
#pragma unroll
      for (int o = SUB / 2; o > 0; o >>= 1) se += __shfl_xor(se, o, SUB);
      const double lse = m + log(se);
      const double w = wl[row];
      for (int j = sub; j < k; j += SUB) {
        const double p = exp(rr[j] - lse);
        if constexpr (PREDICT) {
          if (grow < n) prob[grow * k + j] = p;
        } else {
          rr[j] = w * p;
        }
      }
      if (sub == 0) {
        if constexpr (PREDICT) {
          if (grow < n) label[grow] = am < k ? am : 0;
        } else {
          tl += w * lse;
          tw += w;
        }
      }
    }
    __syncthreads();

    // ---- phase 2: S2_j += (r_j o X)^T X, S1_j += r_j^T X, S0_j += sum r_j
    if constexpr (!PREDICT) {
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        const int j = wave + kGmWaves * c;
        if (j < k) {
#pragma unroll 4
          for (int s = 0; s < TR / 4; ++s) {
            const int i = 4 * s + kq;
            const double r = R[i * RP + j];
            const double* xi = Xs + i * XP + r16;
            const double x0 = xi[0], a0 = r * x0;
            S2[c][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, x0, S2[c][0], 0, 0, 0);
            s1[c][0] += a0;
            s0[c] += r;
            if constexpr (DP == 32) {
              const double x1 = xi[16], a1 = r * x1;
              S2[c][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, x0, S2[c][1], 0, 0, 0);
              S2[c][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, x1, S2[c][2], 0, 0, 0);
              s1[c][1] += a1;
            }
          }
        }
      }
      __syncthreads();
    }
  }

  if constexpr (!PREDICT) {
    const long long cs = 1 + d + (long long)d * d;
    double* pp = part + (long long)blockIdx.x * (cs * k + 2);
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int j = wave + kGmWaves * c;
      if (j < k) {
        double* out = pp + cs * j;
        const double v = lane_groups_sum(s0[c]);
        if (lane == 0) out[0] = v;
#pragma unroll
        for (int b = 0; b < CB; ++b) {
          const double u = lane_groups_sum(s1[c][b]);
          if (kq == 0 && 16 * b + r16 < d) out[1 + 16 * b + r16] = u;
        }
        double* o2 = out + 1 + d;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int ab = t == 0 ? 0 : 1, bb = t == 2 ? 1 : 0;
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int a = 16 * ab + kq + 4 * reg, b = 16 * bb + r16;
            if (a < d && b < d && a >= b) {  // one triangle, mirrored
              const double u = S2[c][t][reg];
              o2[a * d + b] = u;
              o2[b * d + a] = u;
            }
          }
        }
      }
    }
    // the tail sums, added in thread order (the last tile's barrier has released the row tile)
    double* red = Xs;  // 2 * 512 doubles <= TR * XP
    red[tid] = tl;
    red[kGmThreads + tid] = tw;
    __syncthreads();
    if (tid < 2) {
      double s = 0.0;
      for (int i = 0; i < kGmThreads; ++i) s += red[tid * kGmThreads + i];
      pp[cs * k + tid] = s;
    }
  }
}

__global__ __launch_bounds__(256) void gmm_fold_kernel(const double* __restrict__ part, int nparts, long long ps,
                                                       double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= ps) return;
  double s = 0.0;
  for (int b = 0; b < nparts; ++b) s += part[(long long)b * ps + e];
  out[e] = s;
}

bool gm_args_ok(const void* X, long long n, int dp, int d, int k) {
  if (dp != 16 && dp != 32) return false;
  if (d < 1 || d > dp || k < 2 || k > (dp == 16 ? 32 : 16) || n < 0) return false;
  return (reinterpret_cast<size_t>(X) & 7) == 0;  // the 8-byte row loads
}

template <int DP, bool PREDICT>
int gm_launch(int grid, long long lds, hipStream_t st, const void* X, long long n, int d, int k, const double* wts,
              const double* tab, double* part, double* prob, int* label) {
  return cml_launch_lds(gmm_estep_kernel<DP, PREDICT>, grid, kGmThreads, lds, st, (const u16*)X, n, d, k, wts, tab, part,
                        prob, label);
}

template <bool PREDICT>
int gm_launch_dp(int dp, int grid, long long lds, hipStream_t st, const void* X, long long n, int d, int k,
                 const double* wts, const double* tab, double* part, double* prob, int* label) {
  return dp == 16 ? gm_launch<16, PREDICT>(grid, lds, st, X, n, d, k, wts, tab, part, prob, label)
                  : gm_launch<32, PREDICT>(grid, lds, st, X, n, d, k, wts, tab, part, prob, label);
}

}  // namespace

// LDS bytes of K28 at this padded width and k; 0 = outside the kernel's limits.
CML_API long long cml_gmm_lds(int dp, int k) {
  if ((dp != 16 && dp != 32) || k < 2 || k > (dp == 16 ? 32 : 16)) return 0;
  const long long lds = gm_lds_doubles(dp, k) * 8;
  return lds <= kLdsPerCu ? lds : 0;
}

// Workgroups of a launch: a function of (n, dp, k, CUs) only. 0 = unsupported or no rows. The fit form's
// registers (S2 accumulators) leave room for one workgroup per CU; the predict form fits two where the LDS does.
CML_API int cml_gmm_grid(long long n, int dp, int k, int ncu, int predict) {
  const long long lds = cml_gmm_lds(dp, k);
  if (lds == 0 || n <= 0) return 0;
  const long long tr = 2048 / dp;
  return (int)cml_grid_cap((n + tr - 1) / tr, ncu, predict && lds <= kLdsPerCu / 2 ? 2 : 1);
}

// X: bf16 [n, dp] contiguous; wts f64 [n] or null; tab f64 [k dp dp | k dp | k] (A_j^T in 16-column blocks, mu
// zero padded, c); part f64 [grid][k (1 + d + d d) + 2] scratch; out f64 [k (1 + d + d d) + 2]: stats, then tail.
CML_API int cml_gmm_estep(const void* X, long long n, int dp, int d, int k, const double* wts, const double* tab,
                          double* part, int grid, double* out, int ncu, void* stream) {
  if (!gm_args_ok(X, n, dp, d, k) || n == 0 || grid != cml_gmm_grid(n, dp, k, ncu, 0)) return (int)hipErrorInvalidValue;
  const long long lds = cml_gmm_lds(dp, k);
  const long long ps = (long long)k * (1 + d + (long long)d * d) + 2;
  hipStream_t st = (hipStream_t)stream;
  const int rc = gm_launch_dp<false>(dp, grid, lds, st, X, n, d, k, wts, tab, part, nullptr, nullptr);
  if (rc != 0) return rc;
  return cml_launch_fold(gmm_fold_kernel, ps, st, part, grid, ps, out);
}

// prob f64 [n, k], label i32 [n].
CML_API int cml_gmm_predict(const void* X, long long n, int dp, int d, int k, const double* tab, double* prob,
                            int* label, int ncu, void* stream) {
  if (!gm_args_ok(X, n, dp, d, k)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const long long lds = cml_gmm_lds(dp, k);
  const int grid = cml_gmm_grid(n, dp, k, ncu, 1);
  hipStream_t st = (hipStream_t)stream;
  return gm_launch_dp<true>(dp, grid, lds, st, X, n, d, k, nullptr, tab, nullptr, prob, label);
}
