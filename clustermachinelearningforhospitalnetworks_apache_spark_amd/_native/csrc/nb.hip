// K34: the per-class moments and the class scores of naive Bayes on bf16 rows of padded width 16 .. 512 (gfx950).
//
// Moments form. With labels l (int32), weights w (f64, 1 without any) and an optional shift table m [C][d] (f64):
//   n_c = sum_{l = c} w,  S1[c][i] = sum_{l = c} w (x_i - m_ci),  S2[c][i] = sum_{l = c} w (x_i - m_ci)^2
// and bad = [# of x_i < 0, # of x_i not in {0, 1}] over the live columns of every row: the hard-assignment case of
// K28's S1 = R^T X. Per 4 rows and 16 columns one v_mfma_f64_16x16x4_f64 (operand layout: mfma64.h) adds A B with
// A[class][k] = (l_k == class) ? w_k : 0 and B[k][col] = x_k,col - m[l_k][col]; S2 is a second MFMA with B squared
// (skipped unless asked for), a second class block (classes 16 .. 31) a further one, skipped when C <= 16. n_c is a
// VALU sum of the A operand, the two bad counts are integer sums taken where the value is widened. A row whose label
// is outside 0 .. C-1 has an all-zero A column (and shift 0); it still counts towards bad.
//
// Scores form. The table [W | b] (gaussian: [theta | iv | b]) stays in LDS as f64 for the launch.
//   linear / complement   s = X W^T + b on the MFMA with the rows as the A operand; W sits in the XOR-swizzled image
//                         of mfma64.h (lanes along classes, lane groups along columns).
//   gaussian              s_c = b_c - 1/2 sum_i (x_i - theta_ci)^2 iv_ci: the centred quadratic, one (row, class) pair
//                         per lane, f64 fma over the columns in ascending order (never the expanded form, which
//                         cancels where |x - theta| << |x|); theta and iv have the odd pitch DP + 1.
//   lse                   512 / TR lanes per row: max, log-sum-exp, raw (complement: s - lse, else s), prob =
//                         exp(s - lse) and pred, the lowest index among the maxima of raw, as f64; each written once.
//
// Both forms: 512 threads (8 waves) walk a contiguous run of row tiles (tile_run), TR = min(256, 8192 / DP) rows
// each. The bf16 rows of a tile are staged once in LDS; columns >= d and rows past n are stored as 0 (they may hold
// NaN bits); the global loads of tile + 1 are issued before the work on tile and wait in registers. In the moments
// form wave v owns the column tiles {ct : ct mod WC == v mod WC}, WC = min(DP / 16, 8), for the whole launch and keeps
// their blocks in accumulator registers; at DP < 128 the 8 / WC waves that share a column tile take disjoint row
// quarters of every tile ("row splits") and write partials of their own. Every workgroup writes its partials;
// nb_fold_kernel adds them in a fixed order, one wave per entry. No atomics, nothing of size n written by the moments
// form, the same bits on every call; the grid is a function of (n, DP, CUs) only.
//
// LDS pitches: moments rows DP + 16 bf16 (the 2 x 16 lanes of a half wave read rows g, g + 1 at 8 dwords each: 16
// distinct banks of 32), scores rows DP + 4 bf16 (16 rows x one dword: 2 r mod 32 distinct).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), no scratch in any
// instantiation. nb_moments_kernel at DP = 512 holds 4 column tiles x 2 class blocks per wave: 191 VGPRs with the
// second moment (128 of them accumulators), 127 without; 123 / 91 at DP = 256 and 66 .. 90 at DP <= 128.
// nb_scores_kernel: 80 .. 96 VGPRs (linear), 84 .. 102 (gaussian). All LDS is dynamic (cml_nb_lds).
//
// Measured times and rates: the K34 row of PARITY.md (scripts/mb_ml.py nb).
#include "mfma64.h"

#pragma clang fp contract(off)

namespace {

constexpr int kNbThreads = 512;
constexpr int kNbWaves = 8;
constexpr int kNbMaxC = 32;

__host__ __device__ constexpr int nb_tr(int dp) { return 8192 / dp < 256 ? 8192 / dp : 256; }
__host__ __device__ constexpr int nb_wc(int dp) { return dp / 16 < kNbWaves ? dp / 16 : kNbWaves; }
__host__ __device__ constexpr int nb_rs(int dp) { return kNbWaves / nb_wc(dp); }  // row splits of a tile
__host__ __device__ constexpr int nb_rp(int C) { return C | 1; }  // odd f64 pitch of the score tile

constexpr bool nb_dp_ok(int dp) { return dp == 16 || dp == 32 || dp == 64 || dp == 128 || dp == 256 || dp == 512; }

// LDS bytes of the moments form: the row tile, the weights, the labels and, with a shift, its table.
long long nb_moments_lds(int dp, int C, bool shift) {
  const long long tr = nb_tr(dp);
  return tr * (dp + 16) * 2 + tr * 8 + tr * 4 + (shift ? (long long)C * dp * 8 : 0);
}

// Doubles of the table of the scores form in LDS (rounded up to an even count).
__host__ __device__ constexpr long long nb_tab_doubles(int dp, int C, bool gauss) {
  const long long c16 = (C + 15) & ~15;
  const long long t = gauss ? 2LL * C * (dp + 1) + C : c16 * dp + c16;
  return (t + 1) & ~1LL;
}

long long nb_scores_lds(int dp, int C, bool gauss) {
  const long long tr = nb_tr(dp);
  return tr * (dp + 4) * 2 + nb_tab_doubles(dp, C, gauss) * 8 + tr * nb_rp(C) * 8;
}

// One item = 8 bf16 of one row (16 bytes); a thread holds its NI items of a tile in registers.
template <int DP>
struct NbTile {
  static constexpr int TR = nb_tr(DP);
  static constexpr int NI = TR * DP / 8 / kNbThreads;  // 1 at DP = 16, else 2
  static constexpr int CH = DP / 8;                    // items of a row
  uint4 pf[NI];

  __device__ __forceinline__ void fetch(const u16* __restrict__ X, long long n, int d, long long tile, int tid) {
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const int it = tid + kNbThreads * k, row = it / CH, col = 8 * (it % CH);
      const long long r = tile * TR + row;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (r < n && col < d) v = *reinterpret_cast<const uint4*>(X + r * DP + col);
      pf[k] = v;
    }
  }

  // The pad columns are masked by d, not trusted. XP: bf16 pitch of a staged row, a multiple of 4.
  template <int XP>
  __device__ __forceinline__ void stage(u16* __restrict__ Xs, int d, int tid) const {
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const int it = tid + kNbThreads * k, row = it / CH, cc = it % CH;
      const int nv = d - 8 * cc;  // live columns of this item (<= 0: none, >= 8: all)
      auto mk = [nv](int e) { return (2 * e < nv ? 0x0000ffffu : 0u) | (2 * e + 1 < nv ? 0xffff0000u : 0u); };
      const uint4 v = pf[k];
      uint2* dst = reinterpret_cast<uint2*>(Xs + row * XP + 8 * cc);
      dst[0] = make_uint2(v.x & mk(0), v.y & mk(1));
      dst[1] = make_uint2(v.z & mk(2), v.w & mk(3));
    }
  }
};

// ------------------------------------------------------------------------------------------------- moments form
// part: [grid * RS] slots of C (1 + 2 d) doubles = [n_c | S1 | S2] per class, then [grid][2] bad counts.
template <int DP, bool SECOND>
__global__ __launch_bounds__(kNbThreads) void nb_moments_kernel(const u16* __restrict__ X, long long n, int d, int C,
                                                                const int* __restrict__ labels,
                                                                const double* __restrict__ wts,
                                                                const double* __restrict__ shift,
                                                                double* __restrict__ part) {
  constexpr int TR = nb_tr(DP), XP = DP + 16, WC = nb_wc(DP), RS = nb_rs(DP), RR = TR / RS, NCT = DP / 16 / WC;
  constexpr int NM = SECOND ? 2 : 1;
  extern __shared__ __align__(16) unsigned char nb_smem[];
  u16* Xs = reinterpret_cast<u16*>(nb_smem);                           // [TR][XP]
  double* ws = reinterpret_cast<double*>(nb_smem + TR * XP * 2);       // [TR]
  int* ls = reinterpret_cast<int*>(ws + TR);                           // [TR]
  double* ms = reinterpret_cast<double*>(ls + TR);                     // [C][DP], with a shift only
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wave % WC, rs = wave / WC;
  const bool shifted = shift != nullptr;
  const bool two = C > 16;

  if (shifted)
    for (int i = tid; i < C * DP; i += kNbThreads) {
      const int col = i % DP;
      ms[i] = col < d ? shift[(long long)(i / DP) * d + col] : 0.0;
    }

  const long long ntiles = (n + TR - 1) / TR;
  long long t0, t1;
  tile_run(ntiles, t0, t1);

  NbTile<DP> tl;
  int pl = -1;
  double pw = 0.0;
  auto fetch_row = [&](long long tile) {
    if (tid < TR) {
      const long long r = tile * TR + tid;
      pl = r < n ? labels[r] : -1;
      pw = r < n ? (wts != nullptr ? wts[r] : 1.0) : 0.0;
    }
  };

  f64x4 acc[NCT][2][NM];
#pragma unroll
  for (int i = 0; i < NCT; ++i)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int m = 0; m < NM; ++m) acc[i][b][m] = (f64x4)0.0;
  double nc0 = 0.0, nc1 = 0.0;
  unsigned neg = 0, non01 = 0;

  if (t0 < t1) {
    tl.fetch(X, n, d, t0, tid);
    fetch_row(t0);
  }
  for (long long tile = t0; tile < t1; ++tile) {
    tl.template stage<XP>(Xs, d, tid);
    if (tid < TR) {
      ls[tid] = pl;
      ws[tid] = pw;
    }
    __syncthreads();
    if (tile + 1 < t1) {
      tl.fetch(X, n, d, tile + 1, tid);
      fetch_row(tile + 1);
    }
#pragma unroll 2
    for (int s = 0; s < RR / 4; ++s) {
      const int row = rs * RR + 4 * s + g;
      const int l = ls[row];
      const double w = ws[row];
      const bool in = (unsigned)l < (unsigned)C;
      const double a0 = l == c ? w : 0.0;
      const double a1 = l == 16 + c ? w : 0.0;
      if (wc == 0) {
        nc0 += a0;
        nc1 += a1;
      }
#pragma unroll
      for (int i = 0; i < NCT; ++i) {
        const int col = 16 * (wc + WC * i) + c;
        const double x = (double)bf16_to_f32(Xs[row * XP + col]);
        neg += x < 0.0 ? 1u : 0u;
        non01 += (x != 0.0 && x != 1.0) ? 1u : 0u;
        double b = x;
        if (shifted) b = x - (in ? ms[l * DP + col] : 0.0);
        acc[i][0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[i][0][0], 0, 0, 0);
        if (two) acc[i][1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[i][1][0], 0, 0, 0);
        if constexpr (SECOND) {
          const double b2 = b * b;
          acc[i][0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b2, acc[i][0][1], 0, 0, 0);
          if (two) acc[i][1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b2, acc[i][1][1], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // ---- the partials of this (workgroup, row split): register r of a lane is class g + 4 r, column c of its block
  const long long cs = 1 + 2LL * d, ss = cs * C;
  double* slot = part + ((long long)blockIdx.x * RS + rs) * ss;
#pragma unroll
  for (int i = 0; i < NCT; ++i) {
    const int col = 16 * (wc + WC * i) + c;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int cls = 16 * b + g + 4 * r;
        if (cls < C && col < d) {
          slot[cls * cs + 1 + col] = acc[i][b][0][r];
          if constexpr (SECOND) slot[cls * cs + 1 + d + col] = acc[i][b][1][r];
        }
      }
  }
  if (wc == 0) {
    const double v0 = lane_groups_sum(nc0), v1 = lane_groups_sum(nc1);
    if (g == 0) {
      if (c < C) slot[c * cs] = v0;
      if (16 + c < C) slot[(16 + c) * cs] = v1;
    }
  }
  // ---- the bad counts: per wave by shuffles, then in wave order (the last tile's barrier has released the tile)
  unsigned long long bn = neg, bz = non01;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    bn += __shfl_xor(bn, o, 64);
    bz += __shfl_xor(bz, o, 64);
  }
  unsigned long long* red = reinterpret_cast<unsigned long long*>(ws);  // 16 <= TR values
  if (lane == 0) {
    red[2 * wave] = bn;
    red[2 * wave + 1] = bz;
  }
  __syncthreads();
  if (tid < 2) {
    unsigned long long s = 0;
    for (int v = 0; v < kNbWaves; ++v) s += red[2 * v + tid];
    part[(long long)gridDim.x * RS * ss + 2LL * blockIdx.x + tid] = (double)s;
  }
}

// out [C (1 + 2 d) + 2]: one wave per entry. Lane l adds the slots l, l + 64, .. in that order, the 64 sums meet in
// the fixed butterfly of wave_sum_f64 and lane 0 writes: the same bits on every call, and the slots are read side by
// side, not one after the other by one thread. The S2 entries are left as they are without `second`; the two bad
// counts are summed over the workgroups the same way.
__global__ __launch_bounds__(256) void nb_fold_kernel(const double* __restrict__ part, int grid, int rs, int C, int d,
                                                      int second, double* __restrict__ out) {
  const long long cs = 1 + 2LL * d, ss = cs * C;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long e = t >> 6;  // uniform over a wave
  const int lane = (int)(t & 63);
  if (e >= ss + 2) return;
  double s = 0.0;
  if (e < ss) {
    if (e % cs > d && !second) return;
    const long long nslots = (long long)grid * rs;
    for (long long k = lane; k < nslots; k += 64) s += part[k * ss + e];
  } else {
    const double* bad = part + (long long)grid * rs * ss + (e - ss);
    for (int k = lane; k < grid; k += 64) s += bad[2LL * k];
  }
  s = wave_sum_f64(s);
  if (lane == 0) out[e] = s;
}

// -------------------------------------------------------------------------------------------------- scores form
enum { kNbLinear = 0, kNbComplement = 1, kNbGaussian = 2 };

// tab: linear / complement f64 [C16][DP] W zero padded (classes to C16 = 16 ceil(C / 16), columns to DP), then
// [C16] b; gaussian f64 [C][DP] theta, [C][DP] iv (zero padded columns), [C] b.
template <int DP, bool GAUSS>
__global__ __launch_bounds__(kNbThreads) void nb_scores_kernel(const u16* __restrict__ X, long long n, int d, int C,
                                                               int kind, const double* __restrict__ tab,
                                                               double* __restrict__ raw, double* __restrict__ prob,
                                                               double* __restrict__ pred) {
  constexpr int TR = nb_tr(DP), XP = DP + 4, NG = TR / 16, SUB = kNbThreads / TR, TP = DP + 1;
  extern __shared__ __align__(16) unsigned char nb_smem[];
  u16* Xs = reinterpret_cast<u16*>(nb_smem);                          // [TR][XP]
  double* T = reinterpret_cast<double*>(nb_smem + TR * XP * 2);        // the table
  double* R = T + nb_tab_doubles(DP, C, GAUSS);                        // [TR][RP]
  const int RP = nb_rp(C), C16 = (C + 15) & ~15;
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // linear: W image [C16][DP] swizzled, b [C16]; gaussian: theta [C][TP], iv [C][TP], b [C]
  double* bs = GAUSS ? T + 2 * C * TP : T + C16 * DP;
  if constexpr (GAUSS) {
    for (int i = tid; i < 2 * C * DP; i += kNbThreads) T[(i / DP) * TP + i % DP] = tab[i];
    for (int i = tid; i < C; i += kNbThreads) bs[i] = tab[2 * C * DP + i];
  } else {
    for (int i = tid; i < C16 * DP; i += kNbThreads) {
      const int cls = i / DP, col = i % DP;
      T[cls * DP + (unit_swizzle(cls, col) & (DP - 1))] = tab[i];
    }
    for (int i = tid; i < C16; i += kNbThreads) bs[i] = tab[C16 * DP + i];
  }

  const long long ntiles = (n + TR - 1) / TR;
  long long t0, t1;
  tile_run(ntiles, t0, t1);
  NbTile<DP> tl;
  if (t0 < t1) tl.fetch(X, n, d, t0, tid);
  for (long long tile = t0; tile < t1; ++tile) {
    tl.template stage<XP>(Xs, d, tid);
    __syncthreads();  // also: the table is there, and the previous tile's lse step has read R
    if (tile + 1 < t1) tl.fetch(X, n, d, tile + 1, tid);

    // ---- phase 1: s[row][class] into R
    if constexpr (GAUSS) {
      for (int item = tid; item < TR * C; item += kNbThreads) {
        const int row = item / C, cls = item % C;
        const u16* xr = Xs + row * XP;
        const double* th = T + cls * TP;
        const double* iv = T + (C + cls) * TP;
        double q = 0.0;
        for (int col = 0; col < d; col += 4) {  // columns d .. d + 3: x, theta and iv are 0 there
          const uint2 v = *reinterpret_cast<const uint2*>(xr + col);
          const double x0 = bf16hi_to_f64(v.x << 16), x1 = bf16hi_to_f64(v.x & 0xffff0000u);
          const double x2 = bf16hi_to_f64(v.y << 16), x3 = bf16hi_to_f64(v.y & 0xffff0000u);
          const double e0 = x0 - th[col], e1 = x1 - th[col + 1], e2 = x2 - th[col + 2], e3 = x3 - th[col + 3];
          q = __builtin_fma(e0 * e0, iv[col], q);
          q = __builtin_fma(e1 * e1, iv[col + 1], q);
          q = __builtin_fma(e2 * e2, iv[col + 2], q);
          q = __builtin_fma(e3 * e3, iv[col + 3], q);
        }
        R[row * RP + cls] = bs[cls] - 0.5 * q;
      }
    } else {
      const int nsteps = (d + 3) / 4;
      for (int item = wave; item < NG * (C16 / 16); item += kNbWaves) {
        const int grp = item % NG, cb = item / NG;
        const int cls = 16 * cb + r16;  // this lane's class as the B operand and as the result column
        const u16* xr = Xs + (16 * grp + r16) * XP;
        const double* wr = T + cls * DP;
        f64x4 D = (f64x4)0.0;
        for (int s = 0; s < nsteps; ++s) {
          const int t = 4 * s + kq;
          D = __builtin_amdgcn_mfma_f64_16x16x4f64((double)bf16_to_f32(xr[t]),
                                                   wr[unit_swizzle(cls, t) & (DP - 1)], D, 0, 0, 0);
        }
        if (cls < C) {
          const double b = bs[cls];
#pragma unroll
          for (int r = 0; r < 4; ++r) R[(16 * grp + kq + 4 * r) * RP + cls] = D[r] + b;
        }
      }
    }
    __syncthreads();

    // ---- lse: SUB adjacent lanes per row
    {
      const int row = tid / SUB, sub = tid % SUB;
      const long long grow = tile * TR + row;
      const double* rr = R + row * RP;
      double m = -__builtin_huge_val();
      for (int j = sub; j < C; j += SUB) m = fmax(m, rr[j]);
#pragma unroll
      for (int o = SUB / 2; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, SUB));
      double se = 0.0;
      for (int j = sub; j < C; j += SUB) se += exp(rr[j] - m);
#pragma unroll
      for (int o = SUB / 2; o > 0; o >>= 1) se += __shfl_xor(se, o, SUB);
      const double lse = m + log(se);
      double best = -__builtin_huge_val();
      int am = 0x7fffffff;
      for (int j = sub; j < C; j += SUB) {
        const double sv = rr[j], dl = sv - lse;
        const double rv = kind == kNbComplement ? dl : sv;
        if (rv > best) {
          best = rv;
          am = j;
        }
        if (grow < n) {
          raw[grow * C + j] = rv;
          prob[grow * C + j] = exp(dl);
        }
      }
#pragma unroll
      for (int o = SUB / 2; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, SUB);
        const int oa = __shfl_xor(am, o, SUB);
        if (ob > best || (ob == best && oa < am)) {
          best = ob;
          am = oa;
        }
      }
      if (sub == 0 && grow < n) pred[grow] = am < C ? (double)am : 0.0;
    }
    // the next tile's first barrier separates these reads of R from its phase 1
  }
}

bool nb_args_ok(const void* X, long long n, int dp, int d, int C) {
  if (!nb_dp_ok(dp) || d < 1 || d > dp || C < 1 || C > kNbMaxC || n < 0 || X == nullptr) return false;
  return (reinterpret_cast<size_t>(X) & 15) == 0;  // the 16-byte row loads
}

template <int DP>
int nb_launch_moments(int second, int grid, long long lds, hipStream_t st, const void* X, long long n, int d, int C,
                      const int* labels, const double* wts, const double* shift, double* part) {
  return second ? cml_launch_lds(nb_moments_kernel<DP, true>, grid, kNbThreads, lds, st, (const u16*)X, n, d, C, labels,
                                 wts, shift, part)
                : cml_launch_lds(nb_moments_kernel<DP, false>, grid, kNbThreads, lds, st, (const u16*)X, n, d, C, labels,
                                 wts, shift, part);
}

template <int DP>
int nb_launch_scores(int kind, int grid, long long lds, hipStream_t st, const void* X, long long n, int d, int C,
                     const double* tab, double* raw, double* prob, double* pred) {
  return kind == kNbGaussian ? cml_launch_lds(nb_scores_kernel<DP, true>, grid, kNbThreads, lds, st, (const u16*)X, n, d,
                                              C, kind, tab, raw, prob, pred)
                             : cml_launch_lds(nb_scores_kernel<DP, false>, grid, kNbThreads, lds, st, (const u16*)X, n, d,
                                              C, kind, tab, raw, prob, pred);
}

#define NB_BY_DP(dp, call)          \
  switch (dp) {                     \
    case 16: return call(16);       \
    case 32: return call(32);       \
    case 64: return call(64);       \
    case 128: return call(128);     \
    case 256: return call(256);     \
    default: return call(512);      \
  }

}  // namespace

// LDS bytes K34 needs for a model of this padded width, C classes and kind (the larger of the moments form, shifted
// for gaussian, and the scores form); 0 = outside the kernel's limits.
CML_API long long cml_nb_lds(int dp, int C, int gaussian) {
  if (!nb_dp_ok(dp) || C < 1 || C > kNbMaxC) return 0;
  const long long a = nb_moments_lds(dp, C, gaussian != 0), b = nb_scores_lds(dp, C, gaussian != 0);
  const long long lds = a > b ? a : b;
  return lds <= kLdsPerCu ? lds : 0;
}

// Workgroups of a launch of either form: a function of (n, dp, CUs) only (C is taken for the checks). 0 = unsupported
// or no row. Two workgroups per CU where the LDS lets them in together; otherwise they follow each other.
CML_API int cml_nb_grid(long long n, int dp, int C, int ncu) {
  if (!nb_dp_ok(dp) || C < 1 || C > kNbMaxC || n <= 0) return 0;
  const long long tr = nb_tr(dp);
  return (int)cml_grid_cap((n + tr - 1) / tr, ncu, 2);
}

// Doubles of the partial buffer of a moments launch of `grid` workgroups.
CML_API long long cml_nb_part(int dp, int C, int d, int grid) {
  if (!nb_dp_ok(dp)) return 0;
  return (long long)grid * nb_rs(dp) * C * (1 + 2LL * d) + 2LL * grid;
}

// X: bf16 [n, dp] contiguous (16-byte base); labels int32 [n]; wts f64 [n] or null; shift f64 [C, d] or null;
// part f64 [cml_nb_part]; out f64 [C (1 + 2 d) + 2] = [n_c | S1 | S2] per class, then bad; the S2 entries are left
// untouched unless `second`.
CML_API int cml_nb_moments(const void* X, long long n, int dp, int d, int C, const int* labels, const double* wts,
                           const double* shift, int second, double* part, int grid, double* out, int ncu,
                           void* stream) {
  if (!nb_args_ok(X, n, dp, d, C) || n == 0 || labels == nullptr || part == nullptr || out == nullptr ||
      grid != cml_nb_grid(n, dp, C, ncu))
    return (int)hipErrorInvalidValue;
  const long long lds = nb_moments_lds(dp, C, shift != nullptr);
  if (lds > kLdsPerCu) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
#define NB_CALL(DPV) nb_launch_moments<DPV>(second, grid, lds, st, X, n, d, C, labels, wts, shift, part)
  const int rc = [&]() -> int { NB_BY_DP(dp, NB_CALL) }();
#undef NB_CALL
  if (rc != 0) return rc;
  return cml_launch_fold(nb_fold_kernel, 64 * ((long long)C * (1 + 2LL * d) + 2), st, (const double*)part, grid, nb_rs(dp), C, d,
                         second, out);
}

// kind 0 linear, 1 complement, 2 gaussian; tab as nb_scores_kernel describes it; raw, prob f64 [n, C], pred f64 [n].
CML_API int cml_nb_scores(const void* X, long long n, int dp, int d, int C, int kind, const double* tab, double* raw,
                          double* prob, double* pred, int ncu, void* stream) {
  if (!nb_args_ok(X, n, dp, d, C) || kind < 0 || kind > 2 || tab == nullptr || raw == nullptr || prob == nullptr ||
      pred == nullptr)
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const long long lds = nb_scores_lds(dp, C, kind == kNbGaussian);
  if (lds > kLdsPerCu) return (int)hipErrorInvalidValue;
  const int grid = cml_nb_grid(n, dp, C, ncu);
  hipStream_t st = (hipStream_t)stream;
#define NB_CALL(DPV) nb_launch_scores<DPV>(kind, grid, lds, st, X, n, d, C, tab, raw, prob, pred)
  NB_BY_DP(dp, NB_CALL)
#undef NB_CALL
}
