// K26 silhouette from cluster statistics (ClusteringEvaluator): three kernels for bf16 / e4m3 rows in the
// to_device_matrix layout.
//
//   cml_row_sqnorm_f64    |x_i|^2 per row in f64 (the products of bf16 / e4m3 values are exact in f32 and
//                         are added in f64): Q_c = sum w |x|^2, the cosine factor w / |x| and the zero-row
//                         check all come from it.
//   cml_label_wsum        S[c][:] = sum over the rows of cluster c of omega_i x_i in f64, deterministic and
//                         atomic-free: the rows are taken in label order (`perm`, a stable sort of the labels),
//                         cut into units of L consecutive positions. The dp/2 threads of a unit walk its rows
//                         in order, each adding omega·x of its column pair in f64. A cluster that begins and
//                         ends inside one unit is written to S directly; the first and the last segment of a
//                         unit (clusters it may share with its neighbours) go to head / tail partials, which
//                         a second launch (one workgroup per cluster) adds in unit order. The order of every
//                         addition is fixed by (n, L, labels), so two calls return the same bits.
//   cml_silhouette_score  the hot pass, one read of X. D_c(x) for every live cluster c on
//                         v_mfma_f32_16x16x32_bf16, A = 16 centres, B = 16 rows: a lane ends up with 4 centres
//                         of ONE row, so "own cluster and the best of the others" is 4 registers plus two
//                         exchanges (lanes l ^ 16, l ^ 32). The rows are the stationary operand: a wave keeps
//                         RT tiles of 16 rows in registers (loaded once, straight from global memory in the
//                         B-operand layout; e4m3 rows are widened exactly to bf16 on the way) and the centre
//                         table streams past them through LDS in tiles of 16 centres, double-buffered and
//                         shared by the workgroup's 4 waves. No n x K array exists.
//
// The centre operand nu (host, f64 -> f32) is split into three bf16 terms hi + mid + lo = nu exactly (24 bits
// of f32 in 3 x 8), so every product bf16 x bf16 is exact in f32 and only the f32 accumulation of the 3·dp
// products rounds:
//   squaredEuclidean  D_c(x) = r - 2 x·nu_c + kappa_c,  nu_c = mu_c - m, r = |x - m|^2 (in the kernel, f32),
//                     kappa_c = q_c - 2 m·mu_c + |m|^2 + 2 m·nu_c (host, f64), m the weighted global mean:
//                     D_c is translation-invariant and the shift removes the |x|^2-sized cancellation
//   cosine            D_c(x) = 1 - x·nu_c / |x|,  nu_c = mu_c (the mean of the unit rows), kappa_c = 0
//   dead clusters (W_c = 0) and the padding of the last centre tile carry kappa = +inf.
//
// Error model (u = 2^-24, recursive summation of 3·dp exact products, the f32 rounding of nu, r and the
// final three-term sum), for every row i and cluster c:
//   squaredEuclidean  |D_kernel - D_f64| <= E_i = u·[(6·dp + 12)·|x_i|·max_c|nu_c| + (dp + 6)·r_i + 4·max_c|kappa_c|]
//   cosine            |D_kernel - D_f64| <= E_i = u·(6·dp + 16)
// tests/test_silhouette_gpu.py asserts these bounds per row.
//
// Epilogue (f64, a handful of operations per row): a = own·W/(W - w) unless W == w (a cluster of one row's
// weight: s = 0), s = 1 - a/b (a < b), b/a - 1 (a > b), 0 otherwise; sum w·s and sum w are reduced per
// workgroup in f64 (lanes, then waves, in fixed order) to one partial pair; a second launch adds the
// pairs in workgroup order.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ uint4 widen8_e4m3(const uint2 q) {  // 8 e4m3 values -> 8 bf16, exact
  uint4 o;
  o.x = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q.x, 1.0f, false));
  o.y = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q.x, 1.0f, true));
  o.z = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q.y, 1.0f, false));
  o.w = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q.y, 1.0f, true));
  return o;
}

// ------------------------------------------------------------------------------------------- row norms
// 16 lanes per row, lane j takes the 8-value chunks j, j + 16, ...
template <bool F8>
__global__ __launch_bounds__(kThreads) void row_sqnorm_kernel(const void* __restrict__ Xv, long long n, long long ld,
                                                              double* __restrict__ out) {
  const int j = threadIdx.x & 15;
  const long long row = (long long)blockIdx.x * (kThreads / 16) + (threadIdx.x >> 4);
  double acc = 0.0;
  if (row < n) {
    const unsigned char* X = reinterpret_cast<const unsigned char*>(Xv);
    for (long long c = 8 * j; c < ld; c += 128) {
      uint4 v;
      if constexpr (F8) v = widen8_e4m3(*reinterpret_cast<const uint2*>(X + row * ld + c));
      else v = *reinterpret_cast<const uint4*>(X + (row * ld + c) * 2);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float a = __uint_as_float(w[k] << 16), b = __uint_as_float(w[k] & 0xffff0000u);
        acc += (double)(a * a);  // exact in f32: 8-bit significands
        acc += (double)(b * b);
      }
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (row < n && j == 0) out[row] = acc;
}

// ------------------------------------------------------------------------------------- weighted label sums
constexpr int kBatch = 8;  // rows whose loads are in flight together

template <bool F8>
__global__ __launch_bounds__(kThreads) void label_wsum_kernel(
    const void* __restrict__ Xv, long long n, long long ld, int dp, const int* __restrict__ slab /*sorted labels*/,
    const long long* __restrict__ perm, const double* __restrict__ omega, int L, long long nunits, int tpu,
    double* __restrict__ S /*[K][dp]*/, double* __restrict__ head /*[nunits][dp]*/,
    double* __restrict__ tail /*[nunits][dp]*/, int* __restrict__ hl /*[nunits][2]*/) {
  const long long unit = (long long)blockIdx.x * (kThreads / tpu) + threadIdx.x / tpu;
  const int p = threadIdx.x % tpu;  // column pair 2p, 2p + 1
  if (unit >= nunits) return;
  const unsigned char* X = reinterpret_cast<const unsigned char*>(Xv);
  const long long i0 = unit * L, i1 = i0 + L < n ? i0 + L : n;
  const int first = slab[i0];
  int cur = first;
  bool in_head = true;
  double a0 = 0.0, a1 = 0.0;
  for (long long ib = i0; ib < i1; ib += kBatch) {
    int c[kBatch];
    double w[kBatch];
    float x0[kBatch], x1[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      const long long i = ib + k;
      const bool ok = i < i1;
      c[k] = ok ? slab[i] : -1;
      const long long r = ok ? perm[i] : 0;
      w[k] = ok ? (omega != nullptr ? omega[r] : 1.0) : 0.0;
      if constexpr (F8) {
        const unsigned q = ok ? *reinterpret_cast<const u16*>(X + r * ld + 2 * p) : 0u;
        const unsigned b = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q, 1.0f, false));
        x0[k] = __uint_as_float(b << 16);
        x1[k] = __uint_as_float(b & 0xffff0000u);
      } else {
        const unsigned b = ok ? *reinterpret_cast<const unsigned*>(X + (r * ld + 2 * p) * 2) : 0u;
        x0[k] = __uint_as_float(b << 16);
        x1[k] = __uint_as_float(b & 0xffff0000u);
      }
    }
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      if (c[k] < 0) break;  // past the unit's end
      if (c[k] != cur) {
        double* dst = in_head ? head + unit * dp : S + (long long)cur * dp;
        dst[2 * p] = a0;
        dst[2 * p + 1] = a1;
        in_head = false;
        a0 = 0.0;
        a1 = 0.0;
        cur = c[k];
      }
      a0 += w[k] * (double)x0[k];
      a1 += w[k] * (double)x1[k];
    }
  }
  double* dst = in_head ? head + unit * dp : tail + unit * dp;
  dst[2 * p] = a0;
  dst[2 * p + 1] = a1;
  if (p == 0) {
    hl[2 * unit] = first;
    hl[2 * unit + 1] = in_head ? -1 : cur;
  }
}

// One workgroup per cluster: the head / tail partials of the units its rows span, in unit order.
__global__ __launch_bounds__(kThreads) void label_wsum_combine_kernel(const long long* __restrict__ off /*[K+1]*/,
                                                                      int L, int dp, const double* __restrict__ head,
                                                                      const double* __restrict__ tail,
                                                                      const int* __restrict__ hl,
                                                                      double* __restrict__ S) {
  const int c = blockIdx.x;
  const long long s = off[c], e = off[c + 1];
  if (s >= e) return;  // empty cluster: S stays zero
  const long long u0 = s / L, u1 = (e - 1) / L;
  for (int j = threadIdx.x; j < dp; j += kThreads) {
    double acc = 0.0;
    bool any = false;
    for (long long u = u0; u <= u1; ++u) {
      if (hl[2 * u] == c) {
        acc += head[u * dp + j];
        any = true;
      } else if (hl[2 * u + 1] == c) {
        acc += tail[u * dp + j];
        any = true;
      }
    }
    if (any) S[(long long)c * dp + j] = acc;  // else the cluster lay inside one unit and is already written
  }
}

// ----------------------------------------------------------------------------------------------- the score pass
template <int KS>
struct ScoreCfg {
  static constexpr int DP = 32 * KS;
  static constexpr int BP = DP + 16;  // plane pitch (bf16): rows 8 dwords apart mod 64, so the 16 rows x 2 column
                                      // groups of one ds_read_b128 lane group fall on 16 distinct 16-byte slots
  static constexpr int TILE = 3 * 16 * BP;      // bf16 elements of one staged centre tile (hi, mid, lo planes)
  static constexpr int CHUNKS = 3 * 16 * DP / 8;  // 16-byte pieces of a tile in the global table
  static constexpr int CPT = (CHUNKS + kThreads - 1) / kThreads;
  static constexpr size_t LDS = (size_t)2 * TILE * 2 + (size_t)DP * 4 + kWaves * 2 * 8;
};

// a centre tile on its way from the global table to its LDS image: thread tid carries pieces tid, tid + 256, ...
template <int KS>
__device__ __forceinline__ void stage_load(uint4 (&st)[ScoreCfg<KS>::CPT], const u16* __restrict__ tab, int t, int tid) {
  using Cfg = ScoreCfg<KS>;
  const uint4* src = reinterpret_cast<const uint4*>(tab) + (size_t)t * Cfg::CHUNKS;
#pragma unroll
  for (int i = 0; i < Cfg::CPT; ++i) {
    const int q = tid + i * kThreads;
    st[i] = (Cfg::CHUNKS % kThreads == 0 || q < Cfg::CHUNKS) ? src[q] : make_uint4(0u, 0u, 0u, 0u);
  }
}
template <int KS>
__device__ __forceinline__ void stage_store(const uint4 (&st)[ScoreCfg<KS>::CPT], u16* b, int tid) {
  using Cfg = ScoreCfg<KS>;
#pragma unroll
  for (int i = 0; i < Cfg::CPT; ++i) {
    const int q = tid + i * kThreads;
    if (Cfg::CHUNKS % kThreads == 0 || q < Cfg::CHUNKS) {
      const int row = q / (Cfg::DP / 8), ch = q - row * (Cfg::DP / 8);
      *reinterpret_cast<uint4*>(b + row * Cfg::BP + ch * 8) = st[i];
    }
  }
}

template <int KS, int RT, bool F8>
__global__ __launch_bounds__(kThreads) void silhouette_score_kernel(
    const void* __restrict__ Xv, long long n, long long ld, const int* __restrict__ label,
    const double* __restrict__ wt, const u16* __restrict__ tab /*[KT][3][16][DP]*/,
    const float* __restrict__ kappa /*[16 KT]*/, const float* __restrict__ mean /*[DP]*/,
    const double* __restrict__ Wc /*[K]*/, int KT, int cosine, double* __restrict__ partial /*[grid][2]*/,
    float* __restrict__ o_own, float* __restrict__ o_b, int* __restrict__ o_nb, float* __restrict__ o_s) {
  using Cfg = ScoreCfg<KS>;
  constexpr int DP = Cfg::DP, BP = Cfg::BP, CPT = Cfg::CPT;
  extern __shared__ __align__(16) unsigned char smem[];
  u16* buf0 = reinterpret_cast<u16*>(smem);  // two staged centre tiles: buf0 + (t & 1)·TILE
  float* mean_l = reinterpret_cast<float*>(smem + (size_t)2 * Cfg::TILE * 2);
  double* red = reinterpret_cast<double*>(mean_l + DP);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g4 = lane >> 4;
  const unsigned char* X = reinterpret_cast<const unsigned char*>(Xv);

  uint4 st[CPT];
  stage_load<KS>(st, tab, 0, tid);
  for (int i = tid; i < DP; i += kThreads) mean_l[i] = mean[i];
  stage_store<KS>(st, buf0, tid);

  // this wave's rows: RT tiles of 16, lane (r16, g4) holds columns 32s + 8 g4 .. + 7 of row 16u + r16
  const long long base = ((long long)blockIdx.x * kWaves + wave) * (16 * RT);
  bf16x8 xb[RT][KS];
  int lab[RT];
  long long rowi[RT];
#pragma unroll
  for (int u = 0; u < RT; ++u) {
    rowi[u] = base + 16 * u + r16;
    const bool ok = rowi[u] < n;
    lab[u] = ok ? label[rowi[u]] : -1;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int col = 32 * s + 8 * g4;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (ok && col < ld) {
        if constexpr (F8) v = widen8_e4m3(*reinterpret_cast<const uint2*>(X + rowi[u] * ld + col));
        else v = *reinterpret_cast<const uint4*>(X + (rowi[u] * ld + col) * 2);
      }
      xb[u][s] = __builtin_bit_cast(bf16x8, v);
    }
  }
  __syncthreads();  // tile 0 and the mean are staged
  // r = |x - m|^2 of the lane's row (m = 0 for cosine: r = |x|^2)
  float rr[RT], inv[RT];
#pragma unroll
  for (int u = 0; u < RT; ++u) {
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const uint4 v = __builtin_bit_cast(uint4, xb[u][s]);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
      const float4 m0 = *reinterpret_cast<const float4*>(mean_l + 32 * s + 8 * g4);
      const float4 m1 = *reinterpret_cast<const float4*>(mean_l + 32 * s + 8 * g4 + 4);
      const float mm[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float a = __uint_as_float(w[k] << 16) - mm[2 * k];
        const float b = __uint_as_float(w[k] & 0xffff0000u) - mm[2 * k + 1];
        acc += a * a;
        acc += b * b;
      }
    }
    acc += __shfl_xor(acc, 16, 64);
    acc += __shfl_xor(acc, 32, 64);
    rr[u] = acc;
    inv[u] = acc > 0.f ? 1.f / sqrtf(acc) : 0.f;
  }

  float own[RT], best[RT];
  int bi[RT];
#pragma unroll
  for (int u = 0; u < RT; ++u) {
    own[u] = 0.f;
    best[u] = __builtin_huge_valf();
    bi[u] = -1;
  }

  for (int t = 0; t < KT; ++t) {
    const u16* cur = buf0 + (t & 1) * Cfg::TILE;
    if (t + 1 < KT) stage_load<KS>(st, tab, t + 1, tid);
    f32x4 acc[RT];
#pragma unroll
    for (int u = 0; u < RT; ++u) acc[u] = (f32x4)0.f;
    const u16* a0 = cur + r16 * BP + 8 * g4;  // A: centre 16t + r16, columns 32s + 8 g4 .. + 7
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const bf16x8 ah = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(a0 + 32 * s));
      const bf16x8 am = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(a0 + 16 * BP + 32 * s));
      const bf16x8 al = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(a0 + 32 * BP + 32 * s));
#pragma unroll
      for (int u = 0; u < RT; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, xb[u][s], acc[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < RT; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, xb[u][s], acc[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < RT; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, xb[u][s], acc[u], 0, 0, 0);
    }
    // acc[u][reg] = x(row 16u + r16)·nu(centre 16t + 4 g4 + reg)
    const float4 kp4 = *reinterpret_cast<const float4*>(kappa + 16 * t + 4 * g4);
    const float kp[4] = {kp4.x, kp4.y, kp4.z, kp4.w};
#pragma unroll
    for (int u = 0; u < RT; ++u)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int c = 16 * t + 4 * g4 + reg;
        const float dist = cosine ? (1.f - acc[u][reg] * inv[u]) + kp[reg] : (rr[u] - 2.f * acc[u][reg]) + kp[reg];
        if (c == lab[u]) {
          own[u] = dist;
        } else if (dist < best[u]) {
          best[u] = dist;
          bi[u] = c;
        }
      }
    if (t + 1 < KT) stage_store<KS>(st, buf0 + ((t + 1) & 1) * Cfg::TILE, tid);
    __syncthreads();
  }

  double sws = 0.0, sw = 0.0;
#pragma unroll
  for (int u = 0; u < RT; ++u) {
    float o = own[u];  // set on one of the row's four lanes, 0 on the others
    o += __shfl_xor(o, 16, 64);
    o += __shfl_xor(o, 32, 64);
    float b = best[u];
    int ix = bi[u];
#pragma unroll
    for (int sh = 16; sh <= 32; sh <<= 1) {
      const float ob = __shfl_xor(b, sh, 64);
      const int oi = __shfl_xor(ix, sh, 64);
      if (ob < b || (ob == b && oi >= 0 && (ix < 0 || oi < ix))) {
        b = ob;
        ix = oi;
      }
    }
    if (g4 == 0 && rowi[u] < n) {
      const double w = wt != nullptr ? wt[rowi[u]] : 1.0;
      const double W = Wc[lab[u]];
      double sv = 0.0;
      if (W != w) {
        const double a = (double)o * W / (W - w), bd = (double)b;
        sv = a < bd ? 1.0 - a / bd : (a > bd ? bd / a - 1.0 : 0.0);
      }
      sws += w * sv;
      sw += w;
      if (o_own != nullptr) {
        o_own[rowi[u]] = o;
        o_b[rowi[u]] = b;
        o_nb[rowi[u]] = ix;
        o_s[rowi[u]] = (float)sv;
      }
    }
  }
  sws = wave_sum_f64(sws);
  sw = wave_sum_f64(sw);
  if (lane == 0) {
    red[2 * wave] = sws;
    red[2 * wave + 1] = sw;
  }
  __syncthreads();
  if (tid == 0) {
    double a = red[0], b = red[1];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      a += red[2 * w];
      b += red[2 * w + 1];
    }
    partial[2 * (long long)blockIdx.x] = a;
    partial[2 * (long long)blockIdx.x + 1] = b;
  }
}

// out[0..1] = the partial pairs added in workgroup order: thread t folds pairs t, t + 256, ..., then an LDS tree.
__global__ __launch_bounds__(kThreads) void silhouette_final_kernel(const double* __restrict__ partial, long long nb,
                                                                    double* __restrict__ out) {
  __shared__ double sh[2][kThreads];
  double a = 0.0, b = 0.0;
  for (long long i = threadIdx.x; i < nb; i += kThreads) {
    a += partial[2 * i];
    b += partial[2 * i + 1];
  }
  sh[0][threadIdx.x] = a;
  sh[1][threadIdx.x] = b;
  __syncthreads();
#pragma unroll
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = sh[0][0];
    out[1] = sh[1][0];
  }
}

constexpr int score_rt(int ks) { return ks <= 8 ? 4 : 2; }  // row tiles a wave keeps in registers

template <int KS, bool F8>
int launch_score(const void* X, long long n, long long ld, const int* label, const double* wt, const u16* tab,
                 const float* kappa, const float* mean, const double* Wc, int KT, int cosine, double* partial,
                 double* out, float* o_own, float* o_b, int* o_nb, float* o_s, hipStream_t st) {
  constexpr int RT = score_rt(KS);
  const long long nb = (n + kWaves * 16 * RT - 1) / (kWaves * 16 * RT);
  const size_t lds = ScoreCfg<KS>::LDS;
  (void)hipFuncSetAttribute((const void*)silhouette_score_kernel<KS, RT, F8>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((silhouette_score_kernel<KS, RT, F8>), dim3((unsigned)nb), dim3(kThreads), lds, st, X, n, ld,
                     label, wt, tab, kappa, mean, Wc, KT, cosine, partial, o_own, o_b, o_nb, o_s);
  hipLaunchKernelGGL(silhouette_final_kernel, dim3(1), dim3(kThreads), 0, st, partial, nb, out);
  return cml_status();
}

}  // namespace

// dtype: 0 = bf16 rows, 3 = e4m3 rows (the codes of the other launchers). ld in elements, ld % 8 == 0.
CML_API int cml_row_sqnorm_f64(const void* X, long long n, long long ld, int dtype, double* out, void* stream) {
  if (n < 1 || ld < 8 || ld % 8 != 0 || (dtype != 0 && dtype != 3)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const long long nb = (n + kThreads / 16 - 1) / (kThreads / 16);
  if (dtype == 3) hipLaunchKernelGGL(row_sqnorm_kernel<true>, dim3((unsigned)nb), dim3(kThreads), 0, st, X, n, ld, out);
  else hipLaunchKernelGGL(row_sqnorm_kernel<false>, dim3((unsigned)nb), dim3(kThreads), 0, st, X, n, ld, out);
  return cml_status();
}

// S [K][dp] f64, zero-filled by the caller. slab / perm: the labels in ascending order and the row of every
// position (a stable sort); off [K + 1]: the first position of every cluster; omega: per-row f64 factor or
// null; L: positions per unit; head, tail [ceil(n / L)][dp] f64 and hl [ceil(n / L)][2] i32 scratch.
CML_API int cml_label_wsum(const void* X, long long n, long long ld, int dp, int dtype, const int* slab,
                           const long long* perm, const long long* off, const double* omega, int K, int L, double* S,
                           double* head, double* tail, int* hl, void* stream) {
  if (n < 1 || K < 1 || L < 1 || dp < 16 || dp > 512 || (dp & (dp - 1)) != 0 || ld < dp || (dtype != 0 && dtype != 3))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int tpu = dp / 2;
  const long long nunits = (n + L - 1) / L;
  const int upb = kThreads / tpu;
  const long long nb = (nunits + upb - 1) / upb;
  if (dtype == 3)
    hipLaunchKernelGGL(label_wsum_kernel<true>, dim3((unsigned)nb), dim3(kThreads), 0, st, X, n, ld, dp, slab, perm,
                       omega, L, nunits, tpu, S, head, tail, hl);
  else
    hipLaunchKernelGGL(label_wsum_kernel<false>, dim3((unsigned)nb), dim3(kThreads), 0, st, X, n, ld, dp, slab, perm,
                       omega, L, nunits, tpu, S, head, tail, hl);
  hipLaunchKernelGGL(label_wsum_combine_kernel, dim3((unsigned)K), dim3(kThreads), 0, st, off, L, dp, head, tail, hl,
                     S);
  return cml_status();
}

// Rows per workgroup of the score pass at padded width dpk (the caller sizes `partial` by it).
CML_API int cml_silhouette_rows_per_block(int dpk) { return kWaves * 16 * score_rt(dpk / 32); }

// X: bf16 (dtype 0, 16 <= ld <= 512) or e4m3 (dtype 3, ld in {256, 512}) rows, ld % 8 == 0; dpk = max(ld, 32)
// rounded up to a multiple of 32 is the width of the centre table tab [KT][3][16][dpk] (bf16 hi, mid, lo
// planes of nu, zero padded), kappa [16 KT] (+inf: dead or padding), mean [dpk] (zero for cosine), Wc [K] with
// 16 (KT - 1) < K <= 16 KT and 0 <= label < K. partial [ceil(n / rows_per_block)][2], out [2] = (sum w s, sum w).
// The per-row outputs (own, b f32; nb i32: -1 = no other live cluster; s f32) are optional, all or none.
CML_API int cml_silhouette_score(const void* X, long long n, long long ld, int dtype, const int* label,
                                 const double* wt, const void* tab, const float* kappa, const float* mean,
                                 const double* Wc, int KT, int dpk, int cosine, double* partial, double* out,
                                 float* o_own, float* o_b, int* o_nb, float* o_s, void* stream) {
  if (n < 1 || KT < 1 || KT > 64 || ld % 8 != 0 || ld < 16 || ld > 512 || dpk % 32 != 0 || dpk < ld || dpk >= ld + 32)
    return (int)hipErrorInvalidValue;
  if (dtype == 3 ? (ld != 256 && ld != 512) : dtype != 0) return (int)hipErrorInvalidValue;
  if ((o_own == nullptr) != (o_b == nullptr) || (o_own == nullptr) != (o_nb == nullptr) ||
      (o_own == nullptr) != (o_s == nullptr))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const u16* t = (const u16*)tab;
#define CML_SIL(KSV, F8V)                                                                                          \
  if (dpk == 32 * KSV && (dtype == 3) == F8V)                                                                      \
    return launch_score<KSV, F8V>(X, n, ld, label, wt, t, kappa, mean, Wc, KT, cosine, partial, out, o_own, o_b,   \
                                  o_nb, o_s, st);
  CML_SIL(1, false) CML_SIL(2, false) CML_SIL(4, false) CML_SIL(8, false) CML_SIL(16, false)
  CML_SIL(8, true) CML_SIL(16, true)
#undef CML_SIL
  return (int)hipErrorInvalidValue;
}
