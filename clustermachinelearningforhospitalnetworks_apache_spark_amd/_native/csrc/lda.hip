// K29: the variational E-step of online LDA on bf16 rows (gfx950).
//
// Per document x (a row of term counts), with beta = exp(E[log beta]) [k, V] and the prior alpha [k]:
//   e_j = exp(psi(gamma_j) - psi(sum gamma)),  phinorm_w = sum_j e_j beta_jw + 1e-100
//   sweep: gamma'_j = alpha_j + e_j sum_w (x_w / phinorm_w) beta_jw;  change = mean_j |gamma'_j - gamma_j|
// and the document stops after the sweep whose change is not > 1e-3 (so a NaN stops it), at the latest after
// 1000 sweeps. The fit form adds sstats[j][w] = sum_docs e_j x_w / phinorm_w from the final e and phinorm, and
// logphat[j] = sum_docs (psi(gamma_j) - psi(sum gamma)). Every value after the exact bf16 -> f64 widening is f64.
//
// A persistent workgroup of 256 threads (4 waves) keeps beta in LDS as f64 for the whole launch and walks a
// contiguous run of 64-document tiles. Per tile:
//   stage    the rows (through the row list where there is one) go to LDS as bf16, once; pad columns (>= d),
//            rows outside the matrix and documents past B are stored as 0. Inside a 16-term block the values
//            are stored in the order the sweeps read them: position 4 g + r holds term g + 4 r, so that lane
//            group g reads its four values with one 8-byte load.
//   phase A  a wave owns 16 documents, document = lane & 15, lane group g = lane >> 4, and sweeps them to
//            convergence on v_mfma_f64_16x16x4_f64 (operand layout: mfma64.h). Per 16-term block:
//            phinorm^T[term][doc] = beta^T e^T with the
//            lane's e_j (topics g + 4 s) as B; Q = x / phinorm in the accumulator registers, whose register r
//            holds term g + 4 r: exactly the B operand of K-step r of acc[topic][doc] += beta[topic][term] Q^T.
//            acc leaves gamma' with topics g + 4 r on the lane, again in B-operand order. Up to four term blocks
//            are in flight with accumulators of their own. sum gamma and |delta gamma| are sums over the four
//            lane groups of a document. A converged document is frozen; the wave leaves when none is active.
//   phase B  (fit form) after a barrier, term block tb belongs to wave tb & 3 for the whole launch, which keeps
//            sstats[topic][its terms] in accumulator registers: phinorm[doc][term] = e beta per 16 documents,
//            Q = x / phinorm as B and e^T from LDS as A, 4 documents of depth per MFMA.
// At the end a workgroup writes its partial [kp][dp] and its logphat partial; lda_fold_kernel adds the partials
// in workgroup order. No atomics, nothing of size B x V in global memory, the grid depends on (B, dp, k, CUs)
// only, and every loop is bounded by the sweep cap and by B. One workgroup per CU, or two where k <= 16 and two
// LDS images fit (dp <= 256): the second wave on each SIMD works while the first waits on its divisions, psi and
// LDS reads.
//
// beta in LDS is read in two patterns: lanes along terms with lane groups along topics (phinorm), and lanes
// along topics with lane groups along terms (acc). A ds_read_b64 is conflict free when the 32 lanes of a half
// wave fall on 32 distinct doubles mod 32. With rows of pitch max(dp, 32) doubles the term index is XORed with
// f(topic) = 2 (topic & 15) ^ 16 (topic & 1): in the first pattern the two topics of a half wave (g = 0, 1 or
// 2, 3) differ in bit 4 of f and the 16 terms fill the low four bits; in the second the 16 topics give 16
// distinct even f (bits 1..4 are topic bits 0, 1, 2 and 3 ^ 0) and the two terms g, g + 1 differ in bit 0.
#include "mfma64.h"

namespace {

constexpr int kLdThreads = 256;
constexpr int kLdTile = 64;  // documents per tile: 16 per wave
constexpr int kLdMaxSweeps = 1000;

__host__ __device__ constexpr int ld_kp(int k) { return k <= 16 ? 16 : 32; }
__host__ __device__ constexpr int ld_bp(int dp) { return dp < 32 ? 32 : dp; }  // f64 pitch of a beta row

// LDS bytes: beta kp bp, the e tile 64 (kp + 1), alpha kp, the logphat fold 4 kp (all f64), the rows 64 (dp + 8) bf16.
__host__ __device__ constexpr long long ld_lds_bytes(int dp, int k) {
  const int kp = ld_kp(k);
  return 8LL * ((long long)kp * ld_bp(dp) + kLdTile * (kp + 1) + kp + 4 * kp) + 2LL * kLdTile * (dp + 8);
}

__host__ __device__ constexpr bool ld_supported(int dp, int k) {
  if (dp < 16 || dp > 512 || (dp & (dp - 1)) != 0 || k < 2 || k > 32) return false;
  if (k > 16 && dp > 256) return false;
  return ld_lds_bytes(dp, k) <= kLdsPerCu;
}

// psi(x) for x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 10, two steps per division
// (1 / x + 1 / (x + 1) = (2 x + 1) / (x (x + 1)); at most 5 of them), then the asymptotic series through the B12
// term (the next term is below 1e-15 at x = 10).
__device__ __forceinline__ double ld_digamma(double x) {
  double s = 0.0;
#pragma unroll 1
  for (int i = 0; i < 5 && x < 10.0; ++i) {
    s += (2.0 * x + 1.0) / (x * (x + 1.0));
    x += 2.0;
  }
  const double r = 1.0 / x, r2 = r * r;
  const double p = r2 * (1.0 / 12.0 - r2 * (1.0 / 120.0 - r2 * (1.0 / 252.0 - r2 * (1.0 / 240.0 - r2 * (1.0 / 132.0 -
                   r2 * (691.0 / 32760.0))))));
  return log(x) - 0.5 * r - p - s;
}

// Two workgroups share a CU (two waves per SIMD, one hiding the other's VALU and LDS latency) where two LDS images
// fit and the kernel stays inside 256 registers without scratch: one topic tile, up to dp = 256.
__host__ __device__ constexpr int ld_wgs_per_cu(int dp, int k) {
  return k <= 16 && ld_lds_bytes(dp, k) <= 80 * 1024 ? 2 : 1;
}

template <int DP, int KT>
__global__ __launch_bounds__(kLdThreads, ld_wgs_per_cu(DP, 16 * KT)) void lda_estep_kernel(
    const u16* __restrict__ X, long long n, int d, int k, const long long* __restrict__ rows, long long B,
    const double* __restrict__ tab, const double* __restrict__ alpha_g, const double* __restrict__ gamma0,
    double* __restrict__ gamma_out, int* __restrict__ sweeps_out, double* __restrict__ part, int fit) {
  constexpr int KP = 16 * KT;
  constexpr int NI = KP / 4;            // topics per lane: index i <-> topic 16 (i >> 2) + g + 4 (i & 3)
  constexpr int BP = ld_bp(DP);
  constexpr int XP = DP + 8;            // bf16 pitch of a staged row: 8-byte reads of 16 documents x 2 groups fall
                                        // on distinct doubles mod 32 (pitch / 4 = 2 mod 4 doubles)
  constexpr int EP = KP + 1;
  constexpr int NB = DP / 16;           // term blocks
  // term blocks in flight in a sweep: 4, and 2 at dp = 256 where two workgroups share the CU's registers
  constexpr int U = NB < 4 ? NB : (ld_wgs_per_cu(DP, KP) == 2 && DP >= 256 ? 2 : 4);
  constexpr int NBW = (NB + 3) / 4;     // term blocks per wave in phase B
  extern __shared__ __align__(16) unsigned char ld_smem[];
  double* beta = reinterpret_cast<double*>(ld_smem);  // [KP][BP], term index swizzled by the topic
  double* E = beta + KP * BP;                         // [64][EP]: the final e of the tile's documents
  double* al = E + kLdTile * EP;                      // [KP]
  double* red = al + KP;                              // [4][KP]
  u16* Xs = reinterpret_cast<u16*>(red + 4 * KP);     // [64][XP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;

  auto bsw = [](int topic, int term) { return topic * BP + unit_swizzle(topic, term); };

  for (int i = tid; i < KP * DP; i += kLdThreads) beta[bsw(i / DP, i % DP)] = tab[i];
  if (tid < KP) al[tid] = alpha_g[tid];

  int topic_of[NI];
  bool real[NI];
  double a_i[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    topic_of[i] = unit_of_lane(i, g);
    real[i] = topic_of[i] < k;
  }

  f64x4 ss[NBW][KT];
#pragma unroll
  for (int s = 0; s < NBW; ++s)
#pragma unroll
    for (int t = 0; t < KT; ++t) ss[s][t] = (f64x4)0.0;
  double lph[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) lph[i] = 0.0;

  const long long ntiles = (B + kLdTile - 1) / kLdTile;
  long long t0, t1;
  tile_run(ntiles, t0, t1);
  const double inv_k = 1.0 / (double)k;

  for (long long tile = t0; tile < t1; ++tile) {
    const long long base = tile * kLdTile;
    // ---- stage: one 16-term block of one document per item
    for (int item = tid; item < kLdTile * NB; item += kLdThreads) {
      const int doc = item / NB, tb = item % NB;
      const long long di = base + doc;
      uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;
      if (di < B) {
        const long long src = rows ? rows[di] : di;
        if (src >= 0 && src < n) {
          const uint4* p = reinterpret_cast<const uint4*>(X + src * DP + 16 * tb);
          lo = p[0];
          hi = p[1];
        }
      }
      // the same block as in mlp.hip and fm.hip: as a shared function it compiles to other machine code
      const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      unsigned v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const unsigned b = (u & 1) ? (w[u >> 1] >> 16) : (w[u >> 1] & 0xffffu);
        v[u] = 16 * tb + u < d ? b : 0u;  // the pad columns are masked by d, not trusted
      }
      uint2* out = reinterpret_cast<uint2*>(Xs + doc * XP + 16 * tb);
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) out[gg] = make_uint2(v[gg] | (v[gg + 4] << 16), v[gg + 8] | (v[gg + 12] << 16));
    }
    __syncthreads();  // also orders the beta / alpha stores before the first tile's reads

    // ---- phase A: this wave's 16 documents
    const long long di = base + wave * 16 + c;
    const bool valid = di < B;
    double gam[NI], et[NI], el[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      a_i[i] = al[topic_of[i] & (KP - 1)];
      gam[i] = valid && real[i] ? gamma0[di * k + topic_of[i]] : 1.0;
    }
    auto expectation = [&]() {
      double sg = 0.0;
#pragma unroll
      for (int i = 0; i < NI; ++i) sg += real[i] ? gam[i] : 0.0;
      const double ps = ld_digamma(lane_groups_sum(sg));
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        el[i] = real[i] ? ld_digamma(gam[i]) - ps : 0.0;
        et[i] = real[i] ? exp(el[i]) : 0.0;
      }
    };
    expectation();
    bool active = valid;
    int nsweeps = 0;
    const u16* xrow = Xs + (wave * 16 + c) * XP + 4 * g;
    for (int it = 0; it < kLdMaxSweeps; ++it) {
      if (__ballot(active) == 0ull) break;
      f64x4 acc[U][KT];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int t = 0; t < KT; ++t) acc[u][t] = (f64x4)0.0;
#pragma unroll 1
      for (int tb0 = 0; tb0 < NB; tb0 += U) {
        f64x4 D[U];
#pragma unroll
        for (int u = 0; u < U; ++u) D[u] = (f64x4)0.0;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int u = 0; u < U; ++u)
            D[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(beta[bsw(topic_of[i], 16 * (tb0 + u) + c)], et[i], D[u], 0,
                                                        0, 0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint2 xv = *reinterpret_cast<const uint2*>(xrow + 16 * (tb0 + u));
          D[u][0] = bf16hi_to_f64(xv.x << 16) / (D[u][0] + 1e-100);
          D[u][1] = bf16hi_to_f64(xv.x & 0xffff0000u) / (D[u][1] + 1e-100);
          D[u][2] = bf16hi_to_f64(xv.y << 16) / (D[u][2] + 1e-100);
          D[u][3] = bf16hi_to_f64(xv.y & 0xffff0000u) / (D[u][3] + 1e-100);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int u = 0; u < U; ++u)
              acc[u][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(beta[bsw(16 * t + c, 16 * (tb0 + u) + g + 4 * s)],
                                                              D[u][s], acc[u][t], 0, 0, 0);
      }
      double ng[NI], ch = 0.0;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        double a = acc[0][i >> 2][i & 3];
#pragma unroll
        for (int u = 1; u < U; ++u) a += acc[u][i >> 2][i & 3];
        ng[i] = et[i] * a + a_i[i];
        ch += real[i] ? fabs(ng[i] - gam[i]) : 0.0;
      }
      ch = lane_groups_sum(ch) * inv_k;
      if (active) {
#pragma unroll
        for (int i = 0; i < NI; ++i) gam[i] = real[i] ? ng[i] : 1.0;
        expectation();
        ++nsweeps;
      }
      active = active && (ch > 1e-3);
    }
    if (valid) {
#pragma unroll
      for (int i = 0; i < NI; ++i)
        if (real[i]) gamma_out[di * k + topic_of[i]] = gam[i];
      if (g == 0) sweeps_out[di] = nsweeps;
    }

    // ---- phase B: the statistics of the tile
    if (fit) {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        E[(wave * 16 + c) * EP + topic_of[i]] = valid ? et[i] : 0.0;
        lph[i] += valid ? el[i] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int slot = 0; slot < NBW; ++slot) {
        const int tb = wave + 4 * slot;
        if (tb < NB) {
          f64x4 D[4];
#pragma unroll
          for (int dg = 0; dg < 4; ++dg) D[dg] = (f64x4)0.0;
#pragma unroll
          for (int i = 0; i < NI; ++i) {
            const double b = beta[bsw(topic_of[i], 16 * tb + c)];
#pragma unroll
            for (int dg = 0; dg < 4; ++dg)
              D[dg] = __builtin_amdgcn_mfma_f64_16x16x4f64(E[(16 * dg + c) * EP + topic_of[i]], b, D[dg], 0, 0, 0);
          }
          const int xpos = 16 * tb + 4 * (c & 3) + (c >> 2);
#pragma unroll
          for (int dg = 0; dg < 4; ++dg) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const unsigned xb = Xs[(16 * dg + g + 4 * r) * XP + xpos];
              D[dg][r] = bf16hi_to_f64(xb << 16) / (D[dg][r] + 1e-100);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
              for (int t = 0; t < KT; ++t)
                ss[slot][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(E[(16 * dg + g + 4 * s) * EP + 16 * t + c],
                                                                  D[dg][s], ss[slot][t], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();  // the row and e tiles are free for the next tile
  }

  if (fit) {
    double* pp = part + (long long)blockIdx.x * (KP * DP + KP);
#pragma unroll
    for (int slot = 0; slot < NBW; ++slot) {
      const int tb = wave + 4 * slot;
      if (tb < NB) {
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) pp[(16 * t + g + 4 * r) * DP + 16 * tb + c] = ss[slot][t][r];
      }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      double v = lph[i];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
      if (c == 0) red[wave * KP + topic_of[i]] = v;
    }
    __syncthreads();
    if (tid < KP) pp[KP * DP + tid] = ((red[tid] + red[KP + tid]) + red[2 * KP + tid]) + red[3 * KP + tid];
  }
}

// out[j * d + w] = sum of the partials' [j][w] in workgroup order, then logphat [k].
__global__ __launch_bounds__(256) void lda_fold_kernel(const double* __restrict__ part, int nparts, int kp, int dp,
                                                       int k, int d, double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long ns = (long long)k * d;
  if (e >= ns + k) return;
  const long long src = e < ns ? (e / d) * dp + e % d : (long long)kp * dp + (e - ns);
  const long long ps = (long long)kp * dp + kp;
  double s = 0.0;
  for (int b = 0; b < nparts; ++b) s += part[(long long)b * ps + src];
  out[e] = s;
}

__global__ __launch_bounds__(256) void lda_digamma_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                          long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = ld_digamma(in[i]);
}

template <int DP, int KT>
int ld_launch(int grid, hipStream_t st, const void* X, long long n, int d, int k, const long long* rows, long long B,
              const double* tab, const double* alpha, const double* gamma0, double* gamma, int* sweeps, double* part,
              int fit) {
  if constexpr (!ld_supported(DP, 16 * KT)) {
    return (int)hipErrorInvalidValue;
  } else {
    return cml_launch_lds(lda_estep_kernel<DP, KT>, grid, kLdThreads, ld_lds_bytes(DP, 16 * KT), st, (const u16*)X, n, d,
                          k, rows, B, tab, alpha, gamma0, gamma, sweeps, part, fit);
  }
}

template <int KT, typename... Args>
int ld_launch_dp(int dp, Args... a) {
  switch (dp) {
    case 16: return ld_launch<16, KT>(a...);
    case 32: return ld_launch<32, KT>(a...);
    case 64: return ld_launch<64, KT>(a...);
    case 128: return ld_launch<128, KT>(a...);
    case 256: return ld_launch<256, KT>(a...);
    case 512: return ld_launch<512, KT>(a...);
  }
  return (int)hipErrorInvalidValue;
}

}  // namespace

// LDS bytes of K29 at this padded width and k; 0 = outside the kernel's limits.
CML_API long long cml_lda_lds(int dp, int k) { return ld_supported(dp, k) ? ld_lds_bytes(dp, k) : 0; }

// Workgroups of a launch: a function of (B, dp, k, CUs) only. 0 = unsupported or no document. One workgroup per
// CU, two where two LDS images fit.
CML_API int cml_lda_grid(long long B, int dp, int k, int ncu) {
  if (!ld_supported(dp, k) || B <= 0) return 0;
  return (int)cml_grid_cap((B + kLdTile - 1) / kLdTile, ncu, ld_wgs_per_cu(dp, ld_kp(k)));
}

// X: bf16 [n, dp] contiguous; rows: i64 [B] (indices into X; one outside [0, n) reads as an empty document) or
// null for the first B rows; tab: f64 [kp, dp] = exp(E[log beta]) zero padded; alpha: f64 [kp] zero padded;
// gamma0, gamma: f64 [B, k]; sweeps: i32 [B]. fit != 0: part f64 [grid][kp dp + kp] scratch and out f64
// [k d + k] = sstats, then logphat.
CML_API int cml_lda_estep(const void* X, long long n, int dp, int d, int k, const long long* rows, long long B,
                          const double* tab, const double* alpha, const double* gamma0, double* gamma, int* sweeps,
                          double* part, int grid, double* out, int fit, int ncu, void* stream) {
  if (!ld_supported(dp, k) || d < 1 || d > dp || n < 0 || B <= 0 || (rows == nullptr && B > n) ||
      (reinterpret_cast<size_t>(X) & 15) != 0 || grid != cml_lda_grid(B, dp, k, ncu) ||
      (fit && (part == nullptr || out == nullptr)))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int rc = k <= 16 ? ld_launch_dp<1>(dp, grid, st, X, n, d, k, rows, B, tab, alpha, gamma0, gamma, sweeps, part, fit)
                         : ld_launch_dp<2>(dp, grid, st, X, n, d, k, rows, B, tab, alpha, gamma0, gamma, sweeps, part, fit);
  if (rc != 0 || !fit) return rc;
  const long long ne = (long long)k * d + k;
  return cml_launch_fold(lda_fold_kernel, ne, st, part, grid, ld_kp(k), dp, k, d, out);
}

// out[i] = the kernel's psi(in[i]), f64.
CML_API int cml_lda_digamma(const double* in, double* out, long long n, void* stream) {
  if (n <= 0) return 0;
  return cml_launch_fold(lda_digamma_kernel, n, (hipStream_t)stream, in, out, n);
}
