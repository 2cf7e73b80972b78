// K10w: weighted per-cluster sums of bf16 / e4m3 rows for the MFMA KMeans path (weightCol).
//
// The weighted Lloyd step keeps K9 / K9r as they are (weights do not enter the assignment) and replaces
// the segmented f64 sums of kmeans_segacc (kmeans.hip) by sums of the PRODUCTS w_i·x_ij. Those are not
// on a grid, so plain f64 sums would depend on the order of the additions; the project's weighted sums
// are defined instead as the exact sum of the rounded products fl64(w_i·x_ij), correctly rounded
// (kmeans_exact.hip exact_seg_partial_kernel on the f64 array [w·x | w]). This kernel computes the same
// bits straight from the rows in the kernels' own layout: every raw value widens exactly to f64, one
// f64 multiply rounds the product, and a double-double accumulator (exact_util.h dd_add) takes it.
//
// Per cluster c the output rows S / S_lo [k, D + 2] (normalised double-double, S + S_lo = the exact sum):
//   columns 0..D-1  Σ fl64(w_i · x_ij)
//   column  D       Σ w_i
//   column  D+1     Σ fl64(w_i · xn64_i)     (xn64: the row pass's f64 ||x_i||², for the lazy cost)
// over the rows i with label c. Exact — so independent of the order, of the slicing below and of how
// rows are split over ranks — while the addends of a column span fewer than ~106 - 53 - ceil(log2 n)
// binary orders; beyond that still deterministic for a fixed launch shape.
//
// Structure (kmeans_segacc's): one wave per slice of the label-sorted positions, U whole-row gathers
// in flight (CPL columns per lane), the next batch's row ids loaded one batch ahead, w[row] and
// xn64[row] gathered with the batch by lanes 0..U-1, flushes only at cluster boundaries. No atomics:
// a cluster inside one slice is stored by its wave; a slice's first and last clusters go to per-wave
// hi/lo slots, which kmeans_wseg_fix folds in slice order (exact_seg_fix_kernel's scheme).
//
// No contraction anywhere here: the product must round once before it is added.
#pragma clang fp contract(off)

#include "exact_util.h"

namespace {

constexpr int kWsThreads = 256;  // 4 waves

// Positions per wave slice (kmeans.hip seg_chunk): an even split, at least 128.
__device__ __forceinline__ long long wseg_chunk(long long filled, long long waves) {
  const long long c = (filled + waves - 1) / waves;
  return c > 128 ? c : 128;
}

template <int CPL, bool F8> struct WRaw;
template <> struct WRaw<2, false> { using T = unsigned; };
template <> struct WRaw<4, false> { using T = uint2; };
template <> struct WRaw<8, false> { using T = uint4; };
template <> struct WRaw<4, true> { using T = unsigned; };
template <> struct WRaw<8, true> { using T = uint2; };
template <> struct WRaw<16, true> { using T = uint4; };

__device__ __forceinline__ double bcast_f64(double v, int u) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), u);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), u);
  return __hiloint2double(hi, lo);
}

// acc += fl64(wu · x_j) over this lane's CPL columns of one raw row (bf16 pairs or e4m3 bytes).
template <int CPL, bool F8>
__device__ __forceinline__ void wadd_raw(double (&hi)[CPL], double (&lo)[CPL], const typename WRaw<CPL, F8>::T& r,
                                         double wu) {
  const unsigned* ws = reinterpret_cast<const unsigned*>(&r);
  if constexpr (F8) {
    typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int q = 0; q < CPL / 4; ++q) {
      const f2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)ws[q], false);
      const f2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)ws[q], true);
      dd_add(hi[4 * q], lo[4 * q], __dmul_rn(wu, (double)a.x));
      dd_add(hi[4 * q + 1], lo[4 * q + 1], __dmul_rn(wu, (double)a.y));
      dd_add(hi[4 * q + 2], lo[4 * q + 2], __dmul_rn(wu, (double)b.x));
      dd_add(hi[4 * q + 3], lo[4 * q + 3], __dmul_rn(wu, (double)b.y));
    }
  } else {
#pragma unroll
    for (int q = 0; q < CPL / 2; ++q) {
      dd_add(hi[2 * q], lo[2 * q], __dmul_rn(wu, (double)bf16_to_f32((u16)(ws[q] & 0xffffu))));
      dd_add(hi[2 * q + 1], lo[2 * q + 1], __dmul_rn(wu, (double)bf16_to_f32((u16)(ws[q] >> 16))));
    }
  }
}

// Slots: hi partials f64 [2·waves, DO] then lo partials [2·waves, DO] (DO = D + 2); slot 2w is wave w's
// first flushed cluster, 2w+1 its last; slot_c their cluster ids (-1: none).
template <int CPL, bool F8, int U>
__global__ __launch_bounds__(kWsThreads, (CPL <= 4 ? 4 : 1)) void kmeans_wsegacc(
    const void* __restrict__ X, long long n, long long ldx, int Dp, int D, const double* __restrict__ w,
    const double* __restrict__ xn64, const int* __restrict__ perm, const int* __restrict__ seg, int k,
    double* __restrict__ S, double* __restrict__ S_lo, double* __restrict__ slots, int* __restrict__ slot_c) {
  using raw_t = typename WRaw<CPL, F8>::T;
  static_assert(U <= 16, "row ids of a batch sit in lanes 0..U-1");
  const unsigned char* xb = reinterpret_cast<const unsigned char*>(X);
  constexpr int ESZ = F8 ? 1 : 2;  // bytes per element
  const int DO = D + 2;
  const int lane = threadIdx.x & 63;
  const long long waves = (long long)gridDim.x * (kWsThreads / 64);
  const long long wave = (long long)blockIdx.x * (kWsThreads / 64) + (threadIdx.x >> 6);
  n = n < (long long)seg[k] ? n : (long long)seg[k];
  const long long chunk = wseg_chunk(n, waves);
  const long long p0 = wave * chunk;
  if (p0 >= n) {
    if (lane == 0) {
      slot_c[2 * wave] = -1;
      slot_c[2 * wave + 1] = -1;
    }
    return;
  }
  double* slotA = slots + (2 * wave) * (long long)DO;
  double* slotB = slotA + DO;
  const long long lo_off = 2 * waves * (long long)DO;  // hi -> lo half of the slot scratch
  int nflush = 0;
  const long long p1 = p0 + chunk < n ? p0 + chunk : n;
  int lo_ = 0, hi_ = k;  // invariant: seg[lo_] <= p0 < seg[hi_]
  while (hi_ - lo_ > 1) {
    const int mid = (lo_ + hi_) >> 1;
    if (seg[mid] <= p0) lo_ = mid; else hi_ = mid;
  }
  int c = lo_;
  long long next = seg[c + 1];
  while (next <= p0 && c < k - 1) { ++c; next = seg[c + 1]; }  // skip empty clusters
  const int col = CPL * lane;
  const bool active = col < Dp;
  double ah[CPL], al[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) { ah[j] = 0.0; al[j] = 0.0; }
  // Σ w and Σ w·xn64: lane u < U accumulates the batch's row u; the lanes are folded at a flush
  double wh = 0.0, wl = 0.0, qh = 0.0, ql = 0.0;
  // the running sums (normalised) into dh / dl (row of S / S_lo, or a slot and its lo twin), then cleared
  auto flush = [&](double* dh, double* dl) {
    if (active) {
#pragma unroll
      for (int j = 0; j < CPL; ++j)
        if (col + j < D) {
          double h = ah[j], l = al[j];
          dd_norm(h, l);
          dh[col + j] = h;
          dl[col + j] = l;
        }
    }
#pragma unroll
    for (int j = 0; j < CPL; ++j) { ah[j] = 0.0; al[j] = 0.0; }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {  // lanes 0..15 hold the partials (U <= 16)
      const double oh = __shfl_xor(wh, o, 64), ol = __shfl_xor(wl, o, 64);
      const double ph = __shfl_xor(qh, o, 64), pl = __shfl_xor(ql, o, 64);
      dd_add(wh, wl, oh);
      wl += ol;
      dd_add(qh, ql, ph);
      ql += pl;
    }
    if (lane == 0) {
      dd_norm(wh, wl);
      dd_norm(qh, ql);
      dh[D] = wh;
      dl[D] = wl;
      dh[D + 1] = qh;
      dl[D + 1] = ql;
    }
    wh = wl = qh = ql = 0.0;
  };
  // the next batch's row ids are loaded one batch ahead (kmeans_segacc): one memory round trip per batch
  int pr_next = (lane < U && p0 + lane < p1) ? perm[p0 + lane] : 0;
  for (long long p = p0; p < p1; p += U) {
    const int cnt = (int)(p1 - p < U ? p1 - p : U);
    const int pr = pr_next;
    pr_next = (lane < U && p + U + lane < p1) ? perm[p + U + lane] : 0;
    // the batch's weights and norm products, one row per lane (0 past the batch's end)
    double wv = 0.0, qv = 0.0;
    if (lane < cnt) {
      wv = w[pr];
      qv = __dmul_rn(wv, xn64[pr]);
    }
    const long long pe = p + cnt;
    if (next >= pe) {
      raw_t r[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long row = __builtin_amdgcn_readlane(pr, u);
        if (u < cnt && active) {
          r[u] = *reinterpret_cast<const raw_t*>(xb + (row * ldx + col) * ESZ);
        } else {
          r[u] = raw_t{};
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) wadd_raw<CPL, F8>(ah, al, r[u], bcast_f64(wv, u));  // rows past cnt: w = 0, x = 0
      dd_add(wh, wl, wv);
      dd_add(qh, ql, qv);
    } else {
      // a cluster boundary inside this batch (~k + #waves batches per pass): its rows one at a time
#pragma unroll 1
      for (int u = 0; u < cnt; ++u) {
        const long long pos = p + u;
        while (pos >= next) {  // cluster c ended before pos
          if (nflush == 0) {
            flush(slotA, slotA + lo_off);
            if (lane == 0) slot_c[2 * wave] = c;
          } else {  // later clusters are this wave's alone
            flush(S + (long long)c * DO, S_lo + (long long)c * DO);
          }
          ++nflush;
          ++c;
          next = seg[c + 1];
          while (next <= pos && c < k - 1) { ++c; next = seg[c + 1]; }
        }
        const long long row = __builtin_amdgcn_readlane(pr, u);
        raw_t v = raw_t{};
        if (active) v = *reinterpret_cast<const raw_t*>(xb + (row * ldx + col) * ESZ);
        wadd_raw<CPL, F8>(ah, al, v, bcast_f64(wv, u));
        if (lane == u) {
          dd_add(wh, wl, wv);
          dd_add(qh, ql, qv);
        }
      }
    }
  }
  flush(slotB, slotB + lo_off);
  if (lane == 0) {
    if (nflush == 0) slot_c[2 * wave] = -1;
    slot_c[2 * wave + 1] = c;
  }
}

// S[c] / S_lo[c] of the clusters that touch a slice edge: their slot partials (double-double) folded in
// slice order; empty clusters get zeros. One workgroup per cluster.
__global__ __launch_bounds__(256) void kmeans_wseg_fix(const int* __restrict__ seg, int k, int D, long long n,
                                                       long long nwaves, double* __restrict__ S,
                                                       double* __restrict__ S_lo, const double* __restrict__ slots,
                                                       const int* __restrict__ slot_c) {
  const int c = blockIdx.x;
  const int DO = D + 2;
  const long long s0 = seg[c], s1 = seg[c + 1];
  if (s1 <= s0) {
    for (int t = threadIdx.x; t < DO; t += blockDim.x) {
      S[(long long)c * DO + t] = 0.0;
      S_lo[(long long)c * DO + t] = 0.0;
    }
    return;
  }
  const long long chunk = wseg_chunk(n < (long long)seg[k] ? n : (long long)seg[k], nwaves);  // as kmeans_wsegacc
  const long long w0 = s0 / chunk;
  long long w1 = (s1 - 1) / chunk;
  if (w1 >= nwaves) w1 = nwaves - 1;
  const double* slots_lo = slots + 2 * nwaves * (long long)DO;
  bool edge = false;
  for (long long ww = w0; ww <= w1; ++ww) edge |= slot_c[2 * ww] == c || slot_c[2 * ww + 1] == c;
  if (!edge) return;  // complete inside one slice: stored by its wave
  for (int t = threadIdx.x; t < DO; t += blockDim.x) {
    double h = 0.0, l = 0.0;
    for (long long ww = w0; ww <= w1; ++ww) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (slot_c[2 * ww + q] == c) {
          dd_add(h, l, slots[(2 * ww + q) * (long long)DO + t]);
          l += slots_lo[(2 * ww + q) * (long long)DO + t];
        }
      }
    }
    dd_norm(h, l);
    S[(long long)c * DO + t] = h;
    S_lo[(long long)c * DO + t] = l;
  }
}

}  // namespace

// Doubles / ints of the slot scratch of a launch of seg_grid workgroups.
CML_API long long cml_kmeans_wseg_slot_doubles(int seg_grid, int D) {
  return 4LL * seg_grid * (kWsThreads / 64) * (D + 2);
}
CML_API long long cml_kmeans_wseg_slot_ints(int seg_grid) { return 2LL * seg_grid * (kWsThreads / 64); }

// S, S_lo: f64 [k, D + 2]; w, xn64: f64 [>= rows]; perm: int [n] row ids in label order; seg: int [k + 1] first
// sorted position of every cluster (seg[k] = n). cpl: columns per lane (bf16 2/4/8, e4m3 4/8/16; 64·cpl >= Dp).
CML_API int cml_kmeans_weighted_segsum(const void* X, long long n, long long ldx, int Dp, int D, int xfp8,
                                       const double* w, const double* xn64, const int* perm, const int* seg, int k,
                                       int cpl, int seg_grid, double* S, double* S_lo, double* slots, int* slot_c,
                                       void* stream) {
  if (D <= 0 || D > Dp || k <= 0 || n < 0 || seg_grid <= 0 || 64LL * cpl < Dp || ldx < Dp) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const long long waves = (long long)seg_grid * (kWsThreads / 64);
#define CML_WSEG(C, F, UU)                                                                                          \
  hipLaunchKernelGGL((kmeans_wsegacc<C, F, UU>), dim3(seg_grid), dim3(kWsThreads), 0, st, X, n, ldx, Dp, D, w, xn64, \
                     perm, seg, k, S, S_lo, slots, slot_c)
  if (xfp8) {
    if (cpl == 4) CML_WSEG(4, true, 16);
    else if (cpl == 8) CML_WSEG(8, true, 16);
    else if (cpl == 16) CML_WSEG(16, true, 16);
    else return (int)hipErrorInvalidValue;
  } else if (cpl == 2) CML_WSEG(2, false, 16);
  else if (cpl == 4) CML_WSEG(4, false, 16);
  else if (cpl == 8) CML_WSEG(8, false, 16);
  else return (int)hipErrorInvalidValue;
#undef CML_WSEG
  const int e = cml_status();
  if (e) return e;
  hipLaunchKernelGGL(kmeans_wseg_fix, dim3(k), dim3(256), 0, st, seg, k, D, n, waves, S, S_lo, slots, slot_c);
  return cml_status();
}
