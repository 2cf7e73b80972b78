// K27 one restricted 2-means iteration of BisectingKMeans for bf16 / e4m3 rows in the to_device_matrix layout:
// every row of a divided node chooses between the node's two children and the children collect their
// statistics, in one read of the listed rows.
//
//   cml_bisect_step   The rows of the level are listed in (node slot, row) order (`perm`, `pslot`: a stable sort
//                     made once per level) and cut into units of L consecutive positions, as K26's label sums
//                     are. The dp/2 threads of a unit own one column pair each and walk the unit in batches of
//                     8 rows whose loads are in flight together. The label is not given, it is decided in
//                     flight: a thread keeps its column pair of delta = c_R - c_L of the row's node in registers
//                     (reloaded when the slot changes), the batch's 8 partial dot products x·delta are reduced
//                     over the unit's threads (a butterfly of lane exchanges within a wave, LDS across waves:
//                     one barrier per batch) and every thread of the unit sees the same bits, so all take the
//                     same side:
//                       euclidean  right iff 2 x·delta > |c_R|^2 - |c_L|^2   (= |x - c_R|^2 < |x - c_L|^2)
//                       cosine     right iff   x·delta > 0                   (= 1 - x·c_R/|x| < 1 - x·c_L/|x|)
//                     left on ties; a dead child never wins; a node without a live child keeps its rows out
//                     of the statistics. Each thread then adds omega·x of its column pair to the left or the
//                     right accumulator (the other side gets + 0·x, which changes no bit), and the first three
//                     threads of the unit carry W = sum w, Q = sum w |x|^2 and N = rows the same way.
//                     A node that begins and ends inside one unit is written to `stats` directly; the first and
//                     the last segment of a unit go to head / tail partials.
//   combine launch    adds the head / tail partials of the units a node's rows span, in a fixed order.
//
// All arithmetic is f64 on the exact widening of the bf16 / e4m3 values; there are no atomics and nothing
// depends on workgroup scheduling: the order of every addition is fixed by (perm, L), so two calls return the
// same bits. With want_sums = 0 only the choices are written.
//
// Rounding of the decision (u = 2^-53, recursive sums of dp terms): the computed 2 x·delta - thr differs from
// d_L - d_R by at most 2 (dp + 2) u (|x|^2 + (|c_L|^2 + |c_R|^2) / 2) for euclidean and the computed
// x·delta / |x| by at most (dp + 2) u · 2 for cosine; tests/test_bisect_step_gpu.py allows choices to differ
// from an f64 oracle inside four times these bands only.
#include "mfma64.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBatch = 8;  // rows whose loads are in flight together

// 168 registers fit three waves per SIMD (the kernel is bound by the row gather: more waves, more loads in
// flight); four would spill the batch.
template <bool F8>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3))) void bisect_step_kernel(
    const void* __restrict__ Xv, long long ld, int dp, long long npos, const long long* __restrict__ perm,
    const int* __restrict__ pslot, const double* __restrict__ omega, const double* __restrict__ wt,
    const double* __restrict__ nrm2, const double* __restrict__ delta /*[m][dp]*/,
    const double* __restrict__ thr /*[m]*/, const int* __restrict__ alive /*[m][2]*/, int L, long long nunits,
    int tpu, int cosine, int want_sums, unsigned char* __restrict__ choice /*[npos]*/,
    double* __restrict__ stats /*[2m][dp+3]*/, double* __restrict__ head /*[nunits][2][dp+3]*/,
    double* __restrict__ tail /*[nunits][2][dp+3]*/, int* __restrict__ hl /*[nunits][2]*/) {
  __shared__ double red[2][kWaves][kBatch];
  const long long unit = (long long)blockIdx.x * (kThreads / tpu) + threadIdx.x / tpu;
  const int p = threadIdx.x % tpu;  // column pair 2p, 2p + 1
  const bool valid = unit < nunits;
  const unsigned char* X = reinterpret_cast<const unsigned char*>(Xv);
  // every thread of the workgroup runs the same number of batches (the barrier below); a unit past the end and
  // the positions past a unit's end load nothing
  const long long i0 = valid ? unit * L : 0;
  const long long i1 = valid ? (i0 + L < npos ? i0 + L : npos) : 0;
  const int w = dp + 3;          // a statistics row: [S | W | Q | N]
  const int lanes = tpu < 64 ? tpu : 64;
  const int wave = threadIdx.x >> 6;
  const int wpu = tpu > 64 ? tpu / 64 : 1;  // waves per unit
  const int wbase = (threadIdx.x / tpu) * wpu;

  int dslot = -1;  // the slot whose delta is in registers
  double d0 = 0.0, d1 = 0.0;
  const int first = (i0 < i1) ? pslot[i0] : -1;
  int cur = first;  // the slot whose sums are in the accumulators
  double t_cur = 0.0;
  bool al_cur = false, ar_cur = false;
  if (cur >= 0) {
    t_cur = thr[cur];
    al_cur = alive[2 * cur] != 0;
    ar_cur = alive[2 * cur + 1] != 0;
  }
  bool in_head = true;
  double aL0 = 0.0, aL1 = 0.0, aR0 = 0.0, aR1 = 0.0, xL = 0.0, xR = 0.0;  // x*: W (p = 0), Q (p = 1), N (p = 2)

  const int nbatch = L / kBatch;
  for (int b = 0; b < nbatch; ++b) {
    const long long ib = i0 + (long long)b * kBatch;
    int c[kBatch];
    double om[kBatch], aux[kBatch], s[kBatch];
    unsigned xv[kBatch];  // the column pair as two bf16
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      const long long i = ib + k;
      const bool ok = i < i1;
      c[k] = ok ? pslot[i] : -1;
      const long long r = ok ? perm[i] : 0;
      om[k] = ok ? (omega != nullptr ? omega[r] : 1.0) : 0.0;
      double a = 0.0;
      if (ok && want_sums) {
        if (p == 0) a = wt != nullptr ? wt[r] : 1.0;
        else if (p == 1) a = cosine ? 0.0 : (wt != nullptr ? wt[r] : 1.0) * nrm2[r];
        else if (p == 2) a = 1.0;
      }
      aux[k] = a;
      if constexpr (F8) {
        const unsigned q = ok ? *reinterpret_cast<const u16*>(X + r * ld + 2 * p) : 0u;
        const unsigned v = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q, 1.0f, false));
        xv[k] = v;
      } else {
        xv[k] = ok ? *reinterpret_cast<const unsigned*>(X + (r * ld + 2 * p) * 2) : 0u;
      }
    }
    // partial dot products with the delta of every row's own node
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      if (c[k] >= 0 && c[k] != dslot) {
        dslot = c[k];
        d0 = delta[(long long)dslot * dp + 2 * p];
        d1 = delta[(long long)dslot * dp + 2 * p + 1];
      }
      s[k] = bf16hi_to_f64(xv[k] << 16) * d0 + bf16hi_to_f64(xv[k] & 0xffff0000u) * d1;
    }
    // over the unit's threads: a butterfly inside the wave (every lane ends with the same bits) ...
    for (int o = 1; o < lanes; o <<= 1) {
#pragma unroll
      for (int k = 0; k < kBatch; ++k) s[k] += __shfl_xor(s[k], o, 64);
    }
    // ... and the unit's waves in wave order through LDS (double-buffered: one barrier per batch)
    if (tpu > 64) {
      if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kBatch; ++k) red[b & 1][wave][k] = s[k];
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kBatch; ++k) {
        double t = red[b & 1][wbase][k];
        for (int j = 1; j < wpu; ++j) t += red[b & 1][wbase + j][k];
        s[k] = t;
      }
    }
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      if (c[k] < 0) break;  // past the unit's end
      if (c[k] != cur) {
        if (want_sums) {
          double* dst = in_head ? head + unit * 2 * w : stats + (long long)cur * 2 * w;
          dst[2 * p] = aL0;
          dst[2 * p + 1] = aL1;
          dst[w + 2 * p] = aR0;
          dst[w + 2 * p + 1] = aR1;
          if (p < 3) {
            dst[dp + p] = xL;
            dst[w + dp + p] = xR;
          }
        }
        in_head = false;
        aL0 = aL1 = aR0 = aR1 = xL = xR = 0.0;
        cur = c[k];
        t_cur = thr[cur];
        al_cur = alive[2 * cur] != 0;
        ar_cur = alive[2 * cur + 1] != 0;
      }
      const bool go = ar_cur && (!al_cur || 2.0 * s[k] > t_cur);
      if (p == 0) choice[ib + k] = go ? 1 : 0;
      if (want_sums && (al_cur || ar_cur)) {
        const double wl = go ? 0.0 : om[k], wr = go ? om[k] : 0.0;
        const double x0 = bf16hi_to_f64(xv[k] << 16), x1 = bf16hi_to_f64(xv[k] & 0xffff0000u);
        aL0 += wl * x0;
        aL1 += wl * x1;
        aR0 += wr * x0;
        aR1 += wr * x1;
        xL += go ? 0.0 : aux[k];
        xR += go ? aux[k] : 0.0;
      }
    }
  }
  if (!valid || !want_sums || cur < 0) return;
  double* dst = (in_head ? head : tail) + unit * 2 * w;
  dst[2 * p] = aL0;
  dst[2 * p + 1] = aL1;
  dst[w + 2 * p] = aR0;
  dst[w + 2 * p + 1] = aR1;
  if (p < 3) {
    dst[dp + p] = xL;
    dst[w + dp + p] = xR;
  }
  if (p == 0) {
    hl[2 * unit] = first;
    hl[2 * unit + 1] = in_head ? -1 : cur;
  }
}

// The head / tail partials (both children) of the units a node's rows span. A node that spans many units (the
// root's children hold every row) would make one thread walk all of them, so a workgroup takes 16 columns of one
// node and its 16 phases take the units u0 + phase, u0 + phase + 16, ... in order; the 16 phase sums are then
// added in phase order. Which partial of a unit is the node's follows from the unit's place: every unit after
// the node's first holds the node at its head; the first holds it at its tail unless the node begins the unit.
constexpr int kCols = 16, kPhases = kThreads / kCols;

__global__ __launch_bounds__(kThreads) void bisect_combine_kernel(const long long* __restrict__ off /*[m+1]*/, int L,
                                                                  int w2 /*2 (dp + 3)*/,
                                                                  const double* __restrict__ head,
                                                                  const double* __restrict__ tail,
                                                                  const int* __restrict__ hl,
                                                                  double* __restrict__ stats) {
  __shared__ double part[kPhases][kCols];
  const int c = blockIdx.x;
  const int jj = threadIdx.x % kCols, ph = threadIdx.x / kCols;
  const int j = blockIdx.y * kCols + jj;
  const long long s = off[c], e = off[c + 1];
  if (s >= e) return;  // no row: the statistics stay zero
  const long long u0 = s / L, u1 = (e - 1) / L;
  const bool h0 = hl[2 * u0] == c;
  if (u0 == u1 && !h0 && hl[2 * u0 + 1] != c) return;  // the node lay inside one unit and is already written
  double acc = 0.0;
  if (j < w2) {
    for (long long u = u0 + ph; u <= u1; u += kPhases) acc += ((u == u0 && !h0) ? tail : head)[u * w2 + j];
  }
  part[ph][jj] = acc;
  __syncthreads();
  if (ph == 0 && j < w2) {
    double t = part[0][jj];
#pragma unroll
    for (int q = 1; q < kPhases; ++q) t += part[q][jj];
    stats[(long long)c * w2 + j] = t;
  }
}

}  // namespace

// X: bf16 (dtype 0, dp in 16..512, a power of two) or e4m3 (dtype 3, dp in {256, 512}) rows, ld >= dp elements.
// perm [npos] (rows, each < n), pslot [npos] (ascending, each in [0, m)), off [m + 1]: the plan of the level.
// omega, wt, nrm2: f64 per ROW or null (1, 1; nrm2 is required for euclidean sums). delta [m][dp] = c_R - c_L,
// thr [m] = |c_R|^2 - |c_L|^2 (0 for cosine), alive [m][2]. L: positions per unit, a multiple of 8.
// choice [npos]; with want_sums: stats [2m][dp + 3] zero-filled by the caller, head, tail [ceil(npos / L)][2][dp + 3]
// and hl [ceil(npos / L)][2] scratch.
CML_API int cml_bisect_step(const void* X, long long n, long long ld, int dp, int dtype, long long npos,
                            const long long* perm, const int* pslot, const long long* off, const double* omega,
                            const double* wt, const double* nrm2, const double* delta, const double* thr,
                            const int* alive, int m, int L, int cosine, int want_sums, unsigned char* choice,
                            double* stats, double* head, double* tail, int* hl, void* stream) {
  if (npos == 0) return 0;
  if (n < 1 || npos < 0 || m < 1 || L < kBatch || L % kBatch != 0 || dp < 16 || dp > 512 || (dp & (dp - 1)) != 0 ||
      ld < dp)
    return (int)hipErrorInvalidValue;
  if (dtype == 3 ? (dp != 256 && dp != 512) : dtype != 0) return (int)hipErrorInvalidValue;
  if (perm == nullptr || pslot == nullptr || off == nullptr || delta == nullptr || thr == nullptr ||
      alive == nullptr || choice == nullptr)
    return (int)hipErrorInvalidValue;
  if (want_sums && (stats == nullptr || head == nullptr || tail == nullptr || hl == nullptr ||
                    (!cosine && nrm2 == nullptr)))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int tpu = dp / 2;
  const long long nunits = (npos + L - 1) / L;
  const int upb = kThreads / tpu;
  const long long nb = (nunits + upb - 1) / upb;
  if (nb > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (dtype == 3)
    hipLaunchKernelGGL(bisect_step_kernel<true>, dim3((unsigned)nb), dim3(kThreads), 0, st, X, ld, dp, npos, perm,
                       pslot, omega, wt, nrm2, delta, thr, alive, L, nunits, tpu, cosine, want_sums, choice, stats,
                       head, tail, hl);
  else
    hipLaunchKernelGGL(bisect_step_kernel<false>, dim3((unsigned)nb), dim3(kThreads), 0, st, X, ld, dp, npos, perm,
                       pslot, omega, wt, nrm2, delta, thr, alive, L, nunits, tpu, cosine, want_sums, choice, stats,
                       head, tail, hl);
  if (want_sums)
    hipLaunchKernelGGL(bisect_combine_kernel, dim3((unsigned)m, (unsigned)((2 * (dp + 3) + kCols - 1) / kCols)),
                       dim3(kThreads), 0, st, off, L, 2 * (dp + 3), head,
                       tail, hl, stats);
  return cml_status();
}
