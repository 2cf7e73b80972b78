// K33: one IRLS step of a generalized linear model over bf16 rows with 1 <= d <= 128 feature columns (gfx950).
//
// For a row r with label y, weight w (1 without one), offset off (0 without one) and the coefficients (beta, b0):
//   eta = x . beta + b0 + off        (f64 after the exact bf16 -> f64 widening; the init form takes eta = g(mu_init))
//   mu  = project(g^-1(eta)),  z = eta - off + (y - mu) g'(mu),  wt = w / (g'(mu)^2 V(mu))
// and the step form returns G = [X 1 z]^T diag(wt) [X 1 z] in K31's (d + 2, d + 2) layout together with the four
// sums stats = [sum w dev(y, mu), sum w (y - mu)^2 / V(mu), sum w y, sum w]: one read of the rows, nothing of size n
// written. A row with w == 0 (and every row past n) has z = wt = 0 and adds 0 to every sum, whatever its eta.
//
// The kernel is K31 (gram.hip) restricted to one 128-column panel, with the row terms made between the stage and
// the products. 256 threads (4 waves) own a contiguous run (slab) of 64-row tiles. Per tile:
//   stage    the 64 x 128 bf16 rows go to LDS, once; columns >= d and rows >= n are stored as 0 (pad columns may
//            hold NaN bits). The global loads of a tile are issued one tile ahead and wait in registers.
//   eta      lanes 4 r .. 4 r + 3 of the workgroup own row r: lane q adds the 4-column chunks q, q + 4, q + 8 ..
//            in that order with fma, against beta in LDS as f64 (zero past d); the four partial sums meet in a
//            two-step xor butterfly, (q0 + q1) + (q2 + q3) on every lane, and go to es[r]. The chunk of lane q of
//            row r sits at dword 72 r + 2 q + 8 k of the tile (pitch 128 + 16 bf16 = 72 dwords), so the 32 lanes of
//            a half wave (8 rows x 4 chunks) read 64 distinct dwords mod 64: no bank conflict on the ds_read_b64;
//            the beta reads are 4 distinct addresses per wave, broadcast.
//   terms    lane l of wave 2 owns row l of the tile (its y, w and off wait in registers like the rows): it calls
//            glr_row_terms, the one function that the step form and the rows form both use, writes z and wt to the
//            tile's zs / ws and keeps the row's four stat addends in registers. The link and the variance take
//            wave-uniform branches: p in {0, 1, 2, 3} and lp in {0, 1, -1, 0.5} need no pow.
//   products K31's diagonal-pair arrangement on v_mfma_f64_16x16x4_f64: waves 0, 1, 3 the X blocks with tile i <=
//            tile j (10 + 16 + 10), wave 2 the 8 (tile, U) blocks and (U, U), U = [1, z, 0 ..]; the B side is
//            multiplied by wt[row]. Blocks past ceil(d / 16) are skipped (wave-uniform masks).
// Wave 2 and the other three run two copies of the tile loop (the wave index is made provably uniform, so the
// barriers sit in scalar control flow and every wave passes the same four per tile): wave 2 holds 9 accumulators
// beside the registers of exp / log / pow, the others 16 and none of those.
// At the end of its run a workgroup writes its 64 block slots and, after a fixed-order sum over its 64 rows, its four
// stats beside them. glr_fold_kernel adds the slabs in slab order and mirrors. No atomics; the grid depends on
// (n, d, CUs) only; two calls give the same bits. The rows form (mode 2) writes eta, mu, z, wt per row instead; the
// stats form (mode 1) skips the products.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): glr_pass_kernel 250 VGPRs (of
// them 128 accumulators in waves 0, 1, 3) at __launch_bounds__(256, 2), no scratch, 23 040 B LDS (the tile
// 64 * 144 * 2 B, es / zs / ws 3 * 64 * 8 B, beta 128 * 8 B, the stat fold 64 * 4 * 8 B): two workgroups per CU.
// With the row terms on the row owners of all four waves, beside 16 accumulators, the same code needed 160 B of
// scratch per lane. glr_fold_kernel: no LDS, no scratch.
//
// Measured on an MI355X, one step for tweedie (1, log) with weights, best of 3 in three interleaved rounds
// (scripts/mb_ml.py glr_step), against one iteration of the poisson loop of ml/glr.py on the same rows (K24, nine
// torch element-wise kernels, K31):
//   10M x 64  bf16: K33 3.85 ms (1.44 GB read, 0.37 TB/s), the loop 3.24 ms (4.72 GB moved, 1.46 TB/s)
//   10M x 128 bf16: K33 5.73 ms (2.72 GB read, 0.47 TB/s), the loop 5.45 ms (7.28 GB moved, 1.34 TB/s)
// K33 is not faster. Neither form is near the HBM rate; by the instruction counts (not profiled) a tile waits on the
// f64 MFMAs of the wave with the most blocks (all 10 X blocks on wave 0 at d = 64, 16 on wave 1 at d = 128), and
// here the dot products and the row terms of wave 2 come before the products instead of beside them. The two forms
// differ by up to 2e-4 relative in an entry of G: K24 makes eta in f32, K33 in f64.
#include "mfma64.h"

// No contraction in this file: the row terms are the same sequence of roundings wherever they are inlined (the eta
// dot product names its fmas).
#pragma clang fp contract(off)

namespace {

constexpr int kGlThreads = 256;
constexpr int kGlTile = 64;            // rows per tile
constexpr int kGlPanel = 128;          // columns of the one panel
constexpr int kGlXP = kGlPanel + 16;   // bf16 pitch of a staged row
constexpr int kGlSlots = 64;           // block slots of a workgroup: 16 per wave
constexpr int kGlPart = kGlSlots * 256 + 8;  // doubles of a slab's partial: the slots, 4 stats, 4 unused
constexpr int kGlMaxD = 128;

enum { kGlStep = 0, kGlStats = 1, kGlRows = 2 };
enum { kFamGaussian = 0, kFamBinomial = 1, kFamPoisson = 2, kFamGamma = 3, kFamTweedie = 4 };

// fam: whose initialisation, projection and deviance; var: 0 = mu^p, 1 = mu (1 - mu); link: 0 = mu^lp (log at 0),
// 1 = logit.
struct GlrSpec {
  int fam, var, link;
  double p, lp;
};

struct GlrRow {
  double eta, mu, z, wt, dev, pearson, wy, sw;
};

__device__ __forceinline__ double glr_pow(double x, double a) {
  if (a == 1.0) return x;
  if (a == 2.0) return x * x;
  if (a == 3.0) return x * x * x;
  if (a == -1.0) return 1.0 / x;
  if (a == -2.0) return 1.0 / (x * x);
  if (a == 0.5) return sqrt(x);
  if (a == -0.5) return 1.0 / sqrt(x);
  if (a == 0.0) return 1.0;
  return pow(x, a);
}

__device__ __forceinline__ double glr_ylogy(double a, double b) { return a > 0.0 ? a * log(a / b) : 0.0; }

// (y^a - mu^a) / a, log(y / mu) at a == 0
__device__ __forceinline__ double glr_yp(double y, double mu, double a) {
  return a == 0.0 ? log(y / mu) : (glr_pow(y, a) - glr_pow(mu, a)) / a;
}

// The terms of one row. `init`: mu from the family's initialisation and eta = g(mu); else mu = project(g^-1(eta)).
// ops/glr_ops.row_terms is the same sequence of operations in torch.
__device__ __forceinline__ GlrRow glr_row_terms(double eta, double y, double w, double off, const GlrSpec& s,
                                                bool init) {
  const double eps = 1e-16, big = 1.7976931348623157e308;
  const bool power = s.link == 0;
  double mu;
  if (init) {
    if (s.fam == kFamBinomial)
      mu = (w * y + 0.5) / (w + 1.0);
    else if (s.fam == kFamPoisson)
      mu = fmax(y, 0.1);
    else if (s.fam == kFamTweedie && s.p >= 1.0 && s.p < 2.0)
      mu = y == 0.0 ? 0.1 : y;
    else
      mu = y;
    if (!power)
      eta = log(mu / (1.0 - mu));
    else if (s.lp == 1.0)
      eta = mu;
    else if (s.lp == 0.0)
      eta = log(mu);
    else if (s.lp == -1.0)
      eta = 1.0 / mu;
    else if (s.lp == 0.5)
      eta = sqrt(mu);
    else
      eta = pow(mu, s.lp);
  } else {
    if (!power)
      mu = 1.0 / (1.0 + exp(-eta));
    else if (s.lp == 1.0)
      mu = eta;
    else if (s.lp == 0.0)
      mu = exp(eta);
    else if (s.lp == -1.0)
      mu = 1.0 / eta;
    else if (s.lp == 0.5)
      mu = eta * eta;
    else
      mu = pow(eta, 1.0 / s.lp);
    if (s.fam == kFamBinomial)
      mu = fmin(fmax(mu, eps), 1.0 - eps);
    else if (s.fam != kFamGaussian && !(s.fam == kFamTweedie && s.p == 0.0))  // tweedie with p = 0 is gaussian
      mu = fmin(fmax(mu, eps), big);
  }
  double gp;
  if (!power)
    gp = 1.0 / (mu * (1.0 - mu));
  else if (s.lp == 1.0)
    gp = 1.0;
  else if (s.lp == 0.0)
    gp = 1.0 / mu;
  else if (s.lp == -1.0)
    gp = -1.0 / (mu * mu);
  else if (s.lp == 0.5)
    gp = 0.5 / sqrt(mu);
  else
    gp = s.lp * pow(mu, s.lp - 1.0);
  const double V = s.var == 1 ? mu * (1.0 - mu) : glr_pow(mu, s.p);
  const double r = y - mu;
  double dev;
  if (s.fam == kFamGaussian)
    dev = r * r;
  else if (s.fam == kFamBinomial)
    dev = 2.0 * (glr_ylogy(y, mu) + glr_ylogy(1.0 - y, 1.0 - mu));
  else if (s.fam == kFamPoisson)
    dev = 2.0 * (glr_ylogy(y, mu) - r);
  else if (s.fam == kFamGamma)
    dev = 2.0 * (-log(y / mu) + r / mu);
  else {
    const double y1 = (s.p >= 1.0 && s.p < 2.0) ? fmax(y, 0.1) : y;
    dev = 2.0 * (y * glr_yp(y1, mu, 1.0 - s.p) - glr_yp(y, mu, 2.0 - s.p));
  }
  GlrRow o;
  const bool live = w != 0.0;
  o.eta = eta;
  o.mu = mu;
  o.z = live ? (eta - off) + r * gp : 0.0;
  o.wt = live ? w / ((gp * gp) * V) : 0.0;
  o.dev = live ? w * dev : 0.0;
  o.pearson = live ? (w * (r * r)) / V : 0.0;
  o.wy = live ? w * y : 0.0;
  o.sw = w;
  return o;
}

__global__ __launch_bounds__(kGlThreads, 2) void glr_pass_kernel(
    const u16* __restrict__ X, long long n, long long ldx, int wc, int d, const double* __restrict__ y,
    const double* __restrict__ w, const double* __restrict__ off, const double* __restrict__ coef, GlrSpec spec,
    int mode, double* __restrict__ part, double* __restrict__ rows_out) {
  __shared__ __align__(16) u16 Xs[kGlTile][kGlXP];
  __shared__ double es[kGlTile];
  __shared__ double zs[kGlTile];
  __shared__ double ws[kGlTile];
  __shared__ double bs[kGlPanel];
  __shared__ double ss[kGlTile][4];
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int erow = tid >> 2, eq = tid & 3;   // the row whose eta this lane helps with, and its part of it
  const bool init = coef == nullptr;
  const bool products = mode == kGlStep;
  const bool loadx = !init || products;      // the init form needs the rows for the products only
  const int nt = (d + 15) / 16;
  const int slab = blockIdx.x, nslabs = gridDim.x;

  if (tid < kGlPanel) bs[tid] = (!init && tid < d) ? coef[tid] : 0.0;
  const double b0 = init ? 0.0 : coef[d];

  const long long ntiles = (n + kGlTile - 1) / kGlTile;
  long long t0, t1;
  tile_run(ntiles, slab, nslabs, t0, t1);
  double* pu = part + (long long)slab * kGlPart;

  // One item = 8 bf16 of one row (16 bytes); a thread holds its 4 items of a tile in registers. The loads of tile + 1
  // are issued before the work on tile. wc is a multiple of 8, so a chunk is inside the row or not.
  uint4 pf[4];
  auto fetch = [&](long long tile) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int it = tid + kGlThreads * k, row = it >> 4, col = 8 * (it & 15);
      const long long r = tile * kGlTile + row;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (loadx && r < n && col < wc && col < d) v = *reinterpret_cast<const uint4*>(X + r * ldx + col);
      pf[k] = v;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int it = tid + kGlThreads * k, row = it >> 4, cc = it & 15;
      const int nv = d - 8 * cc;  // live columns of this chunk (<= 0: none, >= 8: all)
      auto mk = [nv](int e) { return (2 * e < nv ? 0x0000ffffu : 0u) | (2 * e + 1 < nv ? 0xffff0000u : 0u); };
      uint4 v = pf[k];
      v.x &= mk(0);
      v.y &= mk(1);
      v.z &= mk(2);
      v.w &= mk(3);
      *reinterpret_cast<uint4*>(&Xs[row][8 * cc]) = v;
    }
  };
  // x . beta of row erow to es[erow]: every wave, 4 lanes per row
  auto dots = [&]() {
    if (init) return;
    double dot = 0.0;
    for (int k = 0; k < nt; ++k) {
      const int col = 4 * (eq + 4 * k);
      const uint2 v = *reinterpret_cast<const uint2*>(&Xs[erow][col]);
      dot = __builtin_fma(bf16hi_to_f64(v.x << 16), bs[col], dot);
      dot = __builtin_fma(bf16hi_to_f64(v.x & 0xffff0000u), bs[col + 1], dot);
      dot = __builtin_fma(bf16hi_to_f64(v.y << 16), bs[col + 2], dot);
      dot = __builtin_fma(bf16hi_to_f64(v.y & 0xffff0000u), bs[col + 3], dot);
    }
    dot += __shfl_xor(dot, 1, 64);
    dot += __shfl_xor(dot, 2, 64);
    if (eq == 0) es[erow] = dot;
  };

  if (wave == 2) {
    // ------------------------------------------------ the row terms, the (tile, U) blocks and (U, U)
    unsigned live = 0;
    if (products) {
      for (int t = 0; t < 8; ++t)
        if (t < nt) live |= 1u << t;
      live |= 1u << 8;
    }
    f64x4 acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = (f64x4)0.0;
    double sdev = 0.0, spe = 0.0, swy = 0.0, ssw = 0.0;
    double py = 0.0, pw = 0.0, po = 0.0;
    auto fetch_row = [&](long long tile) {
      const long long r = tile * kGlTile + lane;
      const bool in = r < n;
      py = in && y != nullptr ? y[r] : 0.0;
      pw = in ? (w != nullptr ? w[r] : 1.0) : 0.0;
      po = in && off != nullptr ? off[r] : 0.0;
    };
    if (t0 < t1) {
      fetch(t0);
      fetch_row(t0);
    }
    for (long long tile = t0; tile < t1; ++tile) {
      stage();
      const double cy = py, cw = pw, co = po;
      __syncthreads();
      if (tile + 1 < t1) {
        fetch(tile + 1);
        fetch_row(tile + 1);
      }
      dots();
      __syncthreads();
      {
        const double dot = init ? 0.0 : es[lane];
        const GlrRow t = glr_row_terms((dot + b0) + co, cy, cw, co, spec, init);
        zs[lane] = t.z;
        ws[lane] = t.wt;
        sdev += t.dev;
        spe += t.pearson;
        swy += t.wy;
        ssw += t.sw;
        const long long r = tile * kGlTile + lane;
        if (mode == kGlRows && r < n) {
          rows_out[r] = t.eta;
          rows_out[n + r] = t.mu;
          rows_out[2 * n + r] = t.z;
          rows_out[3 * n + r] = t.wt;
        }
      }
      __syncthreads();
      if (live) {
#pragma unroll 2
        for (int s = 0; s < kGlTile / 4; ++s) {
          const int row = 4 * s + g;
          const double u = c == 0 ? 1.0 : (c == 1 ? zs[row] : 0.0);
          const double ub = ws[row] * u;
#pragma unroll
          for (int t = 0; t < 8; ++t)
            if (live & (1u << t))
              acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)bf16_to_f32(Xs[row][16 * t + c]), ub, acc[t], 0, 0, 0);
          acc[8] = __builtin_amdgcn_mfma_f64_16x16x4f64(u, ub, acc[8], 0, 0, 0);
        }
      }
      __syncthreads();
    }
    if (products) {
      // slot 32 + k, [row][col]: register r of a lane is row (lane >> 4) + 4 r, column lane & 15
      double* pv = pu + 2 * 16 * 256;
#pragma unroll
      for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) pv[k * 256 + (g + 4 * r) * 16 + c] = acc[k][r];
    }
    ss[lane][0] = sdev;
    ss[lane][1] = spe;
    ss[lane][2] = swy;
    ss[lane][3] = ssw;
  } else {
    // ------------------------------------------------ the X blocks with tile i <= tile j
    const int ai = wave >> 1, bj = wave & 1;
    unsigned live = 0;  // bit 4 i + j of the 4 x 4 arrangement
    if (products) {
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
          const int ti = 4 * ai + i, tj = 4 * bj + j;
          if (ti < nt && tj < nt && ti <= tj) live |= 1u << (4 * i + j);
        }
    }
    f64x4 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = (f64x4)0.0;
    if (t0 < t1) fetch(t0);
    for (long long tile = t0; tile < t1; ++tile) {
      stage();
      __syncthreads();
      if (tile + 1 < t1) fetch(tile + 1);
      dots();
      __syncthreads();
      __syncthreads();  // wave 2 makes the row terms between these two
      if (live) {
#pragma unroll 2
        for (int s = 0; s < kGlTile / 4; ++s) {
          const int row = 4 * s + g;
          const double wv = ws[row];
          double a[4], b[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            a[i] = (double)bf16_to_f32(Xs[row][16 * (4 * ai + i) + c]);
            b[i] = wv * (double)bf16_to_f32(Xs[row][16 * (4 * bj + i) + c]);
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
    if (products) {
      double* pv = pu + (long long)wave * 16 * 256;
#pragma unroll
      for (int k = 0; k < 16; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) pv[k * 256 + (g + 4 * r) * 16 + c] = acc[k][r];
    }
  }
  if (mode == kGlRows) return;
  __syncthreads();
  if (tid < 4) {
    double s = 0.0;
    for (int r = 0; r < kGlTile; ++r) s += ss[r][tid];
    pu[kGlSlots * 256 + tid] = s;
  }
}

// out[e] for e < m m: G[i][j], the entry (min, max) of the upper triangle summed over the slabs in slab order (with
// `gram`; left as it is otherwise); out[m m + k]: stat k summed the same way.
__global__ __launch_bounds__(256) void glr_fold_kernel(const double* __restrict__ part, int nslabs, int d, int gram,
                                                       double* __restrict__ out) {
  const int m = d + 2;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)m * m + 4) return;
  long long off;
  if (e >= (long long)m * m) {
    off = kGlSlots * 256 + (e - (long long)m * m);
  } else {
    if (!gram) return;
    const int i = (int)(e / m), j = (int)(e % m);
    const int a = i < j ? i : j, b = i < j ? j : i;
    int slot, row, col;
    if (b < d) {
      const int li = a >> 4, lj = b >> 4;
      slot = 16 * (2 * (li >> 2) + (lj >> 2)) + 4 * (li & 3) + (lj & 3);
      row = a & 15;
      col = b & 15;
    } else if (a < d) {
      slot = 16 * 2 + (a >> 4);
      row = a & 15;
      col = b - d;
    } else {
      slot = 16 * 2 + 8;
      row = a - d;
      col = b - d;
    }
    off = slot * 256 + row * 16 + col;
  }
  double s = 0.0;
  for (int k = 0; k < nslabs; ++k) s += part[(long long)k * kGlPart + off];
  out[e] = s;
}

}  // namespace

// Row slabs of a launch: a function of (n, d, CUs) only; two workgroups per CU, at most one slab per 64-row tile.
// 0 = unsupported width or no row.
CML_API int cml_glr_slabs(long long n, int d, int ncu) {
  if (d < 1 || d > kGlMaxD || n <= 0) return 0;
  return (int)cml_grid_cap((n + kGlTile - 1) / kGlTile, ncu, 2);
}

// Doubles of the partial buffer per slab.
CML_API long long cml_glr_part() { return kGlPart; }

// X: bf16 [n, >= d] rows of pitch ldx elements (16-byte pitch and base), wc >= d readable columns of a row (a multiple
// of 8); y, w, off: f64 [n] or null (0, 1, 0); coef: f64 [d + 1] = (beta, b0), null for the init form (any mode).
// mode 0 (step): part f64 [slabs * cml_glr_part()], out f64 [(d + 2)^2 + 4] = [G | stats]; mode 1 (stats): the same
// with G left untouched; mode 2 (rows): out f64 [4 n] = eta, mu, z, wt, part unused.
CML_API int cml_glr_pass(const void* X, long long n, long long ldx, int wc, int d, const double* y, const double* w,
                         const double* off, const double* coef, int fam, int var, int link, double p, double lp,
                         int mode, double* part, int slabs, double* out, int ncu, void* stream) {
  if (d < 1 || d > kGlMaxD || n <= 0 || X == nullptr || out == nullptr || (mode != kGlRows && part == nullptr) ||
      mode < 0 || mode > 2 || fam < 0 || fam > 4 || var < 0 || var > 1 ||
      link < 0 || link > 1 || (reinterpret_cast<size_t>(X) & 15) != 0 || (ldx & 7) != 0 || (wc & 7) != 0 || wc < d ||
      ldx < wc || slabs != cml_glr_slabs(n, d, ncu))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  GlrSpec spec;
  spec.fam = fam;
  spec.var = var;
  spec.link = link;
  spec.p = p;
  spec.lp = lp;
  hipLaunchKernelGGL(glr_pass_kernel, dim3((unsigned)slabs), dim3(kGlThreads), 0, st, (const u16*)X, n, ldx, wc, d, y, w,
                     off, coef, spec, mode, part, out);
  const int rc = cml_status();
  if (rc != 0 || mode == kGlRows) return rc;
  return cml_launch_fold(glr_fold_kernel, (long long)(d + 2) * (d + 2) + 4, st, (const double*)part, slabs, d,
                         mode == kGlStep ? 1 : 0, out);
}
