// K35: loss and gradient of the Weibull accelerated-failure-time model over bf16 rows of padded width 16 .. 512
// (gfx950): the whole message of one L-BFGS evaluation of AFTSurvivalRegression in one read of the rows.
//
// For a row with logt = log t, censor delta in {0, 1} and coef = (beta[0 .. d), b, ls), sigma = exp(ls), all f64 after
// the exact bf16 -> f64 widening:
//   eta = x . beta + b
//   eps = (logt - eta) / sigma,  ee = exp(eps)
//   r = (delta - ee) / sigma            (d loss / d eta)
//   s = delta + (delta - ee) * eps      (d loss / d ls)
//   l = delta * ls - delta * eps + ee   (the row's negative log-likelihood)
// The fit form returns [X^T r | sum r | sum s | sum l], d + 3 doubles, and writes nothing of size n. The rows form
// writes eta and, when logt and delta are given, r, s and l per row: the values the fit form summed, bit for bit.
//
// The frame is K33's (glr.hip) with the Gram products removed and a gradient in their place; the kernel is a
// template on the padded width DP (the pitch of the rows). 256 threads own a contiguous run (slab) of 64-row tiles.
// Per tile:
//   stage    the 64 x DP bf16 rows go to LDS once, at a pitch of DP + 16 bf16; columns >= d and rows >= n are stored
//            as 0 (pad columns may hold NaN bits: masked as in K33). The global loads of tile + 1 are issued before
//            the work on tile and wait in registers: max(1, DP / 32) uint4 per thread (16 at DP = 512); logt and
//            delta of the tile's rows wait the same way on the row owners.
//   eta      lanes 4 r .. 4 r + 3 own row r: lane q adds the 4-column chunks q, q + 4, q + 8 .. in that order with
//            fma against beta in LDS as f64 (zero past d); the partial sums meet as (q0 + q1) + (q2 + q3).
//            The chunk of lane q of row r sits at dword P r + 2 q + 8 k, P = (DP + 16) / 2 = 8 (DP / 16 + 1): the 32
//            lanes of a half wave (8 rows x 4 chunks) read 8 runs of 8 dwords that start at 8 (DP / 16 + 1) r mod 64.
//            DP / 16 + 1 is odd for DP = 32, 64, 128, 256, 512 (3, 5, 9, 17, 33), so the 8 runs fall on 64 distinct
//            banks: no conflict on the ds_read_b64. For DP = 16 it is 2: rows r and r + 4 share their banks, a
//            two-way conflict on the one read a lane makes there.
//   terms    lane 4 r (q = 0), the owner of row r, calls aft_row_terms, the one function of the fit form and the rows
//            form, writes r to rs[row] and adds r, s, l to its own three registers. A row >= n has r = s = l = 0.
//   gradient plain f64 VALU fmas (each of X^T r and X beta is a matrix-vector product: 15 of the 16 result columns
//            of a v_mfma_f64_16x16x4_f64 would be zeros). Thread tid owns the column pair cp = tid % (DP / 2) and the
//            row group rg = tid / (DP / 2) of G = 512 / DP groups; G <= 32 divides the 64 rows for every width (two
//            rows per group at DP = 16), so G needs no cap. It reads the dword Xs[row][2 cp] of the rows rg, rg + G,
//            rg + 2 G .. in that order (consecutive lanes read consecutive dwords; for DP >= 128 a wave reads one
//            row, conflict-free; for DP = 64, 32, 16 a wave spans 2, 4, 8 rows whose runs overlap on 8, 8 and all
//            banks: at most two-way) and rs[row] as a broadcast, and keeps two f64 accumulators for the whole run.
// Three barriers per tile (two in the rows form). At the end of its run a workgroup adds the G row groups of a
// column in group order through LDS, the three scalars over the 64 row owners in row order, and writes its partial
// of d + 3 doubles; aft_fold_kernel adds the slabs in slab order. No atomics, no host read; the grid is a function
// of (n, d, CUs) only; two calls give the same bits.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), __launch_bounds__(256, 2), no
// scratch in any instantiation; dynamic LDS 128 (DP + 16) + 8 DP + 6144 B (the tile, beta, rs 512 B, the gradient
// fold 4096 B, the scalar fold 1536 B):
//   DP        16     32     64    128    256    512
//   VGPRs     86     86     94    126    126    222
//   LDS B   10368  12544  16896  25600  43008  77824
// Two workgroups of DP = 512 fit the 160 KB of a CU. The grid takes four workgroups per CU for d <= 128, two above.
// aft_fold_kernel: no LDS, no scratch.
//
// Measured on an MI355X, one evaluation, best of 3 in three interleaved rounds (scripts/mb_ml.py aft), bytes read over
// time against the 6.3 TB/s a copy reaches; the reference form is loss_grad_reference, the dense form two GEMVs on an
// f64 copy of the rows with the element-wise passes between them (what f32 / f64 columns keep):
//   10M x 64  bf16: fit 0.67 ms (1.44 GB, 2.13 TB/s, 0.34 of a copy; floor 0.23 ms), reference 235 ms, dense 234 ms;
//                   rows eta only 0.32 ms (4.26 TB/s, 0.68), rows with terms 0.46 ms (3.8 TB/s, 0.60)
//   4M x 256  bf16: fit 0.69 ms (2.11 GB, 3.07 TB/s, 0.49 of a copy; floor 0.34 ms), reference 191 ms, dense 208 ms;
//                   rows eta only 0.44 ms (4.70 TB/s, 0.75), rows with terms 0.56 ms (4.0 TB/s, 0.64)
// K35 wins at both shapes, so no shape is routed to the reference form. The fit form takes twice the time of the
// eta-only rows form; why is not profiled (it adds the row terms, a third barrier per tile and the gradient's second
// pass over the staged tile).
#include "mfma64.h"

// No contraction in this file: the row terms are the same sequence of roundings wherever they are inlined (the eta
// dot product and the gradient name their fmas).
#pragma clang fp contract(off)

namespace {

constexpr int kAfThreads = 256;
constexpr int kAfTile = 64;     // rows per tile
constexpr int kAfMaxDp = 512;
constexpr int kAfFold = 512;    // doubles of the gradient fold: G row groups x DP columns, whatever DP

enum { kAfFit = 0, kAfRowsTerms = 1, kAfRowsEta = 2 };

struct AftRow {
  double r, s, l;
};

// The terms of one row. ops/aft_ops.row_terms is the same sequence of operations in torch.
__device__ __forceinline__ AftRow aft_row_terms(double eta, double logt, double delta, double ls, double sigma) {
  const double eps = (logt - eta) / sigma;
  const double ee = exp(eps);
  AftRow o;
  o.r = (delta - ee) / sigma;
  o.s = delta + (delta - ee) * eps;
  o.l = (delta * ls - delta * eps) + ee;
  return o;
}

constexpr long long aft_lds_bytes(int dp) {
  return 2LL * kAfTile * (dp + 16) + 8LL * dp + 8LL * kAfTile + 8LL * kAfFold + 8LL * 3 * kAfTile;
}

template <int DP>
__global__ __launch_bounds__(kAfThreads, 2) void aft_pass_kernel(
    const u16* __restrict__ X, long long n, long long ldx, int wc, int d, const double* __restrict__ logt,
    const double* __restrict__ delta, const double* __restrict__ coef, int mode, double* __restrict__ part,
    double* __restrict__ out) {
  constexpr int XP = DP + 16;                    // bf16 pitch of a staged row
  constexpr int CPR = DP / 8;                    // 16-byte items of a row
  constexpr int ITEMS = kAfTile * CPR;           // items of a tile
  constexpr int NI = (ITEMS + kAfThreads - 1) / kAfThreads;
  constexpr int CP = DP / 2;                     // column pairs
  constexpr int G = 2 * kAfThreads / DP;         // row groups of the gradient
  constexpr int R = kAfTile / G;                 // rows of a group
  extern __shared__ __align__(16) unsigned char aft_smem[];
  u16* Xs = reinterpret_cast<u16*>(aft_smem);
  double* bs = reinterpret_cast<double*>(aft_smem + 2 * kAfTile * XP);
  double* rs = bs + DP;
  double* gs = rs + kAfTile;
  double* ss = gs + kAfFold;
  const int tid = threadIdx.x;
  const int erow = tid >> 2, eq = tid & 3;       // the row whose eta this lane helps with, and its part of it
  const bool owner = eq == 0;
  const bool fit = mode == kAfFit, terms = mode != kAfRowsEta;
  const int nt = (d + 15) / 16;
  const int cp = tid % CP, rg = tid / CP;

  for (int c = tid; c < DP; c += kAfThreads) bs[c] = c < d ? coef[c] : 0.0;
  const double b = coef[d], ls = coef[d + 1];
  const double sigma = exp(ls);

  const long long ntiles = (n + kAfTile - 1) / kAfTile;
  long long t0, t1;
  tile_run(ntiles, t0, t1);

  // One item = 8 bf16 of one row (16 bytes). wc is a multiple of 8, so an item is inside the row or not.
  uint4 pf[NI];
  double plt = 0.0, pdl = 0.0;
  auto fetch = [&](long long tile) {
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const int it = tid + kAfThreads * k, row = it / CPR, col = 8 * (it % CPR);
      const long long r = tile * kAfTile + row;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (it < ITEMS && r < n && col < wc && col < d) v = *reinterpret_cast<const uint4*>(X + r * ldx + col);
      pf[k] = v;
    }
    if (owner && terms) {
      const long long r = tile * kAfTile + erow;
      const bool in = r < n;
      plt = in ? logt[r] : 0.0;
      pdl = in ? delta[r] : 0.0;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const int it = tid + kAfThreads * k, row = it / CPR, cc = it % CPR;
      const int nv = d - 8 * cc;  // live columns of this item (<= 0: none, >= 8: all)
      auto mk = [nv](int e) { return (2 * e < nv ? 0x0000ffffu : 0u) | (2 * e + 1 < nv ? 0xffff0000u : 0u); };
      uint4 v = pf[k];
      v.x &= mk(0);
      v.y &= mk(1);
      v.z &= mk(2);
      v.w &= mk(3);
      if (it < ITEMS) *reinterpret_cast<uint4*>(&Xs[row * XP + 8 * cc]) = v;
    }
  };

  double g0 = 0.0, g1 = 0.0;             // X^T r of columns 2 cp, 2 cp + 1 over the rows of group rg
  double sr = 0.0, sS = 0.0, sl = 0.0;   // the sums of the row this lane owns in every tile
  if (t0 < t1) fetch(t0);
  for (long long tile = t0; tile < t1; ++tile) {
    stage();
    const double clt = plt, cdl = pdl;
    __syncthreads();
    if (tile + 1 < t1) fetch(tile + 1);
    double dot = 0.0;
    for (int k = 0; k < nt; ++k) {
      const int col = 4 * (eq + 4 * k);
      const uint2 v = *reinterpret_cast<const uint2*>(&Xs[erow * XP + col]);
      dot = __builtin_fma(bf16hi_to_f64(v.x << 16), bs[col], dot);
      dot = __builtin_fma(bf16hi_to_f64(v.x & 0xffff0000u), bs[col + 1], dot);
      dot = __builtin_fma(bf16hi_to_f64(v.y << 16), bs[col + 2], dot);
      dot = __builtin_fma(bf16hi_to_f64(v.y & 0xffff0000u), bs[col + 3], dot);
    }
    dot += __shfl_xor(dot, 1, 64);
    dot += __shfl_xor(dot, 2, 64);
    if (owner) {
      const double eta = dot + b;
      const long long r = tile * kAfTile + erow;
      const bool in = r < n;
      AftRow t;
      t.r = t.s = t.l = 0.0;
      if (terms && in) t = aft_row_terms(eta, clt, cdl, ls, sigma);
      if (fit) {
        rs[erow] = t.r;
        sr += t.r;
        sS += t.s;
        sl += t.l;
      } else if (in) {
        out[r] = eta;
        if (terms) {
          out[n + r] = t.r;
          out[2 * n + r] = t.s;
          out[3 * n + r] = t.l;
        }
      }
    }
    if (fit) {
      __syncthreads();
      const unsigned* xw = reinterpret_cast<const unsigned*>(Xs);
#pragma unroll 8
      for (int j = 0; j < R; ++j) {
        const int row = G * j + rg;
        const unsigned v = xw[row * (XP / 2) + cp];
        const double rr = rs[row];
        g0 = __builtin_fma(bf16hi_to_f64(v << 16), rr, g0);
        g1 = __builtin_fma(bf16hi_to_f64(v & 0xffff0000u), rr, g1);
      }
    }
    __syncthreads();
  }
  if (!fit) return;
  gs[rg * DP + 2 * cp] = g0;
  gs[rg * DP + 2 * cp + 1] = g1;
  if (owner) {
    ss[3 * erow] = sr;
    ss[3 * erow + 1] = sS;
    ss[3 * erow + 2] = sl;
  }
  __syncthreads();
  double* pu = part + (long long)blockIdx.x * (d + 3);
  for (int c = tid; c < d; c += kAfThreads) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += gs[g * DP + c];
    pu[c] = s;
  }
  if (tid < 3) {
    double s = 0.0;
    for (int r = 0; r < kAfTile; ++r) s += ss[3 * r + tid];
    pu[d + tid] = s;
  }
}

// out[e] = the slabs' partials of entry e added in slab order, e < m = d + 3.
__global__ __launch_bounds__(256) void aft_fold_kernel(const double* __restrict__ part, int nslabs, int m,
                                                       double* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= m) return;
  double s = 0.0;
  for (int k = 0; k < nslabs; ++k) s += part[(long long)k * m + e];
  out[e] = s;
}

template <int DP>
int aft_launch(int slabs, hipStream_t st, const u16* X, long long n, long long ldx, int wc, int d, const double* logt,
               const double* delta, const double* coef, int mode, double* part, double* out) {
  return cml_launch_lds(aft_pass_kernel<DP>, slabs, kAfThreads, aft_lds_bytes(DP), st, X, n, ldx, wc, d, logt, delta,
                        coef, mode, part, out);
}

bool aft_width(long long dp) { return dp == 16 || dp == 32 || dp == 64 || dp == 128 || dp == 256 || dp == 512; }

}  // namespace

// Row slabs of a launch: a function of (n, d, CUs) only; four workgroups per CU for d <= 128, two above, at most one
// slab per 64-row tile. 0 = unsupported width or no row.
CML_API int cml_aft_slabs(long long n, int d, int ncu) {
  if (d < 1 || d > kAfMaxDp || n <= 0) return 0;
  return (int)cml_grid_cap((n + kAfTile - 1) / kAfTile, ncu, d <= 128 ? 4 : 2);
}

// Doubles of the partial buffer per slab.
CML_API long long cml_aft_part(int d) { return d + 3; }

// Bytes of dynamic LDS of a launch at the padded width dp; 0 = unsupported width.
CML_API long long cml_aft_lds(int dp) { return aft_width(dp) ? aft_lds_bytes(dp) : 0; }

// X: bf16 [n, >= d] rows of pitch ldx elements, ldx one of 16, 32, .. 512 (16-byte base), wc >= d readable columns of
// a row (a multiple of 8); coef: f64 [d + 2] = (beta, b, ls); logt, delta: f64 [n] (null in mode 2).
// mode 0 (fit): part f64 [slabs * cml_aft_part(d)], out f64 [d + 3] = [X^T r | sum r | sum s | sum l];
// mode 1 (rows with terms): out f64 [4 n] = eta, r, s, l; mode 2 (rows, eta only): out f64 [n] = eta; part unused.
CML_API int cml_aft_pass(const void* X, long long n, long long ldx, int wc, int d, const double* logt,
                         const double* delta, const double* coef, int mode, double* part, int slabs, double* out,
                         int ncu, void* stream) {
  if (d < 1 || n <= 0 || X == nullptr || out == nullptr || coef == nullptr || mode < 0 || mode > 2 ||
      (mode == kAfFit && part == nullptr) || (mode != kAfRowsEta && (logt == nullptr || delta == nullptr)) ||
      (reinterpret_cast<size_t>(X) & 15) != 0 || !aft_width(ldx) || d > ldx || (wc & 7) != 0 || wc < d || ldx < wc ||
      slabs < 1 || slabs != cml_aft_slabs(n, d, ncu))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const u16* x = (const u16*)X;
  int rc;
  switch ((int)ldx) {
    case 16: rc = aft_launch<16>(slabs, st, x, n, ldx, wc, d, logt, delta, coef, mode, part, out); break;
    case 32: rc = aft_launch<32>(slabs, st, x, n, ldx, wc, d, logt, delta, coef, mode, part, out); break;
    case 64: rc = aft_launch<64>(slabs, st, x, n, ldx, wc, d, logt, delta, coef, mode, part, out); break;
    case 128: rc = aft_launch<128>(slabs, st, x, n, ldx, wc, d, logt, delta, coef, mode, part, out); break;
    case 256: rc = aft_launch<256>(slabs, st, x, n, ldx, wc, d, logt, delta, coef, mode, part, out); break;
    default: rc = aft_launch<512>(slabs, st, x, n, ldx, wc, d, logt, delta, coef, mode, part, out); break;
  }
  if (rc != 0 || mode != kAfFit) return rc;
  return cml_launch_fold(aft_fold_kernel, (long long)d + 3, st, (const double*)part, slabs, d + 3, out);
}
