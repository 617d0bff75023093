// gpsig_amd -- pieces shared by the truncated-signature kernels (first order, higher order):
// the per-point feature layout, the pair-tile scheduler, the fused normalisation epilogue and the
// per-row seed (base-kernel second difference).
#pragma once
#include <type_traits>

#include "common.h"

// Rows between exact re-evaluations of the packed RBF seeds' row recurrences (RbfSeedPk::ANCHOR here, the wide
// seed in wide.h, the matrix-core Gram in sig_fo_mf.h).  64 -> 128 (profiles/r6_anchor128_ab.txt, N = 2048): H
// 22.43 -> 22.01 ms, C5 26.54 -> 26.16 ms; headline max-abs error 7.9e-7 -> 9.1e-7.
#ifndef GPSIG_PK_ANCHOR
#define GPSIG_PK_ANCHOR 128
#endif

namespace gpsig {

// Per-point feature record, FS floats (16-byte aligned): [x (DP) | dx (DP) | |dx|^2/2 | g | pad...]
// dx_i = x_{i+1} - x_i (zero for the last point), g_i = <x_i, dx_i> + |dx_i|^2/2 (2*DP+1 is odd, so
// the record always has this slot).  DP = padded channel count of the instantiation.
__host__ __device__ constexpr int feat_stride(int DP) { return ((2 * DP + 1) + 3) & ~3; }

enum Seed : int {
  SEED_RBF_DIFF = 0,    // stable/naive hybrid second difference of exp(-|x-y|^2/2)
  SEED_LIN_DIFF = 1,    // <dx_i, dy_j>
  SEED_RBF_POINT = 2,   // exp(-|x_i-y_j|^2/2)  (difference=False)
  SEED_LIN_POINT = 3,   // <x_i, y_j>           (difference=False)
  // radial profile k(r) = (1 + c1 s + c2 s^2) e^(-s), s = a r, r = |x - y| (the Matern family; a, c1, c2 at run
  // time in SigArgs): RadialSeed below, RadialSeedWide in wide.h
  SEED_RAD_DIFF = 4,    // second difference of the k grid, x-difference first (stable), then over the columns
  SEED_RAD_POINT = 5    // k(x_i, y_j)          (difference=False)
};
__host__ __device__ constexpr bool seed_is_diff(int s) { return s == SEED_RBF_DIFF || s == SEED_LIN_DIFF || s == SEED_RAD_DIFF; }
__host__ __device__ constexpr bool seed_is_radial(int s) { return s == SEED_RAD_DIFF || s == SEED_RAD_POINT; }

struct SigArgs {
  const float *FX, *FY;  // feature records (n1,l1,FS), (n2,l2,FS)
  int n1, l1, n2, l2;
  int fs;                // feature stride in floats
  int M;                 // num_levels
  int order;
  int pair_mode, row_begin, row_end;
  int tiles_a0;          // first A-tile row of this launch (UPPER/RECT)
  int ntb;               // number of B tiles (RECT) / B-tile count per full row (UPPER)
  long long tile_base;   // UPPER: prefix count of tiles before tiles_a0
  const float *rs1, *rs2, *scale;
  float jitter;
  int out_mode;
  float *out;
  int out_row0, out_rows;
  long long out_ld, out_lvl;  // row stride, level stride (elements)
  float *state;               // optional saved forward state for the VJP (gpsig_sig_gram_state)
  int mfma;                   // RBF difference seed: increment dots on the matrix cores (GPSIG_BASE_SEED_MFMA)
  int nblk;                   // column blocks per pair (first order, LP = 64; 1 = unblocked)
  // split diagnostic (GPSIG_GRAM_SPLIT): a producer launch writes each pair's cells dM to
  // dmbuf, a consumer launch streams them through the recursion; blk0 = first logical workgroup of a
  // chunked launch, dmbuf slot of a pair = its workgroup-local index
  float *dmbuf;
  long long blk0;
  // wide channel counts (DP == 0 instantiations, wide.h): channel count, padded record lengths and
  // record strides (floats) of X and Y
  int wd, lw1, lw2;
  long long sx, sy;
  // higher order past the fixed channel counts (linear base kernel, sig_ho.hip): the cells of pair
  // (a, b), row i, column j at tile + (a - tile_a0) tile_as + (b - tile_b0) (l2 - 1) + i tile_ld + j (DIAG:
  // without the b term), a GEMM of the increments; RX / RY the raw (n, l, wd) inputs (level 1 closed form)
  const float *tile;
  long long tile_as, tile_ld;
  int tile_a0, tile_b0;
  const float *RX, *RY;
  int tile_rbf;  // the tile holds RBF difference-seed cells (level 1 closed form of the RBF kernel)
  // DIAG seed tiles of the wide forward (wide.h DiagTiles): pair a at dtile + (a - dt_a0) dt_pair
  const float *dtile;
  int dt_a0;
  long long dt_pair, dt_rows, dt_ld;
  // radial seeds: k(r) = (1 + rad_c1 s + rad_c2 s^2) e^(-s), s = rad_a r (wave-uniform)
  float rad_a, rad_c1, rad_c2;
};

// Saved forward state of a first-order pair (gpsig_sig_gram_state): column sums of levels 1..M-1
// after the last row ((M-1) x (l2-1) floats, level-major), then the raw levels K_1..K_M.
__host__ __device__ inline long long state_stride(int M, int l2) { return (long long)(M - 1) * (l2 - 1) + M; }
__host__ __device__ inline long long state_slot(int a, int b, int n2, bool upper) {
  return upper ? (long long)a * n2 - (long long)a * (a - 1) / 2 + (b - a) : (long long)a * n2 + b;
}

// Wave-uniform record of row i: x_{i+1} (RBF and radial DIFF) or x_i (POINT seeds), dx_i, |dx_i|^2/2.
template <int DP>
struct RowData {
  float x[DP], dx[DP], hdx, g;
  GPSIG_DEV void load(const float *__restrict__ fx, int i, int seed) {
    constexpr int FS = feat_stride(DP);
    const float *__restrict__ fr = fx + (long long)i * FS;
    const float *__restrict__ fp = (seed == SEED_RBF_DIFF || seed == SEED_RAD_DIFF) ? fr + FS : fr;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      x[k] = fp[k];
      dx[k] = fr[DP + k];
    }
    hdx = fr[2 * DP];
    g = fr[2 * DP + 1];
  }
};

// ---------------------------------------------------------------------------------------------
// Per-row seed of the recursion: the W cells dM(i, j), j = gl*W + w, of row i of the grid the
// recursion consumes (signature_algs.py:26 for the DIFF seeds, the raw base-kernel grid otherwise).
// The lane's column data (y_j, dy_j, |dy_j|^2/2) is loaded once per pair; the row data (x_i, dx_i,
// |dx_i|^2/2, x_{i+1}) is wave-uniform and read through the scalar cache.
//
// RBF DIFF: dM = k11 - k10 - k01 + k00 with k = exp(-|x-y|^2/2).  That difference cancels
// catastrophically in fp32 for small increments, so it is evaluated as
//     dM = k00 (em1(p) em1(q) + e^p e^q em1(c)),
//     p = -<x_i - y_j, dx_i> - |dx_i|^2/2,  q = <x_i - y_j, dy_j> - |dy_j|^2/2,  c = <dx_i, dy_j>
// when |p|,|q|,|c| < EM1_TAU (em1 = minimax polynomial), and as the plain corner difference of the
// directly evaluated k grid otherwise (large increments: corners far apart, the product form would
// lose more through exponent-space rounding).  k on row i+1 is evaluated once and reused as the
// next row's k00 / k01 (right neighbour through DPP), so the grid costs one exp per cell.
template <int DP, int W, int SEED>
struct RowSeed {
  static constexpr int FS = feat_stride(DP);
  static constexpr bool DIFF = seed_is_diff(SEED);  // (the radial seeds go to RadialSeed)
  static constexpr int ANCHOR = 8;  // exact |x_i - y_j|^2 every ANCHOR rows (d^2 row recurrence between)
  float y[W][DP], dy[W][DP], hdy[W];
  bool valid_last;  // column W-1 of this lane is a real cell (others: exact zeros by construction)
  bool valid[W];    // POINT seeds
  // RBF_DIFF row state: diff = x_i - y_j, d2 = |diff|^2, kc = k(x_i, y_j), kcR = next lane's kc[0]
  float diff[W][DP], d2[W], kc[W], kcR;

  GPSIG_DEV void init(const float *__restrict__ fx, const float *__restrict__ fy, int gl, int l2) {
    const int ncols = DIFF ? l2 - 1 : l2;
    // Points beyond the sequence are clamped to its last point, whose increment record is zero, so
    // every DIFF-seed cell of a padded column evaluates to exactly 0 (both the stable and the corner
    // form); only the lane's last column can see a foreign right neighbour and is masked.
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const int j = gl * W + w;
      valid[w] = j < ncols;
      const int jj = j < l2 ? j : l2 - 1;
      const float *f = fy + (long long)jj * FS;
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        y[w][k] = f[k];
        dy[w][k] = f[DP + k];
      }
      hdy[w] = f[2 * DP];
    }
    valid_last = valid[W - 1];
    if constexpr (SEED == SEED_RBF_DIFF) {
#pragma unroll
      for (int w = 0; w < W; ++w) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          diff[w][k] = fx[k] - y[w][k];
          s = __builtin_fmaf(diff[w][k], diff[w][k], s);
        }
        d2[w] = s;
        kc[w] = __builtin_amdgcn_exp2f(s * NHL2E);
      }
      kcR = lane_next(kc[0]);
    }
  }

  // Cells of row i.  rd = wave-uniform record of row i (x_{i+1} for RBF DIFF, x_i for POINT seeds).
  // ANCH: re-evaluate |x_{i+1} - y_j|^2 exactly instead of the d2 - 2p recurrence.
  template <bool ANCH>
  GPSIG_DEV void row(const RowData<DP> &rd, float (&dM)[W]) {
    if constexpr (SEED == SEED_RBF_DIFF) {
      // 1) p, q, c from the current diff = x_i - y_j (consumed before diff is overwritten)
      float pp[W], q[W], c[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        float a = -rd.hdx, bq = -hdy[w], cc = 0.0f;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          a = __builtin_fmaf(-diff[w][k], rd.dx[k], a);
          bq = __builtin_fmaf(diff[w][k], dy[w][k], bq);
          cc = __builtin_fmaf(rd.dx[k], dy[w][k], cc);
        }
        pp[w] = a;
        q[w] = bq;
        c[w] = cc;
      }
      // 2) next row: diff = x_{i+1} - y_j, |diff|^2 = d2 - 2p (exact re-anchor every ANCHOR rows)
      float kn[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          diff[w][k] = rd.x[k] - y[w][k];
          if constexpr (ANCH) s = __builtin_fmaf(diff[w][k], diff[w][k], s);
        }
        d2[w] = ANCH ? s : __builtin_fmaf(-2.0f, pp[w], d2[w]);
        kn[w] = __builtin_amdgcn_exp2f(d2[w] * NHL2E);
      }
      const float knR = lane_next(kn[0]);
      // 3) the cells
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const float kn1 = (w + 1 < W) ? kn[w + 1] : knR;
        const float kc1 = (w + 1 < W) ? kc[w + 1] : kcR;
        const float naive = (kn1 - kn[w]) - (kc1 - kc[w]);
        const float Ep = em1_small(pp[w]), Eq = em1_small(q[w]), Ec = em1_small(c[w]);
        const float stable = kc[w] * __builtin_fmaf(Ep, Eq, (1.0f + Ep) * (1.0f + Eq) * Ec);
        const float mx = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(pp[w]), __builtin_fabsf(q[w])),
                                         __builtin_fabsf(c[w]));
        const float v = mx < EM1_TAU ? stable : naive;
        dM[w] = (w + 1 < W || valid_last) ? v : 0.0f;
      }
#pragma unroll
      for (int w = 0; w < W; ++w) kc[w] = kn[w];
      kcR = knR;
    } else if constexpr (SEED == SEED_LIN_DIFF) {
#pragma unroll
      for (int w = 0; w < W; ++w) {
        float c = 0.0f;
#pragma unroll
        for (int k = 0; k < DP; ++k) c = __builtin_fmaf(rd.dx[k], dy[w][k], c);
        dM[w] = (w + 1 < W || valid_last) ? c : 0.0f;  // padded columns have dy == 0; the halo cell of a block is masked
      }
    } else if constexpr (SEED == SEED_RBF_POINT) {
#pragma unroll
      for (int w = 0; w < W; ++w) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          const float t = rd.x[k] - y[w][k];
          s = __builtin_fmaf(t, t, s);
        }
        dM[w] = valid[w] ? __builtin_amdgcn_exp2f(s * NHL2E) : 0.0f;
      }
    } else {
#pragma unroll
      for (int w = 0; w < W; ++w) {
        float c = 0.0f;
#pragma unroll
        for (int k = 0; k < DP; ++k) c = __builtin_fmaf(rd.x[k], y[w][k], c);
        dM[w] = valid[w] ? c : 0.0f;
      }
    }
  }
};

// ---------------------------------------------------------------------------------------------
// Radial seeds (the Matern family, gpsig/kernels.py:1124-1173): k = P(s) e^(-s), P(s) = 1 + c1 s + c2 s^2,
// s = a |x - y|; (a, c1, c2) = (1, 0, 0), (sqrt 3, 1, 0), (sqrt 5, 1, 1/3) are run-time values, so one
// instantiation serves every smoothness.  Same interface as RowSeed.
//
// RAD_POINT: the k grid, one sqrt and one exp2 per cell.
//
// RAD_DIFF: dM = k11 - k10 - k01 + k00.  The plain fp32 corner difference loses up to 1.4e-5 of a level on random
// walks, so the difference over the rows is taken first, in a form without cancellation, and the column
// difference of that after it:
//     delta = s1 - s0 = a <dx_i, 2 (x_i - y_j) + dx_i> / (r1 + r0)       (the dot, not d2_1 - d2_0)
//     u(i, j) = k(x_{i+1}, y_j) - k(x_i, y_j) = e^(-s0) [ P(s1) expm1(-delta) + delta (c1 + c2 (s1 + s0)) ]
//     dM(i, j) = u(i, j + 1) - u(i, j)
// (P(s1) - P(s0) = delta (c1 + c2 (s1 + s0)) exactly.)  For c1 = 1 (the smooth profiles) the -delta of expm1 and
// the +delta c1 cancel down to O(delta s) near r = 0, so the bracket is evaluated with that part taken out by hand,
// expm1(x) = x + x^2 E2(x):
//     u = e^(-s0) delta [ P(s1) delta E2(-delta) + (c1 - 1) + c2 (s1 + s0) - s1 (c1 + c2 s1) ]
// r1 + r0 = 0 (repeated points, the diagonal of a self pair) has a zero numerator: delta = 0 and the cell is
// exactly 0, where the reference clamps r^2 at 1e-40.
// Outside the expm1 polynomial's range (|delta| >= EM1_TAU: k changes by 40 % or more over the step) u is the plain
// difference P(s1) e^(-s1) - P(s0) e^(-s0), which loses nothing there and cannot overflow.  s and e^(-s) of row
// i + 1 become row i's; each row evaluates |x_{i+1} - y_j|^2 directly, so nothing drifts.  The lane's last column
// takes u of the next lane's first column.  Columns past the sequence repeat its last point, so their u are
// equal and their cells exact zeros; the halo column of a column block is masked.

// E2(x) = (expm1(x) - x) / x^2 on |x| < EM1_TAU: Taylor to x^6, 4.3e-8 relative truncation at the ends
GPSIG_DEV float em2_small(float x) {
  float p = 2.480158730e-05f;
  p = __builtin_fmaf(p, x, 1.984126984e-04f);
  p = __builtin_fmaf(p, x, 1.388888889e-03f);
  p = __builtin_fmaf(p, x, 8.333333333e-03f);
  p = __builtin_fmaf(p, x, 4.166666667e-02f);
  p = __builtin_fmaf(p, x, 1.666666667e-01f);
  return __builtin_fmaf(p, x, 0.5f);
}
// u = k(s1) - k(s0) of a radial profile (a, c1, c2 folded into the arguments): s0, e0 = e^(-s0), s1, e1 = e^(-s1),
// num = <dx, 2 (x_{i+1} - y) - dx> = r1^2 - r0^2, a2 = a^2, c1m1 = c1 - 1
GPSIG_DEV float radial_step(float s0, float e0, float s1, float e1, float num, float a2, float c1, float c1m1,
                            float c2) {
  const float den = s1 + s0;
  const float delta = den > 0.0f ? a2 * num * __builtin_amdgcn_rcpf(den) : 0.0f;
  const float q1 = __builtin_fmaf(c2, s1, c1), q0 = __builtin_fmaf(c2, s0, c1);
  const float P1 = __builtin_fmaf(s1, q1, 1.0f), P0 = __builtin_fmaf(s0, q0, 1.0f);
  const float g = __builtin_fmaf(-s1, q1, __builtin_fmaf(c2, den, c1m1));
  const float stable = e0 * delta * __builtin_fmaf(P1 * delta, em2_small(-delta), g);
  const float plain = __builtin_fmaf(P1, e1, -P0 * e0);
  return __builtin_fabsf(delta) < EM1_TAU ? stable : plain;
}

// k of a radial profile at squared distance d2, fp64 (the closed form of level 1)
GPSIG_DEV double radial_profile64(double d2, float a, float c1, float c2) {
  const double s = (double)a * sqrt(d2);
  return (1.0 + s * ((double)c1 + (double)c2 * s)) * exp(-s);
}

template <int DP, int W, int SEED>
struct RadialSeed {
  static_assert(seed_is_radial(SEED), "radial seeds");
  static constexpr int FS = feat_stride(DP);
  static constexpr bool DIFF = SEED == SEED_RAD_DIFF;
  static constexpr int ANCHOR = 1 << 30;  // no row recurrence
  float y[W][DP];
  bool valid_last;  // DIFF: column W-1 of this lane is a real cell
  bool valid[W];    // POINT
  float ra, rc1, rc2;
  float s0[W], e0[W];  // DIFF row state: s = a |x_i - y_j|, e^(-s)

  GPSIG_DEV void set_profile(float a, float c1, float c2) {
    ra = a;
    rc1 = c1;
    rc2 = c2;
  }
  // s = a |x - y_w|
  GPSIG_DEV float dist(const float (&x)[DP], int w) const {
    float d2 = 0.0f;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const float t = x[k] - y[w][k];
      d2 = __builtin_fmaf(t, t, d2);
    }
    return ra * __builtin_amdgcn_sqrtf(d2);
  }
  GPSIG_DEV float profile(float s) const { return __builtin_fmaf(s, __builtin_fmaf(rc2, s, rc1), 1.0f); }

  // set_profile first
  GPSIG_DEV void init(const float *__restrict__ fx, const float *__restrict__ fy, int gl, int l2) {
    const int ncols = DIFF ? l2 - 1 : l2;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const int j = gl * W + w;
      valid[w] = j < ncols;
      const int jj = j < l2 ? j : l2 - 1;
      const float *f = fy + (long long)jj * FS;
#pragma unroll
      for (int k = 0; k < DP; ++k) y[w][k] = f[k];
    }
    valid_last = valid[W - 1];
    if constexpr (DIFF) {
      float x0[DP];
#pragma unroll
      for (int k = 0; k < DP; ++k) x0[k] = fx[k];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        s0[w] = dist(x0, w);
        e0[w] = __builtin_amdgcn_exp2f(-s0[w] * L2E);
      }
    }
  }

  // Cells of row i.  rd = record of row i (x_{i+1} for DIFF, x_i for POINT).
  template <bool ANCH>
  GPSIG_DEV void row(const RowData<DP> &rd, float (&dM)[W]) {
    if constexpr (DIFF) {
      float u[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        float d2 = 0.0f, num = 0.0f;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          const float t = rd.x[k] - y[w][k];  // x_{i+1} - y_j
          d2 = __builtin_fmaf(t, t, d2);
          num = __builtin_fmaf(rd.dx[k], __builtin_fmaf(2.0f, t, -rd.dx[k]), num);
        }
        const float s1 = ra * __builtin_amdgcn_sqrtf(d2);
        const float e1 = __builtin_amdgcn_exp2f(-s1 * L2E);
        u[w] = radial_step(s0[w], e0[w], s1, e1, num, ra * ra, rc1, rc1 - 1.0f, rc2);
        s0[w] = s1;
        e0[w] = e1;
      }
      const float uR = lane_next(u[0]);
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const float u1 = (w + 1 < W) ? u[w + 1] : uR;
        dM[w] = (w + 1 < W || valid_last) ? u1 - u[w] : 0.0f;
      }
    } else {
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const float s = dist(rd.x, w);
        dM[w] = valid[w] ? profile(s) * __builtin_amdgcn_exp2f(-s * L2E) : 0.0f;
      }
    }
  }
};
// the generic per-row seed of a seed kind
template <int DP, int W, int SEED>
using GenSeed = std::conditional_t<seed_is_radial(SEED), RadialSeed<DP, W, SEED>, RowSeed<DP, W, SEED>>;

// ---------------------------------------------------------------------------------------------
// RBF DIFF seed on column pairs (first-order kernel; W even).  Same cells as RowSeed<.., RBF_DIFF>,
// with the per-row work cut to what the recursion needs and laid out for v_pk_* instructions.
// With p_ij = <y_j, dx_i> - g_i (g_i from the feature record), c_ij = <dx_i, dy_j> and
// q_ij = <x_i - y_j, dy_j> - |dy_j|^2/2, the cell is k(x_i,y_j) (Ep Eq + (1 + Ep)(1 + Eq) Ec),
// E* = expm1(*).  The cell is evaluated in increment form (cells()): with the row increment
// d_ij = k(x_{i+1}, y_j) - k(x_i, y_j) = k Ep and w_ij = Ec (1 + Eq) its two terms are d Eq + (k + d) w, and
// both row-to-row quantities are sums of what the cell already computed:
//   k(x_{i+1}, y_j) = k(x_i, y_j) + d_ij               q_{i+1,j} = q_ij + c_ij
//   Eq_{i+1,j} = Eq_ij + w_ij                          (= expm1(q_ij + c_ij), no cancellation)
// d itself chains along the columns (d_{i,j+1} = d_ij + dM_ij: dM is the second difference of the k grid),
// so a row costs one packed dot and one polynomial expm1 (c) per column pair, the dot and expm1 of p for
// the lane's first pair, and six packed operations per pair: no
// exp.  k and Eq are re-evaluated exactly from x_{i+1} - y_j on anchor rows (every ANCHOR rows), so
// rounding drift is bounded by ANCHOR steps.  When |p| or |c| of some cell of the wave reaches
// EM1_TAU (a wave-uniform branch), the next row is evaluated exactly and those cells take the plain
// corner difference of the k grid.
template <int DP, int W>
struct RbfSeedPk {
  static_assert(W % 2 == 0, "column pairs");
  static constexpr int W2 = W / 2;
  static constexpr int FS = feat_stride(DP);
  static constexpr int ANCHOR = GPSIG_PK_ANCHOR;
  // Wide channels (DP >= YG_DP): only column pair 0's points stay in registers (the rows' p dots
  // need them, the other pairs' p follow by the column recurrence); the others are needed only on
  // anchor and slow rows (exact) and are re-read from the records there.  This keeps W = 8 columns per
  // lane within 256 VGPRs at D = 6..8.
  static constexpr int YG_DP = 6;
  // (W = 10, the 10-lane groups: also at any DP, to stay within 256 VGPRs)
  static constexpr bool YG = DP >= YG_DP || W > 8;
  static constexpr int YR = YG ? 1 : W2;
  f2 y[YR][DP], dy[W2][DP], hdy[W2];
  f2 Eq[W2], kc[W2];  // expm1(q_ij), k(x_i, y_j)
  // u_ij = k(x_i, y_j) - k(x_0, y_j), the running sum of the rows' increments d, and du = d of the row just
  // evaluated (exact rows: the difference of the exact k rows).  The exclusive 2-D prefix of the cells
  // telescopes to S_1(i, j) = u_ij - u_i0 (sig_fo.h, levels); u is advanced by step_u() once row i's levels
  // have read it.  Dead where the kernel scans level 1 instead.
  f2 u[W2], du[W2];
  bool valid_last;
  bool clo = false;   // every |c_ij| of the wave < EM1_LO_TAU: Ec by the cubic (bound_c)
  const float *fyb;   // YG: the block's point records, this lane's first column, the last point
  int jl0, jlast;

  // point y_j of column pair w2 (both halves), channel k
  GPSIG_DEV f2 yv(int w2, int k) const {
    if (!YG || w2 < YR) return y[w2 < YR ? w2 : 0][k];
    f2 v;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = jl0 + w2 + h * W2;
      v[h] = fyb[(long long)(j < jlast ? j : jlast) * FS + k];
    }
    return v;
  }
  GPSIG_DEV void init(const float *__restrict__ fx, const float *__restrict__ fy, int gl, int l2) {
    const int ncols = l2 - 1;
    fyb = fy;
    jl0 = gl * W;
    jlast = l2 - 1;
    // columns past the sequence clamp to its last point (zero increment): their cells are exact
    // zeros in the product form; only the lane's last column can see a foreign right neighbour.
    // l2 = points of this column block (its last one the halo point when the block is not the last)
#pragma unroll
    for (int w2 = 0; w2 < W2; ++w2)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = gl * W + w2 + h * W2;  // pair w2 = columns (w2, w2 + W/2) of the lane
        const int jj = j < l2 ? j : l2 - 1;
        const float *f = fy + (long long)jj * FS;
        // a column with no cell (past the sequence, or the right halo point of a column block) gets a
        // zero increment, so its product-form cell is exactly 0
        const bool cell = j < ncols;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          if (w2 < YR) y[w2 < YR ? w2 : 0][k][h] = f[k];
          dy[w2][k][h] = cell ? f[DP + k] : 0.0f;
        }
        hdy[w2][h] = cell ? f[2 * DP] : 0.0f;
        if (w2 == W2 - 1 && h == 1) valid_last = j < ncols;
      }
    float x0[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) x0[k] = fx[k];
    exact(x0, Eq, kc);
#pragma unroll
    for (int w2 = 0; w2 < W2; ++w2) u[w2] = du[w2] = splat2(0.0f);
  }

  // |c_ij| = |<dx_i, dy_j>| <= 2 sqrt(hdx_i hdy_j) (Cauchy-Schwarz on the records' |d|^2/2): when the
  // bound over all rows of x and all columns of the wave stays below EM1_LO_TAU (with margin for the
  // records' rounding), every Ec of the pair block takes the cubic (wave-uniform, once per block).
  GPSIG_DEV void bound_c(const float *__restrict__ fx, int nrows) {
    float hx = 0.0f, hy = 0.0f;
    for (int i = (int)__lane_id(); i < nrows; i += 64) hx = __builtin_fmaxf(hx, fx[(long long)i * FS + 2 * DP]);
#pragma unroll
    for (int w2 = 0; w2 < W2; ++w2) hy = __builtin_fmaxf(hy, __builtin_fmaxf(hdy[w2][0], hdy[w2][1]));
    hx = wave_max(hx);
    hy = wave_max(hy);
    clo = wave_uniform(4.0f * hx * hy < 0.98f * EM1_LO_TAU * EM1_LO_TAU ? 1 : 0) != 0;
  }

  // expm1(q) and k(x, y) of the row with point x, evaluated from x - y
  GPSIG_DEV void exact(const float (&x)[DP], f2 (&Eqo)[W2], f2 (&ko)[W2]) const {
#pragma unroll
    for (int w2 = 0; w2 < W2; ++w2) {
      f2 s = splat2(0.0f), qq = -hdy[w2];
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        const f2 df = splat2(x[k]) - yv(w2, k);
        s = fma2(df, df, s);
        qq = fma2(df, dy[w2][k], qq);
      }
      s = s * splat2(NHL2E);
      Eqo[w2] = em1_small2(qq);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        ko[w2][h] = __builtin_amdgcn_exp2f(s[h]);
        // outside the polynomial range expm1(q) = e^q - 1 loses nothing that matters
        if (!(__builtin_fabsf(qq[h]) < EM1_TAU)) Eqo[w2][h] = __builtin_amdgcn_exp2f(qq[h] * L2E) - 1.0f;
      }
    }
  }

  // Wave-uniform part of row i's record the recurrences need (x_{i+1} is read only on anchor rows
  // and slow rows, straight from the record).
  struct Row {
    float dx[DP], g;
    // record of row i; x_{i+1} = fr[FS .. FS + DP).  Constant address space: the records are read through
    // the scalar cache in every instantiation (the 10-lane groups took them through the vector path)
    cfloat *fr;
    GPSIG_DEV void load(const float *__restrict__ fx, int i) {
      fr = as_const(fx) + (long long)i * FS;
#pragma unroll
      for (int k = 0; k < DP; ++k) dx[k] = fr[DP + k];
      g = fr[2 * DP + 1];
    }
    // member by member (a whole-struct copy in the row loop kept the record in memory: same symptom as at
    // p0_dot)
    GPSIG_DEV void set(const Row &o) {
      fr = o.fr;
#pragma unroll
      for (int k = 0; k < DP; ++k) dx[k] = o.dx[k];
      g = o.g;
    }
  };

  GPSIG_DEV void next_exact(const Row &rd, f2 (&Eqo)[W2], f2 (&ko)[W2]) const {
    float x1[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) x1[k] = rd.fr[FS + k];
    exact(x1, Eqo, ko);
  }

  // p of column pair 0 for the row with record rd.  It reads no row state, so the hot loop takes it a row
  // ahead (sig_fo.h), where its serial chain of packed FMAs has the level recursion to hide behind.
  // It reads through the record's pointer (the same loads as Row::load's, merged with them).  Splats of
  // members of a Row that is carried round a loop were turned (hipcc of ROCm 7.2) into two-float loads of the
  // struct, which then is not promoted to registers.  Symptom in the row loop's assembly: ds_write / ds_read
  // of the record and global_load instead of s_load for it.
  GPSIG_DEV f2 p0_dot(const Row &rd) const {
    f2 a = splat2(-rd.fr[2 * DP + 1]);
#pragma unroll
    for (int k = 0; k < DP; ++k) a = fma2(y[0][k], splat2(rd.fr[DP + k]), a);
    return a;
  }

  // The dots of row i shared by row() and hot_dots(): c (every pair) and p, from pair 0's p0 by the column
  // recurrence described at row().  Returns the lane's range-check value max |p|, |c|.
  template <bool CLO>
  GPSIG_DEV float dots(const Row &rd, f2 p0, f2 (&p)[W2], f2 (&c)[W2]) const {
    // channel-major, so the pairs' dots (each a serial chain of packed FMAs) are written interleaved: a
    // packed result read by the very next instruction costs a wait state
#pragma unroll
    for (int w2 = 0; w2 < W2; ++w2) c[w2] = dy[w2][0] * splat2(rd.dx[0]);
#pragma unroll
    for (int k = 1; k < DP; ++k)
#pragma unroll
      for (int w2 = 0; w2 < W2; ++w2) c[w2] = fma2(dy[w2][k], splat2(rd.dx[k]), c[w2]);
    p[0] = p0;
#pragma unroll
    for (int w2 = 1; w2 < W2; ++w2) p[w2] = p[w2 - 1] + c[w2 - 1];
    float mx = 0.0f;
#pragma unroll
    for (int w2 = 0; w2 < W2; ++w2)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // CLO: every Ec is in the cubic's range a priori, and the pairs after the first never form Ep (their
        // increment d follows the exact chain, cells()), so only the first pair's p meets a polynomial
        if constexpr (CLO) {
          if (w2 == 0) mx = __builtin_fmaxf(mx, __builtin_fabsf(p[w2][h]));
        } else {
          mx = __builtin_fmaxf(__builtin_fmaxf(mx, __builtin_fabsf(p[w2][h])), __builtin_fabsf(c[w2][h]));
        }
      }
    return mx;
  }

  // The cells of row i in increment form, from its dots c and pair 0's p0 and the current kc, Eq.  With
  // d_ij = k(x_{i+1}, y_j) - k(x_i, y_j) = kc Ep and w = Ec (1 + Eq) the cell's two terms read
  //   dM = kc Ep Eq + kc (1 + Ep) (1 + Eq) Ec = d Eq + kn w,   kn = kc + d,   Eqn = Eq + w
  // (kn, Eqn: the next row's kc, Eq), and d chains along the columns exactly: dM is the second difference
  // of the k grid, so d_{i,j+1} = d_ij + dM_ij.  Only pair 0 forms Ep (d = kc Ep); pairs 1 .. W/2-1 follow
  // in-lane, six packed operations per pair.  d is left in du for the level-1 prefix (u).
  // kn / Eqn may be kc / Eq themselves (the hot row advances them in place).
  template <bool CLO>
  GPSIG_DEV void cells(f2 p0, const f2 (&c)[W2], f2 (&dM)[W2], f2 (&kn)[W2], f2 (&Eqn)[W2]) {
    f2 Ec[W2];
    if constexpr (CLO)
      em1_lo2_n<W2>(c, Ec);
    else
      em1_small2_n<W2>(c, Ec);
    const f2 Pp = em1_small2_poly(p0);
    {
      // every product below is rounded: the sums that take d = kc Ep (kc + d, u + d, d + dM) would otherwise
      // be fused with it or not by where the branches of the row loop fall
#pragma clang fp contract(off)
      f2 d = kc[0] * (Pp * p0);
#pragma unroll
      for (int w2 = 0; w2 < W2; ++w2) {
        const f2 k1 = kc[w2] + d;
        const f2 w = fma2(Ec[w2], Eq[w2], Ec[w2]);  // Ec (1 + Eq)
        const f2 m = fma2(d, Eq[w2], k1 * w);
        du[w2] = d;
        dM[w2] = m;
        kn[w2] = k1;
        Eqn[w2] = Eq[w2] + w;
        if (w2 + 1 < W2) d = d + m;
      }
    }
  }

  // u += du: the level-1 prefix state after row i's levels have read it (sig_fo.h)
  GPSIG_DEV void step_u() {
#pragma unroll
    for (int w2 = 0; w2 < W2; ++w2) {
#pragma clang fp contract(off)
      u[w2] = u[w2] + du[w2];
    }
  }

  // Row i of the hot loop (sig_fo.h), p0 = p0_dot(rd), in two calls with the caller's one branch between them.
  // hot_dots: the dots c and the range check; true when a cell of the wave is outside the polynomial range.
  // The caller then leaves the run with no state written and runs row() on the same record (the slow path),
  // which recomputes the same dots.  hot_cells: the cells into dM, with kc and Eq advanced in place by the
  // row-to-row recurrences (the increment form needs the next row's k for the cell itself, so the cells
  // cannot precede the check as long as kc is carried in place).  No exact evaluation lives here, so the
  // loop around the two carries its state in its registers.
  template <bool CLO>
  GPSIG_DEV bool hot_dots(const Row &rd, f2 p0, f2 (&c)[W2]) const {
    f2 p[W2];
    const float mx = dots<CLO>(rd, p0, p, c);
    return __builtin_amdgcn_ballot_w64(mx >= EM1_TAU) != 0;
  }
  template <bool CLO>
  GPSIG_DEV void hot_cells(f2 p0, const f2 (&c)[W2], f2 (&dM)[W2]) {
    cells<CLO>(p0, c, dM, kc, Eq);
  }

  // Cells of row i into dM.  anch (wave-uniform): the next row's state is re-evaluated exactly
  // instead of by the recurrences.
  //
  // Column recurrence of the p side: p_{i,j+1} - p_ij = <y_{j+1} - y_j, dx_i> = c_ij, so
  //   p_{i,j+1} = p_ij + c_ij
  // and only column pair 0 (the lane's columns 0 and W/2) takes the dot and the polynomial; p of pairs
  // 1 .. W/2-1 serves the range check and the slow path alone (the cells chain d, see cells()).  Rows with
  // a cell outside the polynomial range re-evaluate every Ep directly (slow path).
  // CLO: the pair block's |c| bound holds (bound_c): Ec by the cubic, and only |p| is range-checked.
  template <bool CLO = false>
  GPSIG_DEV void row(const Row &rd, bool anch, f2 (&dM)[W2]) {
    f2 p[W2], c[W2], kr[W2], Eqr[W2];
    const float mx = dots<CLO>(rd, p0_dot(rd), p, c);
    const bool slow = __builtin_amdgcn_ballot_w64(mx >= EM1_TAU) != 0;
    cells<CLO>(p[0], c, dM, kr, Eqr);
    if (anch || slow) {
      f2 Eqn[W2], kn[W2];
      next_exact(rd, Eqn, kn);
      if (slow) {
        // a cell outside the polynomial range spoils the chained d of the pairs after it: every in-range
        // cell is re-evaluated from its own p in the product form, the others take the corner difference
        const float knR = lane_next(kn[0][0]), kcR = lane_next(kc[0][0]);  // the next lane's first column
        f2 Epd[W2], Ecd[W2];
        em1_small2_n<W2>(p, Epd);
        em1_small2_n<W2>(c, Ecd);
#pragma unroll
        for (int w = 0; w < W; ++w) {
          const int w2 = w % W2, h = w / W2;
          const float kn1 = (w + 1 < W) ? kn[(w + 1) % W2][(w + 1) / W2] : knR;
          const float kc1 = (w + 1 < W) ? kc[(w + 1) % W2][(w + 1) / W2] : kcR;
          const float naive = (kn1 - kn[w2][h]) - (kc1 - kc[w2][h]);
          const float m = __builtin_fmaxf(__builtin_fabsf(p[w2][h]), __builtin_fabsf(c[w2][h]));
          float t = __builtin_fmaf(Epd[w2][h], Ecd[w2][h], Ecd[w2][h]);
          t = __builtin_fmaf(Eq[w2][h], t, t);
          const float prod = kc[w2][h] * __builtin_fmaf(Epd[w2][h], Eq[w2][h], t);
          float v = m < EM1_TAU ? prod : naive;
          if (w + 1 == W && !valid_last) v = 0.0f;
          dM[w2][h] = v;
        }
      }
#pragma unroll
      for (int w2 = 0; w2 < W2; ++w2) {
        du[w2] = kn[w2] - kc[w2];
        Eq[w2] = Eqn[w2];
        kc[w2] = kn[w2];
      }
    } else {
      // row-to-row recurrences (the cells above were the last readers of kc and Eq)
#pragma unroll
      for (int w2 = 0; w2 < W2; ++w2) {
        kc[w2] = kr[w2];
        Eq[w2] = Eqr[w2];
      }
    }
  }

  // The increment inner products of 4 consecutive rows i0 .. i0+3 on the matrix cores
  // (v_mfma_f32_4x4x1_16b_f32: 16 blocks of 4 x 4 outer products, one k per instruction).  Block b of
  // the wave is lanes 4b .. 4b+3; the A operand of lane l is row i0 + (l & 3), the B operand is the
  // lane's own column, and accumulator register r of lane l receives row i0 + r of column l:
  //   P[w][r] = <y_j, dx_{i0+r}> - g_{i0+r},   Q[w][r] = <dy_j, dx_{i0+r}>,   j = column w of the lane
  // (k-ordered fp32 fma chains, as the VALU dots).  The seed GEMM of the reference (kernels.py:946-957
  // _square_dist -> tf.matmul) restricted to what the recursion consumes.
  GPSIG_DEV void mfma_pc(const float *__restrict__ fx, int i0, f4 (&P)[W], f4 (&Q)[W]) const {
    const float *__restrict__ fa = fx + (long long)(i0 + (int)(__lane_id() & 3)) * FS;
    float ax[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) ax[k] = fa[DP + k];
    const float ng = -fa[2 * DP + 1];
    const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const int w2 = w % W2, h = w / W2;
      f4 accp = __builtin_amdgcn_mfma_f32_4x4x1f32(ng, 1.0f, zero, 0, 0, 0);
      f4 accq = __builtin_amdgcn_mfma_f32_4x4x1f32(ax[0], dy[w2][0][h], zero, 0, 0, 0);
#pragma unroll
      for (int k = 0; k < DP; ++k) accp = __builtin_amdgcn_mfma_f32_4x4x1f32(ax[k], yv(w2, k)[h], accp, 0, 0, 0);
#pragma unroll
      for (int k = 1; k < DP; ++k) accq = __builtin_amdgcn_mfma_f32_4x4x1f32(ax[k], dy[w2][k][h], accq, 0, 0, 0);
      P[w] = accp;
      Q[w] = accq;
    }
  }

  // Cells of row i from its precomputed p, c (column pairs): every pair has its own Ep, so d = kc Ep per
  // pair and the increment form of cells() without the chain.
  GPSIG_DEV void row_pc(const Row &rd, bool anch, const f2 (&p)[W2], const f2 (&c)[W2], f2 (&dM)[W2]) {
    f2 Eqn[W2], kn[W2];
    f2 Ep[W2], Ec[W2];
    em1_small2_n<W2>(p, Ep);
    em1_small2_n<W2>(c, Ec);
    float mx = 0.0f;
#pragma unroll
    for (int w2 = 0; w2 < W2; ++w2) {
#pragma clang fp contract(off)
      const f2 d = kc[w2] * Ep[w2];
      const f2 w = fma2(Ec[w2], Eq[w2], Ec[w2]);
      kn[w2] = kc[w2] + d;
      dM[w2] = fma2(d, Eq[w2], kn[w2] * w);
      Eqn[w2] = Eq[w2] + w;
      du[w2] = d;
#pragma unroll
      for (int h = 0; h < 2; ++h) mx = __builtin_fmaxf(__builtin_fmaxf(mx, __builtin_fabsf(p[w2][h])), __builtin_fabsf(c[w2][h]));
    }
    const bool slow = __builtin_amdgcn_ballot_w64(mx >= EM1_TAU) != 0;
    if (anch || slow) {
      next_exact(rd, Eqn, kn);
#pragma unroll
      for (int w2 = 0; w2 < W2; ++w2) du[w2] = kn[w2] - kc[w2];
    }
    if (slow) {
      // corner difference k11 - k10 - k01 + k00 for the cells outside the polynomial range
      const float knR = lane_next(kn[0][0]), kcR = lane_next(kc[0][0]);
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const int w2 = w % W2, h = w / W2;
        const float kn1 = (w + 1 < W) ? kn[(w + 1) % W2][(w + 1) / W2] : knR;
        const float kc1 = (w + 1 < W) ? kc[(w + 1) % W2][(w + 1) / W2] : kcR;
        const float naive = (kn1 - kn[w2][h]) - (kc1 - kc[w2][h]);
        const float m = __builtin_fmaxf(__builtin_fabsf(p[w2][h]), __builtin_fabsf(c[w2][h]));
        float v = m < EM1_TAU ? dM[w2][h] : naive;
        if (w + 1 == W && !valid_last) v = 0.0f;
        dM[w2][h] = v;
      }
    }
#pragma unroll
    for (int w2 = 0; w2 < W2; ++w2) {
      Eq[w2] = Eqn[w2];
      kc[w2] = kn[w2];
    }
  }
};

// ---------------------------------------------------------------------------------------------
// Level 1 of a DIFF seed in closed form.  K_1 = sum_ij dM_ij telescopes to the corner difference
// k(x_L, y_L) - k(x_L, y_0) - k(x_0, y_L) + k(x_0, y_0) (linear: <x_L - x_0, y_L - y_0>), evaluated
// once per pair in fp64.  The fp32 row sums of dM cancel down to K_1 and lose ~1e-7 of sum|dM|,
// which is the whole error budget when K_1 is small against the cells (K_1 feeds only level 1).
template <int DP, int SEED>
GPSIG_DEV float level1_closed(const float *__restrict__ fx, const float *__restrict__ fy, int l1, int l2,
                               float ra = 0.0f, float rc1 = 0.0f, float rc2 = 0.0f) {
  constexpr int FS = feat_stride(DP);
  const float *x0 = fx, *xl = fx + (long long)(l1 - 1) * FS;
  const float *y0 = fy, *yl = fy + (long long)(l2 - 1) * FS;
  if constexpr (SEED == SEED_RAD_DIFF) {  // the radial profile (ra, rc1, rc2) at the four corners
    auto k = [&](const float *a, const float *b) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < DP; ++c) {
        const double d = (double)a[c] - (double)b[c];
        s = __builtin_fma(d, d, s);
      }
      return radial_profile64(s, ra, rc1, rc2);
    };
    return (float)((k(xl, yl) - k(xl, y0)) - (k(x0, yl) - k(x0, y0)));
  } else if constexpr (SEED == SEED_RBF_DIFF) {
    auto k = [](const float *a, const float *b) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < DP; ++c) {
        const double d = (double)a[c] - (double)b[c];
        s = __builtin_fma(d, d, s);
      }
      return exp(-0.5 * s);
    };
    return (float)((k(xl, yl) - k(xl, y0)) - (k(x0, yl) - k(x0, y0)));
  } else {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < DP; ++c) s = __builtin_fma((double)xl[c] - (double)x0[c], (double)yl[c] - (double)y0[c], s);
    return (float)s;
  }
}

// ---------------------------------------------------------------------------------------------
// Tile scheduler.  A workgroup = 4 waves; wave w takes sequence a = 4*ta + w; the wave's G = 64/LP
// lane groups take b = G*tb + g.  UPPER enumerates only tiles with some b >= a: with k = 4/G,
// tile row ta has ntb - k*ta tiles, prefix P(r) = r*ntb - k*r*(r-1)/2, inverted in closed form.
struct Tile { int ta, tb; };

// sum_{i < n} floor((a i + b) / m), n, m > 0, a, b >= 0 (Euclid-like reduction, O(log m) steps)
__host__ __device__ inline long long floor_sum(long long n, long long m, long long a, long long b) {
  long long ans = 0;
  while (true) {
    if (a >= m) {
      ans += (n - 1) * n / 2 * (a / m);
      a %= m;
    }
    if (b >= m) {
      ans += n * (b / m);
      b %= m;
    }
    const long long y = a * n + b;
    if (y < m) break;
    n = y / m;
    b = y % m;
    const long long t = m;
    m = a;
    a = t;
  }
  return ans;
}
// Tiles of the upper triangle when a tile row (4 sequences a) is not a whole number of B tiles (G = 6
// sequences b per wave, LP = 10): tile row r begins at B tile floor(4 r / G) (the first holding some
// b >= 4 r), so P(r) = r ntb - sum_{t < r} floor(4 t / G).
__host__ __device__ inline long long upper_prefix_g(long long r, long long ntb, int G) {
  return r * ntb - floor_sum(r, G, 4, 0);
}
// The same prefix with G a compile-time constant (the kernel's tile decoder: no runtime division).
// With p / q = 4 / G in lowest terms and r = q Q + R, floor(p (q u + v) / q) = p u + floor(p v / q), so
// sum_{t<r} floor(4t/G) = p q Q (Q-1)/2 + Q S + p Q R + sum_{v<R} floor(p v / q), S = sum_{v<q} floor(p v / q).
template <int G>
__host__ __device__ inline long long upper_prefix_c(long long r, long long ntb) {
  constexpr int gg = G % 4 == 0 ? 4 : (G % 2 == 0 ? 2 : 1);
  constexpr long long p = 4 / gg, q = G / gg;
  long long S = 0;
  for (long long v = 0; v < q; ++v) S += p * v / q;
  const long long Q = r / q, R = r % q;
  long long part = 0;
  for (long long v = 0; v < R; ++v) part += p * v / q;
  return r * ntb - (p * q * Q * (Q - 1) / 2 + Q * S + p * Q * R + part);
}
template <int G>
GPSIG_DEV Tile upper_tile_g(long long t, int ntb) {
  // continuous estimate: sum_{t<r} floor(4t/G) ~ (2/G) r (r - 1) - r (q - 1) / (2q), q = G / gcd(4, G)
  // (the fractional parts average (q-1)/(2q)), so the exact prefixes correct it by a step or two
  constexpr int q = G / (G % 4 == 0 ? 4 : (G % 2 == 0 ? 2 : 1));
  const double A = 2.0 / G, B = ntb + 2.0 / G + (q - 1) / (2.0 * q);
  double disc = B * B - 4.0 * A * (double)t;
  disc = disc < 0 ? 0 : disc;
  long long r = (long long)((B - __builtin_sqrt(disc)) / (2.0 * A));
  if (r < 0) r = 0;
  while (r > 0 && upper_prefix_c<G>(r, ntb) > t) --r;
  while (upper_prefix_c<G>(r + 1, ntb) <= t) ++r;
  Tile tl;
  tl.ta = (int)r;
  tl.tb = (int)(4 * r / G + (t - upper_prefix_c<G>(r, ntb)));
  return tl;
}

GPSIG_DEV Tile upper_tile(long long t, int ntb, int k) {
  // largest r with P(r) <= t
  const double A = 0.5 * k, B = ntb + 0.5 * k;
  double disc = B * B - 4.0 * A * (double)t;
  disc = disc < 0 ? 0 : disc;
  long long r = (long long)((B - __builtin_sqrt(disc)) / (2.0 * A));
  if (r < 0) r = 0;
  auto P = [&](long long rr) { return rr * (long long)ntb - (long long)k * rr * (rr - 1) / 2; };
  while (r > 0 && P(r) > t) --r;
  while (P(r + 1) <= t) ++r;
  Tile tl;
  tl.ta = (int)r;
  tl.tb = (int)(k * r + (t - P(r)));
  return tl;
}

// ---------------------------------------------------------------------------------------------
// Epilogue: levels K_1..K_M (K_0 = 1) of pair (a, b) are in lane 0 of the pair's lane group.
template <int MMAX>
GPSIG_DEV void store_pair(const SigArgs &p, int a, int b, const float (&K)[MMAX + 1]) {
  const int M = p.M;
  const bool diag_mode = p.pair_mode == GPSIG_PAIRS_DIAG;
  if (diag_mode) {
    for (int m = 0; m <= M; ++m) {
      const float v = K[m];
      p.out[(long long)m * p.out_lvl + a] = (p.out_mode == GPSIG_OUT_RSQRT) ? 1.0f / __builtin_sqrtf(v + p.jitter) : v;
    }
    return;
  }
  const bool upper = p.pair_mode == GPSIG_PAIRS_UPPER;
  const bool own = a >= p.out_row0 && a < p.out_row0 + p.out_rows;
  const bool mir = upper && a != b && b >= p.out_row0 && b < p.out_row0 + p.out_rows;
  const long long o1 = (long long)(a - p.out_row0) * p.out_ld + b;
  const long long o2 = (long long)(b - p.out_row0) * p.out_ld + a;
  if (p.out_mode == GPSIG_OUT_LEVELS) {
    for (int m = 0; m <= M; ++m) {
      if (own) p.out[m * p.out_lvl + o1] = K[m];
      if (mir) p.out[m * p.out_lvl + o2] = K[m];
    }
    return;
  }
  const float jit = (upper && a == b) ? p.jitter : 0.0f;
  float sum = 0.0f;
  for (int m = 0; m <= M; ++m) {
    float v = K[m] + jit;
    if (p.rs1) v *= p.rs1[(long long)m * p.n1 + a] * p.rs2[(long long)m * p.n2 + b];
    if (p.scale) v *= p.scale[m];
    if (p.out_mode == GPSIG_OUT_NORM_LEVELS) {
      if (own) p.out[m * p.out_lvl + o1] = v;
      if (mir) p.out[m * p.out_lvl + o2] = v;
    }
    sum += v;
  }
  if (p.out_mode == GPSIG_OUT_NORM_SUM) {
    if (own) p.out[o1] = sum;
    if (mir) p.out[o2] = sum;
  }
}

}  // namespace gpsig
