// gpsig_amd -- float64 first-order truncated signature kernel Gram on gfx950 (kernel template).
//
// The recursion of sig_fo.h evaluated in double from double inputs: dM is the second difference of the
// base-kernel grid (difference = 1) or the grid itself (difference = 0),
//     C_m(j) += dM(i, j) * excl_scan_j(C_{m-1})   (levels high to low per row i),   K_m = sum_j C_m(j).
// One lane group of LP lanes owns one pair (a, b) and streams the rows; each lane keeps W columns.  Nothing
// here is an fp32 trick: fp64 carries the cancellation of the corner differences, provided the cells are
// formed from differences of the inputs --
//   RBF / Matern:  r^2 = sum_k (x_k - y_k)^2 (never |x|^2 + |y|^2 - 2 <x, y>), k at the lane's W + 1 points,
//                  u_j = k(x_{i+1}, y_j) - k(x_i, y_j) with the previous row's k kept in registers,
//                  dM_j = u_{j+1} - u_j.  Points past the sequence repeat its last point, so their u are
//                  equal and their cells exact zeros: no halo case, no mask.
//   linear:        dM = <dx_i, dy_j> from the increments (never a corner difference of <x, y>).
// Repeated points (r = 0) give k = 1 on both rows by the same operations, so the cell is an exact zero.
//
// Channels: any count, a runtime loop over channel-major fp64 records in the workspace (x then dx, one row
// of l values per channel and sequence).  The row's x values are wave-uniform and are read through the
// constant address space (scalar cache); the column values come through the vector cache, once per pass over
// the channels, and a pass serves f64_rows(W) consecutive rows.
//
// The cross-lane scan is a Hillis-Steele scan over the wave whose terms carry a 0/1 weight (source lane in
// the same group), so every lane of every group evaluates the same expression tree and a pair's value does
// not depend on its slot in the wave (seg_incl_scan_n).
#pragma once
#include "sig_common.h"

namespace gpsig {

constexpr int F64_MAX_LEVELS = 8;
constexpr int F64_MAX_COLS = 512;  // cell columns of the one column block (LP 64 x W 8)

enum F64Kind : int { F64_RBF = 0, F64_LINEAR = 1, F64_RADIAL = 2 };

struct F64Args {
  const double *RX, *RY;  // records (n, 2 d, l): channels of x, then of dx (zero at the last point)
  int n1, l1, n2, l2, d;
  int kind, diff;
  int pair_mode, row_begin, row_end;
  int tiles_a0, ntb;
  long long tile_base;
  const double *rs1, *rs2, *scale;
  double jitter;
  int out_mode;
  double *out;
  int out_row0, out_rows;
  long long out_ld, out_lvl;
  double rad_a, rad_c1, rad_c2;  // radial profile k = (1 + c1 s + c2 s^2) e^(-s), s = a r
};

// (W, LP) of a sequence with `cols` cell columns: the smallest group that covers them at W = 4, W = 8 only
// for the last doubling (the 64-lane group).  {0, 0} past F64_MAX_COLS.
struct F64Geo { int W, LP; };
inline F64Geo f64_geometry(int cols) {
  if (cols <= 64) return {4, 16};
  if (cols <= 128) return {4, 32};
  if (cols <= 256) return {4, 64};
  if (cols <= F64_MAX_COLS) return {8, 64};
  return {0, 0};
}

using cdouble = const __attribute__((address_space(4))) double;

// Rows per channel pass of the row loop: R (W + 1) accumulators per lane beside the M W column sums
__host__ __device__ constexpr int f64_rows(int W) { return W <= 4 ? 4 : 2; }

// N inclusive prefix sums over groups of LP lanes (groups at lanes 0, LP, 2 LP, ...)
template <int LP, int N>
GPSIG_DEV void f64_incl_scan_n(double (&v)[N], int gl) {
#pragma unroll
  for (int s = 1; s < LP; s <<= 1) {
    const double f = gl >= s ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = __builtin_fma(__shfl_up(v[k], s, 64), f, v[k]);
  }
}

// Epilogue of sig_common.h's store_pair in double: levels K_0..K_M of pair (a, b)
template <int M>
GPSIG_DEV void f64_store_pair(const F64Args &p, int a, int b, const double (&K)[M + 1]) {
  if (p.pair_mode == GPSIG_PAIRS_DIAG) {
#pragma unroll
    for (int m = 0; m <= M; ++m)
      p.out[(long long)m * p.out_lvl + a] = (p.out_mode == GPSIG_OUT_RSQRT) ? 1.0 / sqrt(K[m] + p.jitter) : K[m];
    return;
  }
  const bool upper = p.pair_mode == GPSIG_PAIRS_UPPER;
  const bool own = a >= p.out_row0 && a < p.out_row0 + p.out_rows;
  const bool mir = upper && a != b && b >= p.out_row0 && b < p.out_row0 + p.out_rows;
  const long long o1 = (long long)(a - p.out_row0) * p.out_ld + b;
  const long long o2 = (long long)(b - p.out_row0) * p.out_ld + a;
  if (p.out_mode == GPSIG_OUT_LEVELS) {
#pragma unroll
    for (int m = 0; m <= M; ++m) {
      if (own) p.out[m * p.out_lvl + o1] = K[m];
      if (mir) p.out[m * p.out_lvl + o2] = K[m];
    }
    return;
  }
  const double jit = (upper && a == b) ? p.jitter : 0.0;
  double sum = 0.0;
#pragma unroll
  for (int m = 0; m <= M; ++m) {
    double v = K[m] + jit;
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

template <int W, int LP, int M>
__global__ __launch_bounds__(256) void sig_f64_kernel(F64Args p) {
  constexpr int G = 64 / LP;
  const int lane = threadIdx.x & 63;
  const int wave = wave_uniform(threadIdx.x >> 6);
  const int g = lane / LP;
  const int gl = lane % LP;
  const bool diagk = p.pair_mode == GPSIG_PAIRS_DIAG;

  // ---- which pair (the tile scheduler of sig_fo.h)
  int a, b;
  if (diagk) {
    a = p.row_begin + (int)blockIdx.x * 4 + wave;
    b = a;
    if (a >= p.row_end) return;
  } else {
    int ta, tb;
    const long long lblk = (long long)blockIdx.x;
    if (p.pair_mode == GPSIG_PAIRS_UPPER) {
      const Tile t = upper_tile(p.tile_base + lblk, p.ntb, 4 / G);
      ta = t.ta;
      tb = t.tb;
    } else {
      ta = p.tiles_a0 + (int)(lblk / p.ntb);
      tb = (int)(lblk % p.ntb);
    }
    a = ta * 4 + wave;
    b = tb * G + g;
    if (a < p.row_begin || a >= p.row_end) return;  // wave-uniform
  }
  bool pair_ok = b < p.n2;
  if (p.pair_mode == GPSIG_PAIRS_UPPER) pair_ok = pair_ok && b >= a;
  if (diagk) pair_ok = (g == 0);
  const int bl = b < p.n2 ? b : p.n2 - 1;

  const int d = p.d, l1 = p.l1, l2 = p.l2;
  const bool diff = p.diff != 0;
  const bool lin = p.kind == F64_LINEAR;
  const int nrows = diff ? l1 - 1 : l1;
  const int ncols = diff ? l2 - 1 : l2;
  cdouble *rx = (cdouble *)(p.RX + (long long)wave_uniform(a) * 2 * d * l1);
  const double *__restrict__ ry = p.RY + (long long)bl * 2 * d * l2;

  // the lane's W + 1 points (clamped to the last point) and which of its W columns hold a cell
  int jj[W + 1];
  bool valid[W];
#pragma unroll
  for (int w = 0; w <= W; ++w) {
    const int j = gl * W + w;
    jj[w] = j < l2 ? j : l2 - 1;
    if (w < W) valid[w] = j < ncols;
  }

  // One pass over the channels for R consecutive rows: every column value is loaded once per pass and used by
  // the R rows (at R = 1 the loads are one per FMA, and the loop waits for them once per channel).
  // acc[r][w] = r^2 between the row's point and the lane's point w (RBF / Matern; the difference seeds evaluate
  // x_{i+1}), or the dot <dx_i, dy_j> / <x_i, y_j> (linear).  Rows past the sequence repeat its last one; the
  // caller skips them.
  constexpr int R = f64_rows(W);
  auto chunk = [&](int i0, double (&acc)[R][W + 1]) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int w = 0; w <= W; ++w) acc[r][w] = 0.0;
    const long long ko = (lin && diff) ? d : 0;  // the increments are the records' second half
    int ir[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = i0 + r + ((!lin && diff) ? 1 : 0);
      ir[r] = i < 0 ? 0 : (i < l1 ? i : l1 - 1);
    }
    for (int c = 0; c < d; ++c) {
      cdouble *xc = rx + (ko + c) * l1;
      const double *__restrict__ yc = ry + (ko + c) * l2;
      double yv[W + 1];
#pragma unroll
      for (int w = 0; w <= W; ++w) yv[w] = yc[jj[w]];
      if (lin) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const double xv = xc[ir[r]];
#pragma unroll
          for (int w = 0; w < W; ++w) acc[r][w] = __builtin_fma(xv, yv[w], acc[r][w]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const double xv = xc[ir[r]];
#pragma unroll
          for (int w = 0; w <= W; ++w) {
            const double t = xv - yv[w];
            acc[r][w] = __builtin_fma(t, t, acc[r][w]);
          }
        }
      }
    }
  };
  // k(r^2) of the RBF / radial profile
  auto profile = [&](double r2) {
    if (p.kind == F64_RBF) return exp(-0.5 * r2);
    const double s = p.rad_a * sqrt(r2);
    return __builtin_fma(s, __builtin_fma(p.rad_c2, s, p.rad_c1), 1.0) * exp(-s);
  };

  double C[M][W];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int w = 0; w < W; ++w) C[m][w] = 0.0;
  double kp[W + 1];  // the previous row's k (difference seeds of the RBF / radial kinds)
#pragma unroll
  for (int w = 0; w <= W; ++w) kp[w] = 0.0;
  if (!lin && diff) {  // k on row 0 (chunk(-1): its first row is x_0)
    double acc[R][W + 1];
    chunk(-1, acc);
#pragma unroll
    for (int w = 0; w <= W; ++w) kp[w] = profile(acc[0][w]);
  }

  constexpr int ML = M > 1 ? M - 1 : 1;
  // the level recursion of one row: exclusive column prefix of C_{m-1} = in-lane prefix + the lanes to the left
  auto levels = [&](const double (&dM)[W]) {
    if constexpr (M > 1) {
      double E[ML][W], T[ML], base[ML];
#pragma unroll
      for (int m = 0; m < ML; ++m) {
        E[m][0] = 0.0;
#pragma unroll
        for (int w = 1; w < W; ++w) E[m][w] = E[m][w - 1] + C[m][w - 1];
        T[m] = E[m][W - 1] + C[m][W - 1];
        base[m] = T[m];
      }
      f64_incl_scan_n<LP, ML>(base, gl);
      // descending m: level m reads C_{m-1} (through E) before level m-1's update writes it
#pragma unroll
      for (int m = M - 2; m >= 0; --m) {
        const double off = base[m] - T[m];
#pragma unroll
        for (int w = 0; w < W; ++w) C[m + 1][w] = __builtin_fma(dM[w], off + E[m][w], C[m + 1][w]);
      }
    }
#pragma unroll
    for (int w = 0; w < W; ++w) C[0][w] += dM[w];
  };

  for (int i0 = 0; i0 < nrows; i0 += R) {
    double acc[R][W + 1];
    chunk(i0, acc);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (i0 + r >= nrows) break;  // wave-uniform
      double dM[W];
      if (lin) {
#pragma unroll
        for (int w = 0; w < W; ++w) dM[w] = valid[w] ? acc[r][w] : 0.0;
      } else if (diff) {
        double u[W + 1];
#pragma unroll
        for (int w = 0; w <= W; ++w) {
          const double kn = profile(acc[r][w]);
          u[w] = kn - kp[w];
          kp[w] = kn;
        }
#pragma unroll
        for (int w = 0; w < W; ++w) dM[w] = u[w + 1] - u[w];
      } else {
#pragma unroll
        for (int w = 0; w < W; ++w) dM[w] = valid[w] ? profile(acc[r][w]) : 0.0;
      }
      levels(dM);
    }
  }

  // ---- K_m = sum_j C_m(j): the group's total stands in its last lane
  double tot[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    double s = C[m][0];
#pragma unroll
    for (int w = 1; w < W; ++w) s += C[m][w];
    tot[m] = s;
  }
  f64_incl_scan_n<LP, M>(tot, gl);
  if (gl == LP - 1 && pair_ok) {
    double K[M + 1];
    K[0] = 1.0;
#pragma unroll
    for (int m = 0; m < M; ++m) K[m + 1] = tot[m];
    f64_store_pair<M>(p, a, b, K);
  }
}

template <int W, int LP, int M>
int launch_f64(const F64Args &a, long long nblocks, hipStream_t s) {
  if (nblocks <= 0) return GPSIG_OK;
  hipLaunchKernelGGL((sig_f64_kernel<W, LP, M>), dim3((unsigned)nblocks), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? GPSIG_OK : GPSIG_ELAUNCH;
}

// sig_f64_launch_m<M> (the geometry dispatch of one level count) is defined in sig_f64_inst.hip, one
// translation unit per level count; declared in internal.h.

}  // namespace gpsig
