// gpsig_amd -- float64 first-order signature Gram and diagonal (include/gpsig_amd.h, "float64 evaluation"):
// the channel-major fp64 records, the route, the workspace plan and the entry points.  The kernel template is
// sig_f64.h, its instantiations sig_f64_inst.hip.  No allocation, no synchronisation; every return code is
// decided before the first launch.
#include "internal.h"
#include "sig_f64.h"

namespace gpsig {

// Records of one batch: R[sq][k][j] = x_j[k] for k < d, R[sq][d + k][j] = x_{j+1}[k] - x_j[k] (0 at the last
// point), each channel a contiguous row of l doubles (the layout idea of wide_records, unpadded: the kernel
// clamps its column index).
__global__ __launch_bounds__(256) void f64_records_kernel(const double *__restrict__ X, int n, int l, int d,
                                                          double *__restrict__ R) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)n * l) return;
  const int sq = (int)(idx / l), j = (int)(idx % l);
  const bool inc = j + 1 < l;
  const double *x = X + idx * d;
  double *r = R + (long long)sq * 2 * d * l + j;
  for (int k = 0; k < d; ++k) {
    const double xv = x[k];
    r[(long long)k * l] = xv;
    r[(long long)(d + k) * l] = inc ? x[d + k] - xv : 0.0;
  }
}

static int f64_records(const double *X, int n, int l, int d, double *R, hipStream_t s) {
  const long long tot = (long long)n * l;
  hipLaunchKernelGGL(f64_records_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, X, n, l, d, R);
  return hipGetLastError() == hipSuccess ? GPSIG_OK : GPSIG_ELAUNCH;
}

static size_t f64_record_bytes(int n, int l, int d) { return align256((size_t)n * 2 * d * l * sizeof(double)); }

// the radial profile of a Matern kind in double (kernels.py:1135-1173)
static void f64_profile_of(int base_kind, F64Args *a) {
  a->rad_a = base_kind == GPSIG_BASE_MATERN52 ? 2.23606797749978969641 : base_kind == GPSIG_BASE_MATERN32 ? 1.73205080756887729353 : 1.0;
  a->rad_c1 = base_kind == GPSIG_BASE_MATERN12 ? 0.0 : 1.0;
  a->rad_c2 = base_kind == GPSIG_BASE_MATERN52 ? 1.0 / 3.0 : 0.0;
}

// GPSIG_OK with the geometry, or the code of the first check that fails
static int f64_route(int l1, int l2, int num_levels, int difference, int pair_mode, F64Geo *g) {
  *g = F64Geo{0, 0};
  const int lmin = difference ? 2 : 1;
  if (num_levels < 1 || l1 < lmin || l2 < lmin) return GPSIG_EINVAL;
  if (pair_mode < GPSIG_PAIRS_RECT || pair_mode > GPSIG_PAIRS_DIAG) return GPSIG_EINVAL;
  if (pair_mode != GPSIG_PAIRS_RECT && l1 != l2) return GPSIG_EINVAL;
  if (num_levels > F64_MAX_LEVELS) return GPSIG_EUNSUPPORTED;
  *g = f64_geometry(difference ? l2 - 1 : l2);
  return g->W == 0 ? GPSIG_EUNSUPPORTED : GPSIG_OK;
}

}  // namespace gpsig

using namespace gpsig;

extern "C" size_t gpsig_sig_f64_workspace_bytes(int n1, int l1, int n2, int l2, int d) {
  if (n1 <= 0 || n2 <= 0 || l1 < 1 || l2 < 1 || d <= 0) return 0;
  return f64_record_bytes(n1, l1, d) + f64_record_bytes(n2, l2, d);
}

extern "C" int gpsig_sig_f64_route(int l1, int l2, int num_levels, int difference, int pair_mode, int *out) {
  if (!out) return GPSIG_EINVAL;
  F64Geo g;
  const int rc = f64_route(l1, l2, num_levels, difference, pair_mode, &g);
  out[0] = g.W;
  out[1] = g.LP;
  return rc;
}

extern "C" int gpsig_sig_gram_f64(const double *X, int n1, int l1, const double *Y, int n2, int l2, int d,
                                  int num_levels, int base_kind, int difference, int pair_mode, int row_begin,
                                  int row_end, const double *rs1, const double *rs2, const double *scale,
                                  double jitter, int out_mode, double *out, int out_row0, int out_rows,
                                  void *workspace, size_t workspace_bytes, gpsig_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!out || num_levels < 1) return GPSIG_EINVAL;
  if (check_pair_args(X, Y, n1, l1, n2, l2, d, difference ? 2 : 1, pair_mode, row_begin, row_end, false, rs1, rs2))
    return GPSIG_EINVAL;
  if (out_mode < GPSIG_OUT_LEVELS || out_mode > GPSIG_OUT_RSQRT) return GPSIG_EINVAL;
  if (out_mode == GPSIG_OUT_RSQRT && pair_mode != GPSIG_PAIRS_DIAG) return GPSIG_EINVAL;
  // the fp32 Gram's A/B flags have no float64 variant; unknown base kinds
  if (base_kind < GPSIG_BASE_RBF || base_kind > GPSIG_BASE_MATERN52) return GPSIG_EUNSUPPORTED;
  F64Geo geo;
  int rc = f64_route(l1, l2, num_levels, difference, pair_mode, &geo);
  if (rc) return rc;
  if (row_end == row_begin) return GPSIG_OK;
  const bool same = (X == Y && n1 == n2 && l1 == l2);
  Carver c;
  c.take(f64_record_bytes(n1, l1, d));
  const size_t o_fy = c.take(f64_record_bytes(n2, l2, d));
  if (!workspace || workspace_bytes < c.total()) return GPSIG_EWORKSPACE;
  PairTiles t;
  if ((rc = pair_tiles(pair_mode, row_begin, row_end, n2, 64 / geo.LP, &t))) return rc;

  double *RX = static_cast<double *>(workspace);
  double *RY = same ? RX : reinterpret_cast<double *>(static_cast<char *>(workspace) + o_fy);
  if ((rc = f64_records(X, n1, l1, d, RX, s))) return rc;
  if (!same && (rc = f64_records(Y, n2, l2, d, RY, s))) return rc;

  F64Args a{};
  a.RX = RX; a.RY = RY;
  a.n1 = n1; a.l1 = l1; a.n2 = n2; a.l2 = l2; a.d = d;
  a.kind = base_kind == GPSIG_BASE_RBF ? F64_RBF : (base_kind == GPSIG_BASE_LINEAR ? F64_LINEAR : F64_RADIAL);
  a.diff = difference ? 1 : 0;
  a.pair_mode = pair_mode;
  a.row_begin = row_begin;
  a.row_end = row_end;
  a.tiles_a0 = t.tiles_a0;
  a.ntb = t.ntb;
  a.tile_base = t.tile_base;
  a.rs1 = rs1; a.rs2 = rs2; a.scale = scale;
  a.jitter = jitter;
  a.out_mode = out_mode;
  a.out = out;
  a.out_row0 = out_row0;
  a.out_rows = out_rows;
  a.out_ld = n2;
  a.out_lvl = pair_mode == GPSIG_PAIRS_DIAG ? (long long)n1 : (long long)out_rows * n2;
  f64_profile_of(base_kind, &a);
  return dispatch<1, 2, 3, 4, 5, 6, 7, 8>(num_levels, [&](auto m) {
    return sig_f64_launch_m<decltype(m)::value>(a, geo.W, geo.LP, t.nblocks, s);
  });
}

extern "C" int gpsig_sig_diag_f64(const double *X, int n, int l, int d, int num_levels, int base_kind,
                                  int difference, double jitter, int out_mode, double *out, void *workspace,
                                  size_t workspace_bytes, gpsig_stream_t stream) {
  if (out_mode != GPSIG_OUT_LEVELS && out_mode != GPSIG_OUT_RSQRT) return GPSIG_EINVAL;
  return gpsig_sig_gram_f64(X, n, l, X, n, l, d, num_levels, base_kind, difference, GPSIG_PAIRS_DIAG, 0, n, nullptr,
                            nullptr, nullptr, jitter, out_mode, out, 0, n, workspace, workspace_bytes, stream);
}
