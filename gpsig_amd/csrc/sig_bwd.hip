// gpsig_amd -- extern "C" entries of the Gram VJPs (include/gpsig_amd.h: gpsig_sig_gram_vjp,
// gpsig_sig_gram_vjp_ho and their workspace queries): argument checks, the workspace plan, feature records,
// tile counts, dispatch to the per-(DP, M) instantiations of sig_bwd_kernel / sig_bwd_pk_kernel (sig_bwd.h,
// sig_bwd_pk.h, sig_bwd_inst.hip) or to the point-weight-tile VJPs (sig_bwd_wide.hip).  Cross-unit
// declarations: internal.h; alignment, carving, knobs, dispatch: host.h.
#include "internal.h"
#include "sig_bwd_pk.h"

namespace gpsig {
// channel counts past the VJP's instantiations: the wide-channel VJP (point-weight tiles + GEMMs; slower
// than the register form at few channels: d = 5 69.7 vs 31.8 ms fwd+bwd at N = 1024, L = 100).
// GPSIG_VJP_FIXED_MAX lowers the crossover for A/B runs.
static int vjp_fixed_max() {
  static const int v = clamp_int(env_int("GPSIG_VJP_FIXED_MAX", 16), 0, 16);
  return v;
}
static bool bwd_wide(int d) { return d > vjp_fixed_max(); }

// The packed column-pair VJP (sig_bwd_pk.h) for the difference seeds in one column block; GPSIG_BWD_PK=0
// keeps sig_bwd_kernel everywhere (A/B runs)
static bool bwd_pk_enabled() {
  static const bool v = env_int("GPSIG_BWD_PK", 1) != 0;
  return v;
}
// Measured (tools/kbench_vjp.hip, N = 1024, D = 5, M = 5, saved state; profiles/r6_vjp_ab.txt): at the same
// geometry the packed kernel is 1-4 % faster (L = 64: 11.12 -> 10.99 ms, L = 128: 27.28 -> 26.13 ms), but at
// 65-100 points sig_bwd_kernel's 20-lane groups (3 pairs per wave, W = 5) beat its 32-lane W = 4 (2 pairs):
// C2 21.79 vs 24.15 ms.  So the packed kernel takes every one-block shape except that segmented geometry.
static BwdGeo bwd_pk_geo(int l2, int DP, int M, int seed) {
  if (!bwd_pk_enabled() || (seed != SEED_RBF_DIFF && seed != SEED_LIN_DIFF)) return {0, 0};
  const BwdGeo old = bwd_geometry(l2, DP, M);
  if (old.LP == 20) return {0, 0};
  return bwd_pk_geometry(l2, DP, M, seed == SEED_RBF_DIFF);
}

// channel padding of the VJP instantiations (never wider than the forward's workspace padding)
static int bwd_pad(int d) {
  if (d <= 6) return d;
  if (d <= 8) return 8;
  if (d <= 16) return 16;
  return 0;
}

static int vjp_seed(int base_kind, bool difference) {
  if (base_kind == GPSIG_BASE_RBF) return difference ? SEED_RBF_DIFF : SEED_RBF_POINT;
  if (base_kind == GPSIG_BASE_LINEAR) return difference ? SEED_LIN_DIFF : SEED_LIN_POINT;
  return -1;
}

static constexpr size_t GSC_BYTES = GSCALE_SLOTS * 9 * sizeof(float);  // dscale partials (M <= 8)

// gscale[m] += sum of the GSCALE_SLOTS partial sums of level m
__global__ void gscale_reduce_kernel(const float *__restrict__ slots, int levels, float *__restrict__ gscale) {
  const int m = threadIdx.x;
  if (m >= levels) return;
  float s = 0.0f;
  for (int k = 0; k < GSCALE_SLOTS; ++k) s += slots[k * levels + m];
  gscale[m] += s;
}

// The route of one Gram VJP call and its workspace, in carve order.
//   register route (order 1 up to vjp_fixed_max() channels): the feature records of X and of Y (none when Y
//     is X), the column-block scratch of one launch chunk (sequences past one block), the dscale partials;
//   tile route (sig_bwd_wide.hip: order 1 at wide channel counts, every order > 1): the dscale partials, the
//     tile VJP's own workspace (any pair mode), the 8-wave higher-order VJP's global slabs (past 509 points).
struct VjpPlan {
  bool tile;
  int DP;  // register route: channel padding, kernel (packed or not), geometry, column blocks
  bool pk;
  BwdGeo geo;
  int nblk;
  long long scr_stride;
  size_t fx, fy, scr, gsc, wide, slab;                     // region bytes
  size_t o_fy, o_scr, o_gsc, o_wide, o_slab, total;        // offsets
};
// false: no kernel for the channel count / geometry
static bool vjp_plan(int n1, int l1, int n2, int l2, int d, int num_levels, int order, int seed, bool difference,
                     bool same, VjpPlan *p) {
  *p = VjpPlan{};
  p->tile = order > 1 || bwd_wide(d);
  p->gsc = GSC_BYTES;
  Carver c;
  if (p->tile) {
    p->wide = sig_bwd_wide_workspace(n1, l1, n2, l2, d);
    p->slab = order > 1 ? ho_bwd_slab_bytes(l2, order, num_levels) : 0;
    p->o_gsc = c.take(p->gsc);
    p->o_wide = c.take(p->wide);
    p->o_slab = c.take(p->slab);
  } else {
    p->DP = bwd_pad(d);
    if (p->DP == 0) return false;
    const BwdGeo pkgeo = bwd_pk_geo(l2, p->DP, num_levels, seed);
    p->pk = pkgeo.W != 0;
    p->geo = p->pk ? pkgeo : bwd_geometry(l2, p->DP, num_levels);
    if (p->geo.W == 0) return false;
    p->nblk = p->pk ? 1 : bwd_blocks(l2, difference, p->geo);
    p->scr_stride = bwd_scratch_floats(difference ? l1 - 1 : l1, num_levels, p->geo.W, p->nblk);
    p->fx = align256((size_t)n1 * l1 * feat_stride(p->DP) * sizeof(float));
    p->fy = same ? 0 : align256((size_t)n2 * l2 * feat_stride(p->DP) * sizeof(float));
    p->scr = (size_t)p->scr_stride * 4 * BWD_CHUNK_BLOCKS * sizeof(float);
    c.take(p->fx);
    p->o_fy = c.take(p->fy);
    p->o_scr = c.take(p->scr);
    p->o_gsc = c.take(p->gsc);
  }
  p->total = c.total();
  return true;
}

// Both routes: seed < 0 and the supported ranges are the caller's checks.
static int vjp_run(const float *X, int n1, int l1, const float *Y, int n2, int l2, int d, int num_levels, int order,
                   int seed, bool difference, int pair_mode, int row_begin, int row_end, const float *gout,
                   int gout_levels, const float *rs1, const float *rs2, const float *scale, float jitter, float *gX,
                   float *gY, float *grs1, float *grs2, float *gscale, const float *state, void *workspace,
                   size_t workspace_bytes, hipStream_t s) {
  const bool same = (X == Y && n1 == n2 && l1 == l2);
  VjpPlan pl;
  if (!vjp_plan(n1, l1, n2, l2, d, num_levels, order, seed, difference, same, &pl)) return GPSIG_EUNSUPPORTED;
  if (row_end == row_begin) return GPSIG_OK;
  if (!workspace || workspace_bytes < pl.total) return GPSIG_EWORKSPACE;
  float *gsc_slots = ws_at(workspace, pl.o_gsc);
  BwdArgs a{};
  a.n1 = n1; a.l1 = l1; a.n2 = n2; a.l2 = l2; a.d = d;
  a.M = num_levels;
  a.pair_mode = pair_mode;
  a.row_begin = row_begin;
  a.row_end = row_end;
  a.gout = gout;
  a.gout_levels = gout_levels ? 1 : 0;
  a.g_ld = n2;
  a.g_lvl = pair_mode == GPSIG_PAIRS_DIAG ? (long long)n1 : (long long)n1 * n2;
  a.rs1 = rs1; a.rs2 = rs2; a.scale = scale;
  a.jitter = jitter;
  a.gX = gX;
  a.gY = pair_mode == GPSIG_PAIRS_RECT ? gY : gX;
  a.grs1 = grs1;
  a.grs2 = pair_mode == GPSIG_PAIRS_RECT ? grs2 : grs1;
  a.state = state;
  int rc;
  if (!pl.tile) {
    float *FX = static_cast<float *>(workspace), *FY = same ? FX : ws_at(workspace, pl.o_fy);
    if ((rc = features(X, n1, l1, d, pl.DP, FX, s))) return rc;
    if (!same && (rc = features(Y, n2, l2, d, pl.DP, FY, s))) return rc;
    a.FX = FX;
    a.FY = FY;
  }
  if (gscale && pair_mode != GPSIG_PAIRS_DIAG) {
    if (hipMemsetAsync(gsc_slots, 0, GSC_BYTES, s) != hipSuccess) return GPSIG_ELAUNCH;
    a.gscale = gsc_slots;
  }
  if (pl.tile) {
    // the VJPs with point-weight tiles and emission GEMMs (sig_bwd_wide.hip)
    a.scratch = pl.slab ? ws_at(workspace, pl.o_slab) : nullptr;
    if ((rc = sig_bwd_wide(a, X, pair_mode == GPSIG_PAIRS_RECT ? Y : X, seed, ws_at(workspace, pl.o_wide), pl.wide, s,
                           order)))
      return rc;
  } else {
    a.nblk = pl.nblk;
    a.scratch = pl.scr_stride ? ws_at(workspace, pl.o_scr) : nullptr;
    a.scr_stride = pl.scr_stride;
    PairTiles t;
    if ((rc = pair_tiles(pair_mode, row_begin, row_end, n2, 64 / pl.geo.LP, &t))) return rc;
    a.tiles_a0 = t.tiles_a0;
    a.ntb = t.ntb;
    a.tile_base = t.tile_base;
    if (t.nblocks <= 0) return GPSIG_OK;
    // column-block launches go in chunks of BWD_CHUNK_BLOCKS workgroups (the scratch holds one chunk)
    const long long chunk = pl.scr_stride ? BWD_CHUNK_BLOCKS : t.nblocks;
    for (long long c = 0; c < t.nblocks; c += chunk) {
      a.blk0 = c;
      const long long nb = t.nblocks - c < chunk ? t.nblocks - c : chunk;
      rc = dispatch<1, 2, 3, 4, 5, 6, 8, 16>(pl.DP, [&](auto dp) {
        return dispatch<1, 2, 3, 4, 5, 6, 7, 8>(a.M, [&](auto m) {
          constexpr int DP = decltype(dp)::value, M = decltype(m)::value;
          return pl.pk ? sig_bwd_pk_launch_dpm<DP, M>(a, seed, pl.geo, nb, s) : sig_bwd_launch_dpm<DP, M>(a, seed, nb, s);
        });
      });
      if (rc) return rc;
    }
  }
  if (a.gscale) {
    hipLaunchKernelGGL(gscale_reduce_kernel, dim3(1), dim3(64), 0, s, gsc_slots, num_levels + 1, gscale);
    if (hipGetLastError() != hipSuccess) return GPSIG_ELAUNCH;
  }
  return GPSIG_OK;
}

// the checks gpsig_sig_gram_vjp and gpsig_sig_gram_vjp_ho share
static int vjp_check(const float *X, int n1, int l1, const float *Y, int n2, int l2, int d, int num_levels, int lmin,
                     int pair_mode, int row_begin, int row_end, const float *gout, int gout_levels, const float *rs1,
                     const float *rs2, float *gX, float *gY) {
  if (!gout || !gX || num_levels < 1) return GPSIG_EINVAL;
  if (check_pair_args(X, Y, n1, l1, n2, l2, d, lmin, pair_mode, row_begin, row_end, true, rs1, rs2)) return GPSIG_EINVAL;
  if (pair_mode == GPSIG_PAIRS_RECT && !gY) return GPSIG_EINVAL;
  if (pair_mode == GPSIG_PAIRS_DIAG && !gout_levels) return GPSIG_EINVAL;
  return GPSIG_OK;
}

}  // namespace gpsig

using namespace gpsig;

extern "C" int gpsig_sig_gram_vjp(const float *X, int n1, int l1, const float *Y, int n2, int l2, int d,
                                  int num_levels, int base_kind, int difference, int pair_mode, int row_begin, int row_end,
                                  const float *gout, int gout_levels, const float *rs1, const float *rs2,
                                  const float *scale, float jitter, float *gX, float *gY, float *grs1, float *grs2,
                                  float *gscale, const float *state, void *workspace, size_t workspace_bytes,
                                  gpsig_stream_t stream) {
  if (vjp_check(X, n1, l1, Y, n2, l2, d, num_levels, difference ? 2 : 1, pair_mode, row_begin, row_end, gout,
                gout_levels, rs1, rs2, gX, gY))
    return GPSIG_EINVAL;
  if (state && (pair_mode == GPSIG_PAIRS_DIAG || !difference)) return GPSIG_EINVAL;
  const int seed = vjp_seed(base_kind, difference != 0);
  if (seed < 0 || num_levels > 8) return GPSIG_EUNSUPPORTED;
  return vjp_run(X, n1, l1, Y, n2, l2, d, num_levels, 1, seed, difference != 0, pair_mode, row_begin, row_end, gout,
                 gout_levels, rs1, rs2, scale, jitter, gX, gY, grs1, grs2, gscale, state, workspace, workspace_bytes,
                 reinterpret_cast<hipStream_t>(stream));
}

// The query names no base kind and no X == Y: the largest of the plans those allow.
extern "C" size_t gpsig_sig_vjp_workspace_bytes(int n1, int l1, int n2, int l2, int d, int num_levels, int difference) {
  if (n1 <= 0 || n2 <= 0 || l1 < 1 || l2 < 1 || d <= 0) return 0;
  size_t best = 0;
  for (int base : {GPSIG_BASE_RBF, GPSIG_BASE_LINEAR}) {
    VjpPlan p;
    if (!vjp_plan(n1, l1, n2, l2, d, num_levels, 1, vjp_seed(base, difference != 0), difference != 0, false, &p)) continue;
    best = p.total > best ? p.total : best;
  }
  return best;
}

extern "C" int gpsig_sig_gram_vjp_ho(const float *X, int n1, int l1, const float *Y, int n2, int l2, int d,
                                     int num_levels, int order, int base_kind, int pair_mode, int row_begin,
                                     int row_end, const float *gout, int gout_levels, const float *rs1,
                                     const float *rs2, const float *scale, float jitter, float *gX, float *gY,
                                     float *grs1, float *grs2, float *gscale, void *workspace,
                                     size_t workspace_bytes, gpsig_stream_t stream) {
  if (order < 1 || vjp_check(X, n1, l1, Y, n2, l2, d, num_levels, 2, pair_mode, row_begin, row_end, gout, gout_levels,
                             rs1, rs2, gX, gY))
    return GPSIG_EINVAL;
  if (order == 1 || num_levels == 1)  // the first-order recursion
    return gpsig_sig_gram_vjp(X, n1, l1, Y, n2, l2, d, num_levels, base_kind, 1, pair_mode, row_begin, row_end, gout,
                              gout_levels, rs1, rs2, scale, jitter, gX, gY, grs1, grs2, gscale, nullptr, workspace,
                              workspace_bytes, stream);
  const int seed = vjp_seed(base_kind, true);
  if (seed < 0 || !ho_bwd_supported(l2, order, num_levels, seed)) return GPSIG_EUNSUPPORTED;
  return vjp_run(X, n1, l1, Y, n2, l2, d, num_levels, order, seed, true, pair_mode, row_begin, row_end, gout,
                 gout_levels, rs1, rs2, scale, jitter, gX, gY, grs1, grs2, gscale, nullptr, workspace, workspace_bytes,
                 reinterpret_cast<hipStream_t>(stream));
}

// gpsig_sig_vjp_ho_route: gpsig_sig_gram_vjp_ho's checks in its order, then the plan its launches follow
// (sig_ho_bwd.hip), the slab region of vjp_plan and the chunk loop of sig_bwd_wide; no launch, no device
extern "C" int gpsig_sig_vjp_ho_route(int n1, int l1, int n2, int l2, int d, int num_levels, int order, int base_kind,
                                      int pair_mode, int row_begin, int row_end, int *out) {
  if (!out || num_levels < 2 || order < 2) return GPSIG_EINVAL;
  // the query has no inputs: out stands in for the pointers the shared check wants present
  if (check_pair_args(out, out, n1, l1, n2, l2, d, 2, pair_mode, row_begin, row_end, false)) return GPSIG_EINVAL;
  for (int i = 0; i < GPSIG_SIG_VJP_HO_ROUTE_INTS; ++i) out[i] = 0;
  const int seed = vjp_seed(base_kind, true);
  HoVjpRoute r{};
  if (seed < 0 || !ho_bwd_supported(l2, order, num_levels, seed)) return GPSIG_EUNSUPPORTED;
  sig_ho_bwd_route_plan(l2, order, num_levels, &r);
  VjpPlan pl;
  if (!vjp_plan(n1, l1, n2, l2, d, num_levels, order, seed, true, pair_mode != GPSIG_PAIRS_RECT, &pl))
    return GPSIG_EUNSUPPORTED;
  r.slab_bytes = pl.slab;
  // no rows: vjp_run returns before the chunk loop, so the geometry alone
  const int rc = row_end == row_begin ? GPSIG_OK : sig_bwd_wide_ho_route(n1, l1, n2, l2, d, num_levels, order, seed,
                                                                         pair_mode, row_begin, row_end, &r);
  out[0] = r.kernel;
  out[1] = r.W;
  out[2] = r.waves;
  out[3] = r.slots;
  out[4] = r.variant;
  out[5] = (int)r.lds_bytes;
  out[6] = r.slab_bytes > 0x7fffffff ? 0x7fffffff : (int)r.slab_bytes;
  out[7] = r.chunks;
  out[8] = r.launches;
  return rc;
}

extern "C" size_t gpsig_sig_vjp_ho_workspace_bytes(int n1, int l1, int n2, int l2, int d, int num_levels, int order,
                                                   int base_kind) {
  if (n1 <= 0 || n2 <= 0 || l1 < 2 || l2 < 2 || d <= 0 || order < 1) return 0;
  if (vjp_seed(base_kind, true) < 0) return 0;  // base kinds without a VJP (the Matern family)
  if (order == 1 || num_levels == 1) return gpsig_sig_vjp_workspace_bytes(n1, l1, n2, l2, d, num_levels, 1);
  const int seed = vjp_seed(base_kind, true);
  VjpPlan p;
  if (seed < 0 || !ho_bwd_supported(l2, order, num_levels, seed)) return 0;
  return vjp_plan(n1, l1, n2, l2, d, num_levels, order, seed, true, false, &p) ? p.total : 0;
}
