// gpsig_amd -- extern "C" entry points (include/gpsig_amd.h): argument checks, workspace plans, tile counts,
// and dispatch to the templated kernels.  No allocation, no synchronisation.  The launchers of the other
// translation units are declared in internal.h; alignment, carving, knobs and the shared checks in host.h.
#include "internal.h"
#include "wide.h"

using namespace gpsig;

// Channel padding of the feature records: exact for the first-order kernels up to 6 channels,
// multiples the instantiation tables cover otherwise (sig_fo_inst / sig_ho).
static int pad_channels(int d, int order) {
  if (order == 1 && d <= 6) return d;
  if (order > 1 && d <= 4) return 4;
  if (d <= 8) return 8;
  if (d <= 16) return 16;
  if (d <= 32) return 32;
  return 0;
}

// Channel counts past the fixed instantiations (8) run the first-order forward on channel-major records
// with a runtime channel loop (wide.h), which beats the padded fixed kernels from 9 channels on
// (N = 1024, L = 128, M = 4: d = 16 12.7 vs 15.4 ms, d = 32 23.5 vs 35.6 ms; d = 8 7.7 vs 6.4 ms).
// GPSIG_FO_FIXED_MAX lowers the crossover for A/B runs (0 sends every channel count to the wide kernels).
static int fo_fixed_max() {
  static const int v = clamp_int(env_int("GPSIG_FO_FIXED_MAX", 8), 0, 8);
  return v;
}
static bool wide_channels(int d, int order) { return order == 1 && d > fo_fixed_max(); }

// The wide-channel Gram with the increment GEMM on the matrix cores (sig_fo_mf.h) for the difference seeds
// of the Gram pair modes; GPSIG_WIDE_MF=0 keeps the runtime-channel-loop kernel (A/B runs).
static bool wide_mf_enabled() {
  static const bool v = env_int("GPSIG_WIDE_MF", 1) != 0;
  return v;
}

static size_t feat_bytes(int n, int l, int d) {
  size_t wb = d > fo_fixed_max() ? align256((size_t)n * wide_rec_floats(d, l) * sizeof(float)) : 0;
  const size_t mb = d > fo_fixed_max() ? align256(mf_records_bytes(n, l, d)) : 0;
  wb = mb > wb ? mb : wb;
  const int DP = pad_channels(d, 2);  // the wider of the two paddings
  const size_t fb = DP ? align256((size_t)n * l * feat_stride(DP) * sizeof(float)) : 0;
  return wb > fb ? wb : fb;
}

static int seed_of(int base_kind, int difference) {
  if (base_kind == GPSIG_BASE_RBF) return difference ? SEED_RBF_DIFF : SEED_RBF_POINT;
  if (base_kind == GPSIG_BASE_LINEAR) return difference ? SEED_LIN_DIFF : SEED_LIN_POINT;
  if (base_kind >= GPSIG_BASE_MATERN12 && base_kind <= GPSIG_BASE_MATERN52) return difference ? SEED_RAD_DIFF : SEED_RAD_POINT;
  return -1;
}

// The radial profile k(r) = (1 + c1 s + c2 s^2) e^(-s), s = a r, of a Matern kind (kernels.py:1135-1173)
static void radial_profile_of(int base_kind, SigArgs *a) {
  a->rad_a = base_kind == GPSIG_BASE_MATERN52 ? 2.2360679774997897f : base_kind == GPSIG_BASE_MATERN32 ? 1.7320508075688772f : 1.0f;
  a->rad_c1 = base_kind == GPSIG_BASE_MATERN12 ? 0.0f : 1.0f;
  a->rad_c2 = base_kind == GPSIG_BASE_MATERN52 ? (float)(1.0 / 3.0) : 0.0f;
}

// the wide diagonal's seed tiles (wide.h DiagTiles, RBF difference seed): one chunk of pairs
static bool diag_tiled(int n, int l, int d, int order) {
  if (order != 1 || d <= fo_fixed_max() || n <= 0) return false;
  int W, LP;
  fo_wide_geo(l, SEED_RBF_DIFF, &W, &LP);
  return (long long)LP * W >= l && diag_tiles_apply(l, d, W, LP, SEED_RBF_DIFF, 1);
}
// its tiles at the wide forward's geometry, and *cp = the pairs of one chunk of n
static DiagTiles diag_tiles_plan(int n, int l, int *cp) {
  int W, LP;
  fo_wide_geo(l, SEED_RBF_DIFF, &W, &LP);
  const DiagTiles dt = diag_tiles_of(l, W, LP);
  *cp = diag_tile_pairs(dt, n);
  return dt;
}
// chunks of cp pairs over the rows [row_begin, row_end); chunk k covers [row_begin + k cp, ...)
static int diag_tile_chunks(int row_begin, int row_end, int cp) { return (row_end - row_begin + cp - 1) / cp; }

extern "C" size_t gpsig_sig_split_bytes(int l1, int l2, int d, int num_levels) {
  const int DP = pad_channels(d, 1);
  if (DP == 0 || l1 < 2 || l2 < 2 || num_levels < 1 || num_levels > 8) return 0;
  return fo_split_bytes(l1, l2, DP, num_levels);
}

// The kernel path of one sig_gram_impl call (past the increment-tile mode of sig_ho.hip) and its workspace,
// in carve order: the feature records of X and of Y (none when Y is X), the split diagnostic's cells, the
// matrix-core Gram's column-block carries (sequences past 160 points), the wide diagonal's seed tiles.
struct GramPlan {
  int DP;                                // channel padding of the fixed kernels, 0: wide
  bool wide, mf, dtiles;                 // runtime channel loop; matrix-core Gram; diagonal seed tiles
  size_t fx, fy, dm, mc, dt;             // region bytes (0: the path has no such region)
  size_t o_fy, o_dm, o_mc, o_dt, total;  // offsets (fx at 0)
};
// false: no kernel for the channel count at this order
static bool gram_plan(int n1, int l1, int n2, int l2, int d, int num_levels, int order, int seed, int pair_mode,
                      bool same, bool split, bool state, GramPlan *p) {
  *p = GramPlan{};
  p->wide = wide_channels(d, order);
  p->DP = p->wide ? 0 : pad_channels(d, order);
  if (p->DP == 0 && !p->wide) return false;
  p->mf = p->wide && wide_mf_enabled() && pair_mode != GPSIG_PAIRS_DIAG &&
          (seed == SEED_RBF_DIFF || seed == SEED_LIN_DIFF) && mf_gram_applies(d, l2);
  p->dtiles = p->wide && pair_mode == GPSIG_PAIRS_DIAG && seed == SEED_RBF_DIFF && !state && diag_tiled(n1, l1, d, order);
  const size_t fs = p->wide ? 0 : (size_t)feat_stride(p->DP) * sizeof(float);
  p->fx = p->wide ? feat_bytes(n1, l1, d) : align256((size_t)n1 * l1 * fs);
  p->fy = same ? 0 : (p->wide ? feat_bytes(n2, l2, d) : align256((size_t)n2 * l2 * fs));
  p->dm = split ? gpsig_sig_split_bytes(l1, l2, d, num_levels) : 0;
  p->mc = p->mf ? align256(mf_gram_scratch_bytes(l1, l2, d)) : 0;
  if (p->dtiles) {
    int cp;
    const DiagTiles dt = diag_tiles_plan(n1, l1, &cp);
    p->dt = align256((size_t)cp * dt.pair * sizeof(float));
  }
  Carver c;
  c.take(p->fx);
  p->o_fy = c.take(p->fy);
  p->o_dm = c.take(p->dm);
  p->o_mc = c.take(p->mc);
  p->o_dt = c.take(p->dt);
  p->total = c.total();
  return true;
}

// The query names no order, seed, pair mode, state or X == Y: region by region the largest of the plans
// those allow (the carve order is fixed, so this covers every plan sig_gram_impl can choose; the split
// diagnostic's cells come on top, gpsig_sig_split_bytes).  As before it does not ask the UPPER / DIAG modes
// for equal shapes.
extern "C" size_t gpsig_sig_workspace_bytes(int n1, int l1, int n2, int l2, int d) {
  GramPlan m{};
  for (int order : {1, 2})
    for (int pm : {GPSIG_PAIRS_RECT, GPSIG_PAIRS_UPPER, GPSIG_PAIRS_DIAG}) {
      GramPlan p;
      if (!gram_plan(n1, l1, n2, l2, d, 1, order, SEED_RBF_DIFF, pm, false, false, false, &p)) continue;
      m.fx = p.fx > m.fx ? p.fx : m.fx;
      m.fy = p.fy > m.fy ? p.fy : m.fy;
      m.mc = p.mc > m.mc ? p.mc : m.mc;
      m.dt = p.dt > m.dt ? p.dt : m.dt;
    }
  return m.fx + m.fy + m.mc + m.dt;
}

// The workspace of one gpsig_sig_gram / gpsig_sig_diag call: the feature records, or for the higher-order
// recursion past 32 channels the increments and one chunk's increment tile (sig_ho.hip tile mode).
extern "C" size_t gpsig_sig_workspace_bytes_ex(int n1, int l1, int n2, int l2, int d, int order, int pair_mode) {
  if (n1 <= 0 || n2 <= 0 || l1 < 1 || l2 < 1 || d <= 0) return 0;
  if (ho_tiled(d, order) && l1 >= 2 && l2 >= 2) return ho_tile_bytes(n1, l1, n2, l2, d, pair_mode);
  return gpsig_sig_workspace_bytes(n1, l1, n2, l2, d);
}

static int sig_gram_impl(const float *X, int n1, int l1, const float *Y, int n2, int l2, int d, int num_levels,
                         int order, int base_kind, int difference, int pair_mode, int row_begin, int row_end,
                         const float *rs1, const float *rs2, const float *scale, float jitter, int out_mode,
                         float *out, int out_row0, int out_rows, float *state, void *workspace,
                         size_t workspace_bytes, gpsig_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!out || num_levels < 1) return GPSIG_EINVAL;
  if (check_pair_args(X, Y, n1, l1, n2, l2, d, difference ? 2 : 1, pair_mode, row_begin, row_end, false, rs1, rs2))
    return GPSIG_EINVAL;
  if (out_mode < GPSIG_OUT_LEVELS || out_mode > GPSIG_OUT_RSQRT) return GPSIG_EINVAL;
  if (out_mode == GPSIG_OUT_RSQRT && pair_mode != GPSIG_PAIRS_DIAG) return GPSIG_EINVAL;
  if (order < 1) return GPSIG_EINVAL;
  const bool mfma = (base_kind & GPSIG_BASE_SEED_MFMA) != 0;
  const bool split = (base_kind & GPSIG_GRAM_SPLIT) != 0;
  base_kind &= ~(GPSIG_BASE_SEED_MFMA | GPSIG_GRAM_SPLIT);
  const int seed = seed_of(base_kind, difference);
  if (mfma && (seed != SEED_RBF_DIFF || order != 1 || state)) return GPSIG_EUNSUPPORTED;
  if (split && (mfma || seed != SEED_RBF_DIFF || order != 1 || state || pair_mode == GPSIG_PAIRS_DIAG))
    return GPSIG_EUNSUPPORTED;
  const bool tiled = ho_tiled(d, order);  // higher order past 32 channels: cells from an increment-Gram tile
  if (tiled && ((seed != SEED_LIN_DIFF && seed != SEED_RBF_DIFF) || mfma || split || state)) return GPSIG_EUNSUPPORTED;
  const bool same = (X == Y && n1 == n2 && l1 == l2);
  GramPlan pl{};
  const bool planned = !tiled && gram_plan(n1, l1, n2, l2, d, num_levels, order, seed, pair_mode, same, split,
                                           state != nullptr, &pl);
  if (seed < 0 || (!planned && !tiled)) return GPSIG_EUNSUPPORTED;
  if (pl.wide && (mfma || split)) return GPSIG_EUNSUPPORTED;
  if (state && seed_is_radial(seed)) return GPSIG_EUNSUPPORTED;  // forward only: no VJP reads a saved state
  if (row_end == row_begin) return GPSIG_OK;

  SigArgs a{};
  a.n1 = n1; a.l1 = l1; a.n2 = n2; a.l2 = l2;
  a.M = num_levels;
  a.order = order;
  a.pair_mode = pair_mode;
  a.row_begin = row_begin;
  a.row_end = row_end;
  a.rs1 = rs1; a.rs2 = rs2; a.scale = scale;
  a.jitter = jitter;
  a.out_mode = out_mode;
  a.out = out;
  a.out_row0 = out_row0;
  a.out_rows = out_rows;
  a.out_ld = n2;
  a.out_lvl = pair_mode == GPSIG_PAIRS_DIAG ? (long long)n1 : (long long)out_rows * n2;
  if (seed_is_radial(seed)) radial_profile_of(base_kind, &a);
  if (tiled) return sig_ho_tiled(a, X, Y, d, seed, workspace, workspace_bytes, s);

  const int DP = pl.DP;
  const bool wide = pl.wide, mf = pl.mf;
  if (split && pl.dm == 0) return GPSIG_EUNSUPPORTED;
  if (!workspace || workspace_bytes < pl.total) return GPSIG_EWORKSPACE;
  float *FX = static_cast<float *>(workspace);
  float *FY = same ? FX : ws_at(workspace, pl.o_fy);
  int rc = mf ? mf_records(X, n1, l1, d, FX, s) : wide ? wide_records(X, n1, l1, d, FX, s) : features(X, n1, l1, d, DP, FX, s);
  if (rc) return rc;
  if (!same && (rc = mf ? mf_records(Y, n2, l2, d, FY, s)
                        : wide ? wide_records(Y, n2, l2, d, FY, s) : features(Y, n2, l2, d, DP, FY, s)))
    return rc;

  a.FX = FX;
  a.FY = FY;
  a.fs = feat_stride(DP);
  a.state = state;
  a.mfma = mfma ? 1 : 0;
  a.dmbuf = split ? ws_at(workspace, pl.o_dm) : nullptr;
  a.wd = d;
  a.lw1 = wide_lw(l1);
  a.lw2 = wide_lw(l2);
  a.sx = wide_rec_floats(d, l1);
  a.sy = wide_rec_floats(d, l2);
  if (mf) return sig_fo_mf(a, d, seed, pl.mc ? ws_at(workspace, pl.o_mc) : nullptr, s);

  if (pl.dtiles) {
    // the diagonal's pairs in chunks: their seed tiles (two batched GEMMs + the anchors), then the launch
    int cp;
    const DiagTiles dt = diag_tiles_plan(n1, l1, &cp);
    float *T = ws_at(workspace, pl.o_dt);
    a.dtile = T;
    a.dt_pair = dt.pair;
    a.dt_rows = dt.rows;
    a.dt_ld = dt.ld;
    const int nchunks = diag_tile_chunks(row_begin, row_end, cp);
    for (int k = 0; k < nchunks; ++k) {
      const int c0 = row_begin + k * cp, c1 = c0 + cp < row_end ? c0 + cp : row_end;
      if ((rc = wide_diag_tiles(FX, a.sx, d, a.lw1, c0, c1 - c0, dt, T, s))) return rc;
      SigArgs c = a;
      c.row_begin = c0;
      c.row_end = c1;
      c.dt_a0 = c0;
      PairTiles t;
      if ((rc = pair_tiles(pair_mode, c0, c1, n2, 1, &t))) return rc;
      if ((rc = sig_fo_launch(c, DP, seed, t.nblocks, s))) return rc;
    }
    return GPSIG_OK;
  }
  const int LP = (order == 1) ? fo_lanes_per_pair(l2, DP, num_levels, mfma, seed, split) : ho_lanes_per_pair(l2, order, num_levels);
  if (LP == 0) return GPSIG_EUNSUPPORTED;
  PairTiles t;
  if ((rc = pair_tiles(pair_mode, row_begin, row_end, n2, 64 / LP, &t))) return rc;
  a.tiles_a0 = t.tiles_a0;
  a.ntb = t.ntb;
  a.tile_base = t.tile_base;
  return (order == 1) ? sig_fo_launch(a, DP, seed, t.nblocks, s) : sig_ho_launch(a, DP, seed, t.nblocks, s);
}

// gpsig_sig_fo_route: the choices of sig_gram_impl at order 1 (gpsig_sig_gram / gpsig_sig_diag, and
// gpsig_sig_gram_state where state != 0), in its order and by the helpers it calls: gram_plan, then sig_fo_mf's
// tiles and launches (sig_fo_mf_route), the diagonal's tile chunks (diag_tiles_plan, diag_tile_chunks), or
// fo_lanes_per_pair, pair_tiles and sig_fo_launch's geometry (sig_fo_route); no launch, no device
extern "C" int gpsig_sig_fo_route(int n1, int l1, int n2, int l2, int d, int num_levels, int base_kind,
                                  int difference, int pair_mode, int row_begin, int row_end, int state, int *out) {
  if (!out || num_levels < 1) return GPSIG_EINVAL;
  // the query has no inputs: out stands in for the pointers the shared check wants present
  if (check_pair_args(out, out, n1, l1, n2, l2, d, difference ? 2 : 1, pair_mode, row_begin, row_end, false))
    return GPSIG_EINVAL;
  // gpsig_sig_gram_state: difference seeds, RECT / UPPER, a state some pair fills
  if (state && (!difference || gpsig_sig_state_bytes(n1, n2, l2, num_levels, pair_mode) == 0)) return GPSIG_EINVAL;
  for (int i = 0; i < GPSIG_SIG_FO_ROUTE_INTS; ++i) out[i] = 0;
  if (base_kind & (GPSIG_BASE_SEED_MFMA | GPSIG_GRAM_SPLIT)) return GPSIG_EUNSUPPORTED;  // A/B variants: not described
  const int seed = seed_of(base_kind, difference);
  GramPlan pl{};
  const bool planned = gram_plan(n1, l1, n2, l2, d, num_levels, 1, seed, pair_mode, pair_mode != GPSIG_PAIRS_RECT,
                                 false, state != 0, &pl);
  if (seed < 0 || !planned) return GPSIG_EUNSUPPORTED;
  if (state && seed_is_radial(seed)) return GPSIG_EUNSUPPORTED;
  const bool diag = pair_mode == GPSIG_PAIRS_DIAG;
  FoRoute r{};
  int rc = GPSIG_OK, cp = 0, G = 0;
  if (pl.mf) {
    rc = sig_fo_mf_route(n2, l1, l2, d, num_levels, seed, pair_mode, row_begin, row_end, &r);
    r.carry = pl.mc;
  } else if (pl.dtiles) {
    diag_tiles_plan(n1, l1, &cp);
    const int nchunks = diag_tile_chunks(row_begin, row_end, cp);
    for (int k = 0; k < nchunks && !rc; ++k) {
      const int c0 = row_begin + k * cp, c1 = c0 + cp < row_end ? c0 + cp : row_end;
      PairTiles t;
      if ((rc = pair_tiles(pair_mode, c0, c1, n2, 1, &t))) break;
      rc = sig_fo_route(l1, l2, pl.DP, num_levels, seed, diag, state != 0, t.nblocks, &r);
    }
    if (nchunks == 0) rc = sig_fo_route(l1, l2, pl.DP, num_levels, seed, diag, state != 0, 0, &r);  // the geometry alone
    G = 64 / r.LP;
  } else {
    const int LP = fo_lanes_per_pair(l2, pl.DP, num_levels, false, seed, false);
    if (LP == 0) return GPSIG_EUNSUPPORTED;
    G = 64 / LP;
    PairTiles t{};
    if (row_end > row_begin && (rc = pair_tiles(pair_mode, row_begin, row_end, n2, G, &t))) return rc;
    rc = sig_fo_route(l1, l2, pl.DP, num_levels, seed, diag, state != 0, t.nblocks, &r);
  }
  auto clampi = [](unsigned long long v) { return v > 0x7fffffffULL ? 0x7fffffff : (int)v; };
  out[0] = pl.mf ? 2 : (pl.wide ? 1 : 0);
  out[1] = pl.DP;
  out[2] = r.W;
  out[3] = r.LP;
  out[4] = r.nblk;
  out[5] = clampi(r.carry);
  out[6] = pl.mf ? 0 : (diag ? 1 : G);
  out[7] = r.xb;
  out[8] = r.nw;
  out[9] = r.np;
  out[10] = r.cw;
  out[11] = pl.dtiles ? 1 : 0;
  out[12] = cp;
  out[13] = clampi((unsigned long long)r.workgroups);
  out[14] = r.launches;
  return row_end == row_begin ? GPSIG_OK : rc;  // no rows: the entry returns before any launch
}

// gpsig_sig_ho_route: the choices of sig_gram_impl at order > 1 and of sig_ho_launch / sig_ho_tiled under it,
// in sig_gram_impl's order and by the helpers it calls (ho_tiled, gram_plan, ho_lanes_per_pair, pair_tiles;
// sig_ho.hip: ho_w, ho_plan, the tile chunks); no launch, no device
extern "C" int gpsig_sig_ho_route(int n1, int l1, int n2, int l2, int d, int num_levels, int order, int base_kind,
                                  int difference, int pair_mode, int row_begin, int row_end, int *out) {
  if (!out || num_levels < 1 || order < 2) return GPSIG_EINVAL;
  // the query has no inputs: out stands in for the pointers the shared check wants present
  if (check_pair_args(out, out, n1, l1, n2, l2, d, difference ? 2 : 1, pair_mode, row_begin, row_end, false))
    return GPSIG_EINVAL;
  for (int i = 0; i < GPSIG_SIG_HO_ROUTE_INTS; ++i) out[i] = 0;
  if (base_kind & (GPSIG_BASE_SEED_MFMA | GPSIG_GRAM_SPLIT)) return GPSIG_EUNSUPPORTED;  // first-order variants
  const int seed = seed_of(base_kind, difference);
  const bool tiled = ho_tiled(d, order);
  if (tiled && seed != SEED_LIN_DIFF && seed != SEED_RBF_DIFF) return GPSIG_EUNSUPPORTED;
  GramPlan pl{};
  const bool planned = !tiled && gram_plan(n1, l1, n2, l2, d, num_levels, order, seed, pair_mode,
                                           pair_mode != GPSIG_PAIRS_RECT, false, false, &pl);
  if (seed < 0 || (!planned && !tiled)) return GPSIG_EUNSUPPORTED;
  HoRoute r{};
  int rc;
  if (tiled) {
    rc = sig_ho_tiled_route(n1, l1, n2, l2, d, num_levels, order, seed, pair_mode, row_begin, row_end, &r);
  } else {
    if (ho_lanes_per_pair(l2, order, num_levels) == 0) return GPSIG_EUNSUPPORTED;
    PairTiles t{};
    if (row_end > row_begin && (rc = pair_tiles(pair_mode, row_begin, row_end, n2, 1, &t))) return rc;
    rc = sig_ho_route(l1, l2, num_levels, order, seed, t.nblocks, &r);
  }
  out[0] = tiled ? 1 : 0;
  out[1] = tiled ? 0 : pl.DP;
  out[2] = r.W;
  out[3] = r.nblk;
  out[4] = r.split;
  out[5] = r.carry > 0x7fffffff ? 0x7fffffff : (int)r.carry;
  out[6] = r.launches;
  return row_end == row_begin ? GPSIG_OK : rc;  // no rows: the entry returns before any launch
}

extern "C" int gpsig_sig_gram(const float *X, int n1, int l1, const float *Y, int n2, int l2, int d, int num_levels,
                              int order, int base_kind, int difference, int pair_mode, int row_begin, int row_end,
                              const float *rs1, const float *rs2, const float *scale, float jitter, int out_mode,
                              float *out, int out_row0, int out_rows, void *workspace, size_t workspace_bytes,
                              gpsig_stream_t stream) {
  return sig_gram_impl(X, n1, l1, Y, n2, l2, d, num_levels, order, base_kind, difference, pair_mode, row_begin,
                       row_end, rs1, rs2, scale, jitter, out_mode, out, out_row0, out_rows, nullptr, workspace,
                       workspace_bytes, stream);
}

extern "C" size_t gpsig_sig_state_bytes(int n1, int n2, int l2, int num_levels, int pair_mode) {
  if (n1 <= 0 || n2 <= 0 || l2 < 2 || num_levels < 1) return 0;
  long long slots;
  if (pair_mode == GPSIG_PAIRS_RECT) slots = (long long)n1 * n2;
  else if (pair_mode == GPSIG_PAIRS_UPPER && n1 == n2) slots = (long long)n1 * (n1 + 1) / 2;
  else return 0;
  return (size_t)slots * (size_t)state_stride(num_levels, l2) * sizeof(float);
}

extern "C" int gpsig_sig_gram_state(const float *X, int n1, int l1, const float *Y, int n2, int l2, int d,
                                    int num_levels, int base_kind, int pair_mode, int row_begin, int row_end,
                                    const float *rs1, const float *rs2, const float *scale, float jitter,
                                    int out_mode, float *out, int out_row0, int out_rows, float *state,
                                    size_t state_bytes, void *workspace, size_t workspace_bytes,
                                    gpsig_stream_t stream) {
  if (!state) return GPSIG_EINVAL;
  if (pair_mode != GPSIG_PAIRS_RECT && pair_mode != GPSIG_PAIRS_UPPER) return GPSIG_EINVAL;
  const size_t need = gpsig_sig_state_bytes(n1, n2, l2, num_levels, pair_mode);
  if (need == 0) return GPSIG_EINVAL;
  if (state_bytes < need) return GPSIG_EWORKSPACE;
  return sig_gram_impl(X, n1, l1, Y, n2, l2, d, num_levels, 1, base_kind, 1, pair_mode, row_begin, row_end, rs1,
                       rs2, scale, jitter, out_mode, out, out_row0, out_rows, state, workspace, workspace_bytes,
                       stream);
}

extern "C" int gpsig_sig_diag(const float *X, int n, int l, int d, int num_levels, int order, int base_kind,
                              int difference, float jitter, int out_mode, float *out, void *workspace,
                              size_t workspace_bytes, gpsig_stream_t stream) {
  if (out_mode != GPSIG_OUT_LEVELS && out_mode != GPSIG_OUT_RSQRT) return GPSIG_EINVAL;
  return gpsig_sig_gram(X, n, l, X, n, l, d, num_levels, order, base_kind, difference, GPSIG_PAIRS_DIAG, 0, n,
                        nullptr, nullptr, nullptr, jitter, out_mode, out, 0, n, workspace, workspace_bytes, stream);
}

extern "C" size_t gpsig_pde_scratch_bytes(int n1, int l1, int n2, int l2, int d, int dyadic, int pair_mode) {
  if (!pde_tiled(d, dyadic)) return 0;
  return pde_tile_scratch_bytes(n1, l1, n2, l2, d, pair_mode);
}

extern "C" int gpsig_pde_gram_ex(const float *X, int n1, int l1, const float *Y, int n2, int l2, int d, int dyadic,
                                 int solver, int pair_mode, int row_begin, int row_end, float *out, int out_row0,
                                 int out_rows, void *scratch, size_t scratch_bytes, gpsig_stream_t stream) {
  if (!out || check_pair_args(X, Y, n1, l1, n2, l2, d, 2, pair_mode, row_begin, row_end, false)) return GPSIG_EINVAL;
  if (dyadic < 0 || dyadic > 8 || (solver != 0 && solver != 1)) return GPSIG_EINVAL;
  if (row_end == row_begin) return GPSIG_OK;
  if (pde_tiled(d, dyadic))
    return pde_launch_tiled(X, n1, l1, Y, n2, l2, d, dyadic, solver, pair_mode, row_begin, row_end, out, out_row0,
                            out_rows, n2, scratch, scratch_bytes, reinterpret_cast<hipStream_t>(stream));
  return pde_launch(X, n1, l1, Y, n2, l2, d, dyadic, solver, pair_mode, row_begin, row_end, out, out_row0,
                    out_rows, n2, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int gpsig_pde_gram(const float *X, int n1, int l1, const float *Y, int n2, int l2, int d, int dyadic,
                              int solver, int pair_mode, int row_begin, int row_end, float *out, int out_row0,
                              int out_rows, gpsig_stream_t stream) {
  return gpsig_pde_gram_ex(X, n1, l1, Y, n2, l2, d, dyadic, solver, pair_mode, row_begin, row_end, out, out_row0,
                           out_rows, nullptr, 0, stream);
}

extern "C" int gpsig_pde_diag_ex(const float *X, int n, int l, int d, int dyadic, int solver, float *out,
                                 void *scratch, size_t scratch_bytes, gpsig_stream_t stream) {
  return gpsig_pde_gram_ex(X, n, l, X, n, l, d, dyadic, solver, GPSIG_PAIRS_DIAG, 0, n, out, 0, n, scratch,
                           scratch_bytes, stream);
}

extern "C" int gpsig_pde_diag(const float *X, int n, int l, int d, int dyadic, int solver, float *out,
                              gpsig_stream_t stream) {
  return gpsig_pde_diag_ex(X, n, l, d, dyadic, solver, out, nullptr, 0, stream);
}

extern "C" int gpsig_sym_assemble(const float *src, const long long *row_off, long long level_stride, int n,
                                  int levels, float *dst, gpsig_stream_t stream) {
  if (!src || !dst || !row_off || n <= 0 || levels <= 0 || level_stride < 0) return GPSIG_EINVAL;
  return sym_assemble_launch(src, row_off, level_stride, n, levels, dst, reinterpret_cast<hipStream_t>(stream));
}

extern "C" const char *gpsig_version(void) { return "gpsig_amd 0.1 (gfx950)"; }
