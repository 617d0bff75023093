// gpsig_amd -- the one place for declarations that cross translation units: every non-template function that
// one .hip file defines and another calls, and the per-instantiation launch templates (defined and explicitly
// instantiated in the *_inst.hip units).  Every file that defines or calls one of them includes this header,
// so the compiler checks the definition against the declaration; default arguments live only here.  Also the
// pair-mode tile counts shared by the launchers.
#pragma once
#include "host.h"
#include "sig_common.h"

namespace gpsig {

struct BwdArgs;     // sig_bwd.h
struct BwdGeo;      // sig_bwd.h
struct MfArgs;      // sig_fo_mf.h
struct TvsBwdArgs;  // sig_tvs_bwd.h
struct DiagTiles;   // wide.h

// ---- sig_fo.hip: feature records, the first-order forward and its geometry
int features(const float *X, int n, int l, int d, int DP, float *F, hipStream_t s);
int wide_records(const float *X, int n, int l, int d, float *R, hipStream_t s);
int sig_fo_launch(const SigArgs &a, int DP, int seed, long long nblocks, hipStream_t s);
int fo_lanes_per_pair(int l2, int DP, int M, bool mf, int seed, bool split);
void fo_wide_geo(int l2, int seed, int *W, int *LP);
size_t fo_split_bytes(int l1, int l2, int DP, int M);
template <int DP, int M>
int sig_fo_launch_dpm(const SigArgs &a, int seed, long long nblocks, hipStream_t s);  // sig_fo_inst.hip
// gpsig_sig_fo_route: what sig_fo_launch (nblocks workgroups) / sig_fo_mf would choose, and their return
// (include/gpsig_amd.h for the values; workgroups and launches add up over the calls of one query)
struct FoRoute {
  int W, LP, nblk;      // columns per lane, lanes per pair, column blocks
  int nw, np, cw, xb;   // matrix cores: waves per workgroup, operand parts, floats per carry row, x-sequences per workgroup
  int launches;         // kernel launches
  long long workgroups;
  size_t carry;         // dynamic LDS of a blocked launch's carries (sig_fo_launch)
};
int sig_fo_route(int l1, int l2, int DP, int M, int seed, bool diag, bool state, long long nblocks, FoRoute *r);

// ---- sig_f64_inst.hip: the float64 first-order kernels of one level count
struct F64Args;  // sig_f64.h
template <int M>
int sig_f64_launch_m(const F64Args &a, int W, int LP, long long nblocks, hipStream_t s);

// ---- sig_fo_mf.hip: the matrix-core wide Gram
int mf_records(const float *X, int n, int l, int d, float *R, hipStream_t s);
size_t mf_records_bytes(int n, int l, int d);
bool mf_gram_applies(int d, int l2);
size_t mf_gram_scratch_bytes(int l1, int l2, int d);
int sig_fo_mf(const SigArgs &a, int d, int seed, float *scratch, hipStream_t s);
int sig_fo_mf_route(int n2, int l1, int l2, int d, int M, int seed, int pair_mode, int row_begin, int row_end,
                    FoRoute *r);
int sig_fo_mf_cells(const float *FX, int n1, int l1, const float *FY, int n2, int l2, int d, int pair_mode,
                    int row_begin, int row_end, float *dm, int dm_a0, int dm_b0, long long dm_as, long long dm_bs,
                    long long dm_ld, hipStream_t s);
int sig_fo_mf_cells_launch(const MfArgs &a, long long nblocks, hipStream_t s);  // sig_fo_mf_inst.hip (M = 1)

// ---- sig_ho.hip: the higher-order forward
int sig_ho_launch(const SigArgs &a, int DP, int seed, long long nblocks, hipStream_t s);
int ho_lanes_per_pair(int l2, int order, int M);
bool ho_tiled(int d, int order);
size_t ho_tile_bytes(int n1, int l1, int n2, int l2, int d, int pair_mode);
int sig_ho_tiled(SigArgs a, const float *X, const float *Y, int d, int seed, void *workspace, size_t workspace_bytes,
                 hipStream_t s);
// gpsig_sig_ho_route: what sig_ho_launch (nblocks workgroups) / sig_ho_tiled would choose, and their return
struct HoRoute {
  int W, nblk, split, launches;  // columns per lane, column blocks, SPLIT kernel, kernel launches (tile mode: chunks)
  size_t carry;                  // dynamic LDS of the plain blocked kernel's carries
};
int sig_ho_route(int l1, int l2, int M, int order, int seed, long long nblocks, HoRoute *r);
int sig_ho_tiled_route(int n1, int l1, int n2, int l2, int d, int M, int order, int seed, int pair_mode,
                       int row_begin, int row_end, HoRoute *r);

// ---- pde.hip: the Goursat PDE forward and the increment tiles
int pde_launch(const float *X, int n1, int l1, const float *Y, int n2, int l2, int d, int dyadic, int solver,
               int pair_mode, int row_begin, int row_end, float *out, int out_row0, int out_rows,
               long long out_ld, hipStream_t s);
int pde_launch_tiled(const float *X, int n1, int l1, const float *Y, int n2, int l2, int d, int dyadic, int solver,
                     int pair_mode, int row_begin, int row_end, float *out, int out_row0, int out_rows,
                     long long out_ld, void *scratch, size_t scratch_bytes, hipStream_t s);
bool pde_tiled(int d, int dyadic);
// channel instantiation of the fixed PDE kernels, forward and adjoint (0: none, the increment tiles)
inline int pde_dp(int d) { return d <= 8 ? d : (d <= 16 ? 16 : 0); }
// gpsig_pde_route's forward half: out[0..6] = family, DP, REP, W, LP, column blocks, sub (include/gpsig_amd.h)
int pde_fwd_route(int l1, int l2, int d, int dyadic, int solver, int pair_mode, int *out);
void pde_tile_chunk(int n1, int l1, int n2, int l2, int pair_mode, int &rows, long long &cols);
size_t pde_tile_scratch_bytes(int n1, int l1, int n2, int l2, int d, int pair_mode);
int increments_launch(const float *X, int n, int l, int d, float *dX, hipStream_t s);
int sym_assemble_launch(const float *src, const long long *row_off, long long level_stride, int n, int levels,
                        float *dst, hipStream_t s);

// ---- sig_bwd_inst.hip / sig_bwd_wide_inst.hip: the first-order VJP's instantiations
template <int DP, int M>
int sig_bwd_launch_dpm(const BwdArgs &a, int seed, long long nblocks, hipStream_t s);
template <int DP, int M>
int sig_bwd_pk_launch_dpm(const BwdArgs &a, int seed, BwdGeo geo, long long nblocks, hipStream_t s);
template <int M>
int sig_bwd_wide_launch_m(const BwdArgs &a, int seed, long long nblocks, hipStream_t s);

// ---- sig_bwd_wide.hip: the VJPs on point-weight tiles, the diagonal's seed tiles
size_t sig_bwd_wide_workspace(int n1, int l1, int n2, int l2, int d);
int sig_bwd_wide(BwdArgs a, const float *X, const float *Y, int seed, void *workspace, size_t workspace_bytes,
                 hipStream_t s, int order = 1);
DiagTiles diag_tiles_of(int l, int W, int LP);
bool diag_tiles_apply(int l, int d, int W, int LP, int seed, int order);
int wide_diag_tiles(const float *FX, long long sx, int d, int lw, int a0, int npairs, DiagTiles dt, float *T,
                    hipStream_t s);

// ---- sig_ho_bwd.hip: the higher-order VJP
bool ho_bwd_supported(int l2, int order, int M, int seed);
size_t ho_bwd_slab_bytes(int l2, int order, int M);
int sig_ho_bwd_launch(const BwdArgs &a, int order, int seed, long long nblocks, hipStream_t s);
// gpsig_sig_vjp_ho_route: the plan sig_ho_bwd_launch follows (ho_bwd_plan, sig_ho_bwd_split.h), the slab region
// of the workspace, and the row chunks and kernel launches of sig_bwd_wide (include/gpsig_amd.h for the values)
struct HoVjpRoute {
  int kernel, W, waves, slots, variant, chunks, launches;
  size_t lds_bytes, slab_bytes;
};
bool sig_ho_bwd_route_plan(int l2, int order, int M, HoVjpRoute *r);  // false: no kernel covers the shape
// launches of one chunk of sig_bwd_wide: rows [row_begin, row_end), nblocks pair tiles
int sig_ho_bwd_route_launches(int l2, int order, int M, int pair_mode, int row_begin, int row_end, int n2,
                              long long nblocks, int *launches);
// sig_bwd_wide.hip: r->chunks and r->launches of a call over rows [row_begin, row_end), and its return code
int sig_bwd_wide_ho_route(int n1, int l1, int n2, int l2, int d, int M, int order, int seed, int pair_mode,
                          int row_begin, int row_end, HoVjpRoute *r);

// ---- sig_tens.hip / sig_tvs_pk.hip: tensors against sequences
size_t tvs_features_bytes(int n, int l, int d);
int tvs_features_launch(const float *X, int n, int l, int d, float *Ft, hipStream_t s);
int tvs_pk_launch(const float *Z, int lt, int t, int increments, int d, const float *Ft, int n, int l, int M,
                  float *out, float *Zp, bool rbf, float *state, hipStream_t s);
int tvs_wide_launch(const float *Z, int lt, int t, int increments, int d, const float *X, const float *Ft, int n,
                    int l, int M, float *out, float *Zw, bool rbf, float *state, void *seedws, hipStream_t s);
size_t tvs_pk_zp_bytes(int lt, int t, int d);
size_t tvs_seed_bytes(int n, int l, int d, int lt, int t);
size_t tvs_tile_budget();  // GPSIG_TVS_TILE_BYTES

// ---- sig_tvs_bwd_inst.hip / sig_tvs_bwd_wide.hip: the tens-vs-seq VJP
template <int DP, bool INCR>
int tvs_bwd_launch_dp(const TvsBwdArgs &a, int M, bool rbf, bool diff, hipStream_t s);
size_t tvs_bwd_wide_workspace(int n, int l, int d, int lt, int t);
int tvs_bwd_wide(const float *Z, int lt, int t, int incr, int d, const float *X, int n, int l, int M, bool rbf,
                 bool diff, const float *gout, float *gZ, float *gX, const float *state, void *workspace,
                 size_t workspace_bytes, hipStream_t s);

// ---- tens_vjp_mm.hip: the tensor Gram and its VJP past 32 channels
size_t tens_gram_mm_bytes(int lt, int t);
int tens_gram_mm(const float *Z, int lt, int t, int incr, int d, int M, int rbf, float *out, void *workspace,
                 size_t workspace_bytes, hipStream_t s);
size_t tens_gram_vjp_mm_bytes(int lt, int t, int incr, int d, int rbf);
int tens_gram_vjp_mm(const float *Z, int lt, int t, int incr, int d, int M, int rbf, const float *gout, float *gZ,
                     void *workspace, size_t workspace_bytes, hipStream_t s);

// ---- pair-mode tile counts
// Workgroups of a launch over the pairs of rows [row_begin, row_end): 4 x-sequences (one per wave) against
// G y-sequences per workgroup.  DIAG: the pairs (a, a); RECT: tile rows x ntb B tiles; UPPER: the tiles with
// some b >= a, tile row r starting at B tile floor(4 r / G) (upper_prefix_g; G = 6 for the 10-lane groups is
// not a whole ratio).  GPSIG_EUNSUPPORTED past 2^31 - 1 workgroups.
struct PairTiles {
  long long nblocks, tile_base;
  int tiles_a0, ntb;
};
inline int pair_tiles(int pair_mode, int row_begin, int row_end, int n2, int G, PairTiles *t) {
  *t = PairTiles{};
  if (pair_mode == GPSIG_PAIRS_DIAG) {
    t->nblocks = (row_end - row_begin + 3) / 4;
  } else {
    const int ta0 = row_begin / 4, ta1 = (row_end + 3) / 4;
    t->tiles_a0 = ta0;
    t->ntb = (n2 + G - 1) / G;
    if (pair_mode == GPSIG_PAIRS_RECT) {
      t->nblocks = (long long)(ta1 - ta0) * t->ntb;
    } else {
      t->tile_base = upper_prefix_g(ta0, t->ntb, G);
      t->nblocks = upper_prefix_g(ta1, t->ntb, G) - t->tile_base;
    }
  }
  return t->nblocks > 0x7fffffffLL ? GPSIG_EUNSUPPORTED : GPSIG_OK;
}

}  // namespace gpsig
