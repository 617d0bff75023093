// gpsig_amd -- instantiations of the LDS-state higher-order Gram VJP (sig_ho_bwd_lds.h) for one effective
// order (GPSIG_ORD): every level count whose multiplier slab fits the LDS, W = 4 (l2 <= 256) and 8 (l2 <= 512);
// the split kernels (257 .. 509 points on 4 waves, 510 .. 1017 on 8 waves with a global slab).
#include "internal.h"
#include "sig_ho_bwd_split.h"

#ifndef GPSIG_ORD
#error "GPSIG_ORD"
#endif

namespace gpsig {

// The plan (ho_bwd_plan, sig_ho_bwd_split.h) decides which of these runs; each asserts the plan's condition for
// its (order, levels), so a kernel whose state does not fit is never instantiated, and that its slab has the
// slots the plan counts.
template <int ORD, int M>
constexpr bool ho_slots_match() { return ho_bwd_slots(ORD, M) == HoBwdLayout<ORD, M>::np + HoBwdLayout<ORD, M>::ncb; }

template <int ORD, int M, int W>
static int launch_lds(const BwdArgs &a, int seed, long long nblocks, hipStream_t s) {
  constexpr size_t lds = ho_bwd_lds_slab_bytes<ORD, M, W>();
  static_assert(ho_slots_match<ORD, M>(), "slab slots");
  static_assert(ho_bwd_lds_ok(ORD, M, W) && lds + ho_bwd_lds_cbuf_bytes(W) <= HO_BWD_LDS_BUDGET, "LDS");
  if (seed == SEED_RBF_DIFF)
    hipLaunchKernelGGL((sig_ho_bwd_lds_kernel<ORD, M, W, SEED_RBF_DIFF>), dim3((unsigned)nblocks), dim3(64), lds, s, a);
  else if (seed == SEED_LIN_DIFF)
    hipLaunchKernelGGL((sig_ho_bwd_lds_kernel<ORD, M, W, SEED_LIN_DIFF>), dim3((unsigned)nblocks), dim3(64), lds, s, a);
  else
    return GPSIG_EUNSUPPORTED;
  return hipGetLastError() == hipSuccess ? GPSIG_OK : GPSIG_ELAUNCH;
}

// one pair over the 4 SIMDs of a CU (sig_ho_bwd_split.h): 257..509 points; GPSIG_HO_SPLIT=0 keeps the one-wave
// kernel (A/B)
template <int ORD, int M>
static int launch_split(const BwdArgs &a, int seed, long long nblocks, hipStream_t s) {
  constexpr size_t lds = ho_bwd_split_slab_bytes<ORD, M>();
  static_assert(ho_slots_match<ORD, M>() && lds == ho_bwd_split4_lds_bytes(ORD, M), "slab slots");
  static_assert(ho_bwd_split4_ok(ORD, M), "LDS");
  if (seed == SEED_RBF_DIFF)
    hipLaunchKernelGGL((sig_ho_bwd_split_kernel<ORD, M, SEED_RBF_DIFF>), dim3((unsigned)nblocks),
                       dim3(64 * HO_SPLIT_NW), lds, s, a);
  else if (seed == SEED_LIN_DIFF)
    hipLaunchKernelGGL((sig_ho_bwd_split_kernel<ORD, M, SEED_LIN_DIFF>), dim3((unsigned)nblocks),
                       dim3(64 * HO_SPLIT_NW), lds, s, a);
  else
    return GPSIG_EUNSUPPORTED;
  return hipGetLastError() == hipSuccess ? GPSIG_OK : GPSIG_ELAUNCH;
}

// 510 .. 1017 points: 8 waves per pair, 2 per SIMD, the slab in the caller's global region (a.scratch), at most
// HO_SPLIT8_BLOCKS workgroups per launch (each owns scr_stride floats of the region)
template <int ORD, int M>
static int launch_split8(BwdArgs a, const HoBwdPlan &pl, int seed, long long nblocks, hipStream_t s) {
  constexpr int NW = HO_SPLIT8_NW;
  static_assert(ho_slots_match<ORD, M>() && ho_split8_ok(ORD, M), "8-wave form");
  if (!a.scratch) return GPSIG_EWORKSPACE;
  static_assert(ho_split_slab_floats_rt(ORD, M, NW) == ho_split_slab_floats<ORD, M>(NW), "slab stride");
  a.scr_stride = pl.slab_floats;  // the stride the workspace's slab region was sized by
  for (long long b0 = 0; b0 < nblocks; b0 += HO_SPLIT8_BLOCKS) {
    const long long nb = nblocks - b0 < HO_SPLIT8_BLOCKS ? nblocks - b0 : HO_SPLIT8_BLOCKS;
    BwdArgs c = a;
    c.blk0 = a.blk0 + b0;
    if (seed == SEED_RBF_DIFF)
      hipLaunchKernelGGL((sig_ho_bwd_split_kernel<ORD, M, SEED_RBF_DIFF, NW>), dim3((unsigned)nb), dim3(64 * NW), 0, s, c);
    else if (seed == SEED_LIN_DIFF)
      hipLaunchKernelGGL((sig_ho_bwd_split_kernel<ORD, M, SEED_LIN_DIFF, NW>), dim3((unsigned)nb), dim3(64 * NW), 0, s, c);
    else
      return GPSIG_EUNSUPPORTED;
    if (hipGetLastError() != hipSuccess) return GPSIG_ELAUNCH;
  }
  return GPSIG_OK;
}

// launches what the plan says: a kernel is instantiated exactly where the plan can choose it for (ORD, M)
template <int ORD, int M>
static int launch_lds_w(const BwdArgs &a, const HoBwdPlan &pl, int seed, long long nblocks, hipStream_t s) {
  if constexpr (ho_split8_ok(ORD, M)) {
    if (pl.kernel == HO_BWD_SPLIT8) return launch_split8<ORD, M>(a, pl, seed, nblocks, s);
  }
  if constexpr (ho_bwd_lds_ok(ORD, M, 4)) {
    if (pl.kernel == HO_BWD_LDS && pl.W == 4) return launch_lds<ORD, M, 4>(a, seed, nblocks, s);
  }
  if constexpr (ho_bwd_split4_ok(ORD, M)) {
    if (pl.kernel == HO_BWD_SPLIT4) return launch_split<ORD, M>(a, seed, nblocks, s);
  }
  if constexpr (ho_bwd_lds_ok(ORD, M, 8)) {
    if (pl.kernel == HO_BWD_LDS && pl.W == 8) return launch_lds<ORD, M, 8>(a, seed, nblocks, s);
  }
  return GPSIG_EUNSUPPORTED;
}

template <>
int sig_ho_bwd_lds_launch_o<GPSIG_ORD>(const BwdArgs &a, const HoBwdPlan &pl, int seed, long long nblocks,
                                       hipStream_t s) {
  constexpr int O = GPSIG_ORD;
  return dispatch<2, 3, 4, 5, 6, 7, 8>(a.M, [&](auto lv) {
    constexpr int M = decltype(lv)::value;
    if constexpr (M >= O) return launch_lds_w<O, M>(a, pl, seed, nblocks, s); else return (int)GPSIG_EUNSUPPORTED;
  });
}

}  // namespace gpsig
