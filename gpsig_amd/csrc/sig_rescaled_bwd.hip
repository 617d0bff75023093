// gpsig_amd -- gpsig_rescaled_vjp: the gradient of gpsig_rescaled (sig_tens.hip) by Z and X.  The kernel is
// sig_rescaled_bwd.h, instantiated per level in sig_rescaled_bwd_inst.hip; this unit holds the entry point, its
// argument checks and the weights of the ones tensor.
#include "internal.h"
#include "sig_rescaled_bwd.h"

namespace gpsig {

// wones[i-1][n] = sum_t gout[i][n][t]: out = -K(t) + K(ones), so K_i(ones) of sequence n collects every t
__global__ __launch_bounds__(64) void rescaled_bwd_wones_kernel(const float *gout, int M, int n, int t, float *wones) {
  const long long row = blockIdx.x;  // (i-1) * n + nn
  const float *g = gout + ((long long)n + row) * t;
  float s = 0.f;
  for (int k = threadIdx.x; k < t; k += 64) s += g[k];
  s = group_sum<64>(s);
  if (threadIdx.x == 0) wones[row] = s;
}

}  // namespace gpsig

using namespace gpsig;

// the forward's envelope (sig_tens.hip rs_w): l - 1 <= 128, or <= 256 up to four levels
static bool rs_bwd_supported(int l, int num_levels) {
  if (num_levels < 1 || num_levels > 6) return false;
  return l - 1 <= 128 || (num_levels <= 4 && l - 1 <= 256);
}

extern "C" int gpsig_rescaled_vjp(const float *Z, int lt, int t, const float *X, int n, int l, int d, int num_levels,
                                  int embedding, const float *gout, float *gZ, float *gX, void *workspace,
                                  size_t workspace_bytes, gpsig_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!Z || !X || !gout || !gZ || !gX || t <= 0 || n <= 0 || l < 2 || d <= 0 || num_levels < 1) return GPSIG_EINVAL;
  if (lt != num_levels * (num_levels + 1) / 2 || (embedding != 0 && embedding != 1)) return GPSIG_EINVAL;
  if (!rs_bwd_supported(l, num_levels)) return GPSIG_EUNSUPPORTED;
  if ((long long)n * (t + 1) > 0x7fffffffLL || (long long)n * num_levels > 0x7fffffffLL) return GPSIG_EUNSUPPORTED;
  // wones (num_levels, n): the size of the forward's K(ones) buffer, so the forward's query serves both
  if (!workspace || workspace_bytes < gpsig_rescaled_workspace_bytes(n, num_levels)) return GPSIG_EWORKSPACE;
  float *wones = static_cast<float *>(workspace);
  hipLaunchKernelGGL(rescaled_bwd_wones_kernel, dim3((unsigned)(n * num_levels)), dim3(64), 0, s, gout, num_levels, n,
                     t, wones);
  if (hipGetLastError() != hipSuccess) return GPSIG_ELAUNCH;
  RsBwdArgs a{Z, X, gout, wones, gZ, gX, t, n, l, d, num_levels, embedding, 0};
  // the levels are independent chains: one launch each, the longest first
  for (int i = num_levels; i >= 1; --i) {
    const int rc = dispatch<1, 2, 3, 4, 5, 6>(
        i, [&](auto lv) { return rescaled_bwd_launch_level<decltype(lv)::value>(a, s); });
    if (rc) return rc;
  }
  return GPSIG_OK;
}
