// gpsig_amd -- host-side helpers shared by the entry points and the launchers (plain C++17, no device code):
// 256-byte alignment and workspace carving, the environment knobs' reader, value-to-template dispatch and the
// argument checks every pair-mode entry point shares.
#pragma once
#include <stddef.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/gpsig_amd.h"

namespace gpsig {

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Workspace regions in carve order.  take(bytes) returns the region's offset; a plan keeps the offsets and
// total(), so the size query and the entry's pointers come from the same arithmetic.  Sizes are taken as
// given (callers align the regions that need it).
struct Carver {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off += bytes;
    return o;
  }
  size_t total() const { return off; }
};
inline float *ws_at(void *base, size_t off) { return reinterpret_cast<float *>(static_cast<char *>(base) + off); }

// Environment knobs (A/B runs, tests).  These read the variable now; a knob that is read once keeps the value
// in a function-local static at its accessor.
inline int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline long long env_ll(const char *name, long long dflt) {
  const char *e = getenv(name);
  return e ? atoll(e) : dflt;
}
inline char env_char(const char *name) {  // first character, '\0' when unset
  const char *e = getenv(name);
  return e ? e[0] : '\0';
}
inline int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// GPSIG_HO_SPLIT=0 keeps the one-wave / plain higher-order kernels (sig_ho.hip, sig_ho_bwd_lds_inst.hip); read
// per call (the tests switch it between calls)
inline bool ho_split_on() { return env_char("GPSIG_HO_SPLIT") != '0'; }

// Runtime value -> template argument: f(std::integral_constant<int, V>{}) for the V of the list equal to v,
// GPSIG_EUNSUPPORTED for a value not in the list.  Each site lists the values it has instantiations for:
//   dispatch<1, 2, 3>(M, [&](auto m) { return launch<m.value>(args); })
template <int... Vs, class F>
inline int dispatch(int v, F &&f) {
  int rc = GPSIG_EUNSUPPORTED;
  // a left fold: the branches are instantiated (and their kernels emitted) in the order of the list
  (void)(... || (v == Vs ? (rc = f(std::integral_constant<int, Vs>{}), true) : false));
  return rc;
}

// The argument checks the pair-mode entry points share (GPSIG_EINVAL or GPSIG_OK): inputs present, positive
// counts, sequences of at least lmin points, a valid pair mode and row window; the UPPER / DIAG modes pair X
// with itself (same shapes, and the same pointer where same_ptr); rs1 / rs2 come together or not at all.
inline int check_pair_args(const void *X, const void *Y, int n1, int l1, int n2, int l2, int d, int lmin,
                           int pair_mode, int row_begin, int row_end, bool same_ptr, const void *rs1 = nullptr,
                           const void *rs2 = nullptr) {
  if (!X || !Y || n1 <= 0 || n2 <= 0 || d <= 0 || l1 < lmin || l2 < lmin) return GPSIG_EINVAL;
  if (pair_mode < GPSIG_PAIRS_RECT || pair_mode > GPSIG_PAIRS_DIAG) return GPSIG_EINVAL;
  if (row_begin < 0 || row_end > n1 || row_begin > row_end) return GPSIG_EINVAL;
  if (pair_mode != GPSIG_PAIRS_RECT && (n1 != n2 || l1 != l2 || (same_ptr && X != Y))) return GPSIG_EINVAL;
  if ((rs1 == nullptr) != (rs2 == nullptr)) return GPSIG_EINVAL;
  return GPSIG_OK;
}

}  // namespace gpsig
