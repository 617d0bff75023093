// gpsig_amd -- VJP of the VOSF rescaled kernel (gpsig_rescaled, sig_tens.hip rescaled_kernel): the reverse of
// the block recursion of signature_algs_vosf.py:11-48 on the self-Gram of x_n.
//
// One wave handles one (sequence n, tensor t', level I); t' = T is the ones tensor.  Level I is its own chain of
// I stages over the components r0 .. r0+I-1 (r0 = I(I-1)/2) with seeds h_s(p,q) = sum_d lam_{r0+s,t',d} delta_d(p,q)
// and blocks R_s[a][b] = h_s P_s[a][b], a, b <= s (P_0 = 1):
//   P_{s+1}[0][0] = excl_q(sum_b CB_s[b])          P_{s+1}[0][y] = CB_s[y-1] / (y+1)
//   P_{s+1}[x][0] = excl_q(sum_b R_s[x-1][b]) / (x+1)   P_{s+1}[x][y] = R_s[x-1][y-1] / ((x+1)(y+1))
// CB_s[b] = column sums over the earlier rows of sum_a R_s[a][b];  K_I = sum of all cells of stage I-1.
//
// Sweep 1 runs the rows upwards and keeps only CB (I(I-1)/2 sums per column).  Sweep 2 runs the rows downwards:
// it takes the row's column sums out of CB again (stages in ascending order, so every stage sees the state before
// the row), keeps the row's multipliers P in LDS, and reverses the stages with G_s[a][b] = dLoss/dR_s[a][b]:
//   A[a][b]     = G_s[a][b] h_s / ((a+1)(b+1))
//   G_{s-1}[a][b] = GB_{s-1}[b] + exclsuffix_q(A[a+1][0]) + A[a+1][b+1]
//   GB_{s-1}[b] += exclsuffix_q(A[0][0]) + A[0][b+1]           (column sums over the later rows)
//   Dh_s        = sum_{a,b} G_s[a][b] P_s[a][b]               (= dLoss/dh_s(p,q))
// Nothing of size L^2 leaves the registers and the LDS.
//
// Rows and columns are the same sequence and every seed is symmetric, so Dh_s(p,q) = Dh_s(q,p): the column
// points' share of dLoss/dX equals the row points', and the kernel forms the row side only and doubles it.  The row
// side is wave-uniform: gZ[r0+s,t',d] += sum_q Dh_s delta_d, and with E_d = sum_s lam_{s,d} Dh_s
//   gx_{p+1,d} += 2 sum_q E_d ddelta_d/dx_{p+1,d},   gx_{p,d} += 2 sum_q E_d ddelta_d/dx_{p,d}
// are reduced over the wave per row and channel (a runtime channel loop).  The two x sums of a point nearly cancel
// (the adjoint of the increment is a difference of neighbouring rows), so their products and sums are formed in
// fp64 and meet in a two-row fp64 LDS accumulator; a point's row is complete once the row below it is done and
// leaves with one fp32 atomic per channel.  gZ of the level collects in LDS and leaves at the end.  A channel count
// whose accumulators do not fit the LDS (thousands) takes the direct form: the row's reduced sums go to gZ and gX as
// fp32 atomics at once.
#pragma once
#include <type_traits>

#include "common.h"
#include "host.h"

namespace gpsig {

struct RsBwdArgs {
  const float *Z;      // (LT, T, d)
  const float *X;      // (n, l, d)
  const float *gout;   // (M+1, n, T)
  const float *wones;  // (M, n): sum_t gout[i, n, t], the weight of K_i(ones)
  float *gZ, *gX;
  int t, n, l, d, M, emb;
  int direct;          // 1: no LDS accumulators, the reduced row sums go to global memory at once
};

template <int B, int E, class F>
GPSIG_DEV void rs_static_for(F &&f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    rs_static_for<B + 1, E>(f);
  }
}
// the same, downwards: f(E-1), ..., f(B)
template <int B, int E, class F>
GPSIG_DEV void rs_static_rfor(F &&f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, E - 1>{});
    rs_static_rfor<B, E - 1>(f);
  }
}

// multipliers of stages 1 .. I-1 kept per column: sum (s+1)^2
constexpr int rs_np(int I) {
  int n = 0;
  for (int s = 1; s < I; ++s) n += (s + 1) * (s + 1);
  return n;
}
constexpr int rs_poff(int s) { return rs_np(s); }         // first multiplier of stage s (s >= 1)
constexpr int rs_cboff(int s) { return s * (s + 1) / 2; }  // first column sum of stage s
// LDS of one wave: the multipliers, two point rows of x-gradient sums in fp64, the level's gZ sums
inline size_t rs_bwd_lds_bytes(int I, int W, int d, bool direct) {
  return ((size_t)rs_np(I) * 64 * W + (direct ? 0 : (size_t)4 * d + (size_t)I * d)) * sizeof(float);
}
constexpr size_t RS_BWD_LDS_MAX = 160 * 1024;

// Inclusive prefix sum over the wave in fp64 (lane 63: the total).
GPSIG_DEV double rs_wave_incl_scan_d(double v) {
  v += dpp_d<0x111>(v);
  v += dpp_d<0x112>(v);
  v += dpp_d<0x114>(v);
  v += dpp_d<0x118>(v);
  v += dpp_d<0x142, 0xA>(v);
  v += dpp_d<0x143, 0xC>(v);
  return v;
}

// Exclusive prefix (REV = false) or suffix (REV = true) sums over the 64 W columns col = lane W + w, N at once.
template <int N, int W, bool REV>
GPSIG_DEV void rs_xscan(const float (&v)[N][W], float (&o)[N][W]) {
  float t[N][W], tot[N];
  const int rl = 63 - (int)__lane_id();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if constexpr (!REV) {
      t[k][0] = v[k][0];
#pragma unroll
      for (int w = 1; w < W; ++w) t[k][w] = t[k][w - 1] + v[k][w];
      tot[k] = t[k][W - 1];
    } else {
      t[k][W - 1] = v[k][W - 1];
#pragma unroll
      for (int w = W - 2; w >= 0; --w) t[k][w] = t[k][w + 1] + v[k][w];
      tot[k] = __shfl(t[k][0], rl, 64);  // lanes mirrored: the suffix becomes a prefix
    }
  }
  group_incl_scan_n<64, N>(tot);
#pragma unroll
  for (int k = 0; k < N; ++k) {
    float base = lane_prev(tot[k]);  // lane 0 reads 0
    if constexpr (!REV) {
      o[k][0] = base;
#pragma unroll
      for (int w = 1; w < W; ++w) o[k][w] = base + t[k][w - 1];
    } else {
      base = __shfl(base, rl, 64);
      o[k][W - 1] = base;
#pragma unroll
      for (int w = W - 2; w >= 0; --w) o[k][w] = base + t[k][w + 1];
    }
  }
}

// One channel of the increment seed and its derivatives by the row points:
//   del = delta(p,q), a1 = d delta / d x_{p+1}, a0 = d delta / d x_p
// a = x_p, da = x_{p+1} - x_p, b = x_q, db = x_{q+1} - x_q.  RBF: delta is the second difference of
// e(u) = exp(-u^2/2); with p = log e(p+1,q)/e(p,q) etc. (sig_tens.hip rbf_second_diff) the expm1 form has no
// cancellation, and neither have the first differences of psi(u) = -u e(u) written on the same expm1 values.
template <bool RBF>
GPSIG_DEV void rs_seed(float a, float da, float b, float db, float &del, float &a1, float &a0) {
  if constexpr (!RBF) {
    del = da * db;
    a1 = db;
    a0 = -db;
  } else {
    const float df = a - b;
    const float p = __builtin_fmaf(-df, da, -0.5f * da * da);
    const float q = __builtin_fmaf(df, db, -0.5f * db * db);
    const float c = da * db;
    const float k00 = fast_exp(-0.5f * df * df);
    const float u10 = df + da, u01 = df - db, u11 = u10 - db;
    const float mx = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(p), __builtin_fabsf(q)), __builtin_fabsf(c));
    if (mx < EM1_TAU) {
      const float Ep = em1_small(p), Eq = em1_small(q), Ec = em1_small(c);
      del = k00 * __builtin_fmaf(Ep, Eq, (1.0f + Ep) * (1.0f + Eq) * Ec);
      const float Eqc = __builtin_fmaf(Eq, Ec, Eq + Ec);
      a1 = -k00 * (1.0f + Ep) * __builtin_fmaf(Eqc, u10, -(1.0f + Eqc) * db);
      a0 = k00 * __builtin_fmaf(Eq, df, -(1.0f + Eq) * db);
    } else {
      const float e11 = fast_exp(-0.5f * u11 * u11), e10 = fast_exp(-0.5f * u10 * u10);
      const float e01 = fast_exp(-0.5f * u01 * u01);
      del = (e11 - e10) - (e01 - k00);
      a1 = __builtin_fmaf(e10, u10, -e11 * u11);
      a0 = __builtin_fmaf(e01, u01, -k00 * df);
    }
  }
}

template <int I, int W, bool RBF>
__global__ __launch_bounds__(64) void rescaled_bwd_kernel(RsBwdArgs a) {
  extern __shared__ float rs_lds[];
  constexpr int NC = 64 * W;
  constexpr int NCB = I * (I - 1) / 2, NCBA = NCB > 0 ? NCB : 1;
  constexpr int r0 = I * (I - 1) / 2;
  const int lane = threadIdx.x;
  const int T = a.t, d = a.d, L = a.l;
  const int nn = (int)(blockIdx.x / (unsigned)(T + 1));
  const int tt = (int)(blockIdx.x % (unsigned)(T + 1));  // tt == T: the ones tensor
  const bool ones = tt == T;
  const float *x = a.X + (long long)nn * L * d;
  cfloat *xc = as_const(x);
  cfloat *zc = as_const(a.Z);
  float *Pl = rs_lds;                                                   // [rs_np(I)][NC]
  double *gxl = reinterpret_cast<double *>(rs_lds + rs_np(I) * NC);     // [2][d]: points of parity 0 / 1
  float *gzl = rs_lds + rs_np(I) * NC + 4 * d;                          // [I][d]
  if (!a.direct) {
    for (int e = lane; e < 2 * d; e += 64) gxl[e] = 0.0;
    for (int e = lane; e < I * d; e += 64) gzl[e] = 0.f;
    __syncthreads();
  }
  float *gxn = a.gX + (long long)nn * L * d;
  // weight of K_I for this pair: out = -K(t) + K(ones)
  const float wgt = ones ? a.wones[(long long)(I - 1) * a.n + nn] : -a.gout[((long long)I * a.n + nn) * T + tt];

  bool valid[W];
  int jjw[W];
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const int j = lane * W + w;
    valid[w] = j < L - 1;
    jjw[w] = j < L - 1 ? j : L - 2;
  }
  auto lam = [&](int s, int q) -> float { return ones ? 1.0f : zc[((long long)(r0 + s) * T + tt) * d + q]; };

  float CB[NCBA][W], GB[NCBA][W];
#pragma unroll
  for (int k = 0; k < NCBA; ++k)
#pragma unroll
    for (int w = 0; w < W; ++w) CB[k][w] = GB[k][w] = 0.f;

  // stage seeds of row pr: h[s][w] = sum_q lam_{s,q} delta_q(pr, col w), zero past the last column
  auto seeds = [&](int pr, float (&h)[I][W]) {
#pragma unroll
    for (int s = 0; s < I; ++s)
#pragma unroll
      for (int w = 0; w < W; ++w) h[s][w] = 0.f;
    for (int q = 0; q < d; ++q) {
      const float xq = xc[pr * d + q], dxq = xc[(pr + 1) * d + q] - xq;
      float dl[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const float xw = x[jjw[w] * d + q], dxw = x[(jjw[w] + 1) * d + q] - xw;
        float a1, a0;
        rs_seed<RBF>(xq, dxq, xw, dxw, dl[w], a1, a0);
        dl[w] = valid[w] ? dl[w] : 0.f;
      }
#pragma unroll
      for (int s = 0; s < I; ++s) {
        const float lq = lam(s, q);
#pragma unroll
        for (int w = 0; w < W; ++w) h[s][w] = __builtin_fmaf(lq, dl[w], h[s][w]);
      }
    }
  };

  // The stages of one row.  UNDO = false (sweep 1): CB += the row's column sums after their use.  UNDO = true
  // (sweep 2): CB -= the column sums first (the state before the row), and the multipliers go to LDS.
  auto stages = [&](const float (&h)[I][W], auto undo) {
    constexpr bool UNDO = decltype(undo)::value;
    float R[I][I][W];
#pragma unroll
    for (int w = 0; w < W; ++w) R[0][0][w] = h[0][w];
    rs_static_for<0, I - 1>([&](auto sc) {
      constexpr int s = decltype(sc)::value, n = s + 1, cb0 = rs_cboff(s);
      float colsum[n][W], sc_in[n + 1][W], sc_out[n + 1][W];
#pragma unroll
      for (int b = 0; b < n; ++b)
#pragma unroll
        for (int w = 0; w < W; ++w) {
          float cs = 0.f, rs = 0.f;
#pragma unroll
          for (int k = 0; k < n; ++k) {
            cs += R[k][b][w];
            rs += R[b][k][w];
          }
          colsum[b][w] = cs;
          sc_in[b + 1][w] = rs;
          if constexpr (UNDO) CB[cb0 + b][w] -= cs;
        }
#pragma unroll
      for (int w = 0; w < W; ++w) {
        float sv = 0.f;
#pragma unroll
        for (int b = 0; b < n; ++b) sv += CB[cb0 + b][w];
        sc_in[0][w] = sv;
      }
      rs_xscan<n + 1, W, false>(sc_in, sc_out);
      // multipliers of stage s+1, in place of R (descending: [x][y] reads [x-1][y-1])
#pragma unroll
      for (int x1 = n; x1 >= 1; --x1)
#pragma unroll
        for (int y1 = n; y1 >= 1; --y1) {
          const float f = 1.0f / (float)((x1 + 1) * (y1 + 1));
#pragma unroll
          for (int w = 0; w < W; ++w) R[x1][y1][w] = f * R[x1 - 1][y1 - 1][w];
        }
#pragma unroll
      for (int y1 = 1; y1 <= n; ++y1) {
        const float f = 1.0f / (float)(y1 + 1);
#pragma unroll
        for (int w = 0; w < W; ++w) R[0][y1][w] = f * CB[cb0 + y1 - 1][w];
      }
#pragma unroll
      for (int x1 = 1; x1 <= n; ++x1) {
        const float f = 1.0f / (float)(x1 + 1);
#pragma unroll
        for (int w = 0; w < W; ++w) R[x1][0][w] = f * sc_out[x1][w];
      }
#pragma unroll
      for (int w = 0; w < W; ++w) R[0][0][w] = sc_out[0][w];
      if constexpr (!UNDO) {
#pragma unroll
        for (int b = 0; b < n; ++b)
#pragma unroll
          for (int w = 0; w < W; ++w) CB[cb0 + b][w] += colsum[b][w];
      }
#pragma unroll
      for (int x1 = 0; x1 <= n; ++x1)
#pragma unroll
        for (int y1 = 0; y1 <= n; ++y1)
#pragma unroll
          for (int w = 0; w < W; ++w) {
            if constexpr (UNDO) Pl[(rs_poff(s + 1) + x1 * (n + 1) + y1) * NC + w * 64 + lane] = R[x1][y1][w];
            R[x1][y1][w] *= h[s + 1][w];
          }
    });
  };

  // ---- sweep 1: the column sums after the last row
  if constexpr (I > 1) {
    for (int pr = 0; pr < L - 1; ++pr) {
      float h[I][W];
      seeds(pr, h);
      stages(h, std::false_type{});
    }
  }

  // ---- sweep 2: rows downwards
  for (int pr = L - 2; pr >= 0; --pr) {
    float h[I][W], Dh[I][W];
    seeds(pr, h);
    stages(h, std::true_type{});
    float G[I][I][W];
#pragma unroll
    for (int x1 = 0; x1 < I; ++x1)
#pragma unroll
      for (int y1 = 0; y1 < I; ++y1)
#pragma unroll
        for (int w = 0; w < W; ++w) G[x1][y1][w] = wgt;
    rs_static_rfor<0, I>([&](auto sc) {
      constexpr int s = decltype(sc)::value, n = s + 1;
      if constexpr (s == 0) {
#pragma unroll
        for (int w = 0; w < W; ++w) Dh[0][w] = G[0][0][w];
      } else {
        constexpr int gb0 = rs_cboff(s - 1);
#pragma unroll
        for (int w = 0; w < W; ++w) Dh[s][w] = 0.f;
        float sc_in[s + 1][W], sc_out[s + 1][W];
#pragma unroll
        for (int x1 = 0; x1 < n; ++x1)
#pragma unroll
          for (int y1 = 0; y1 < n; ++y1) {
            const float f = 1.0f / (float)((x1 + 1) * (y1 + 1));
#pragma unroll
            for (int w = 0; w < W; ++w) {
              const float P = Pl[(rs_poff(s) + x1 * n + y1) * NC + w * 64 + lane];
              Dh[s][w] = __builtin_fmaf(G[x1][y1][w], P, Dh[s][w]);
              G[x1][y1][w] *= f * h[s][w];  // A[x1][y1]
            }
          }
#pragma unroll
        for (int x1 = 0; x1 < n; ++x1)
#pragma unroll
          for (int w = 0; w < W; ++w) sc_in[x1][w] = G[x1][0][w];
        rs_xscan<s + 1, W, true>(sc_in, sc_out);
        float Gn[s][s][W];
#pragma unroll
        for (int x1 = 0; x1 < s; ++x1)
#pragma unroll
          for (int y1 = 0; y1 < s; ++y1)
#pragma unroll
            for (int w = 0; w < W; ++w) Gn[x1][y1][w] = GB[gb0 + y1][w] + sc_out[x1 + 1][w] + G[x1 + 1][y1 + 1][w];
#pragma unroll
        for (int y1 = 0; y1 < s; ++y1)
#pragma unroll
          for (int w = 0; w < W; ++w) GB[gb0 + y1][w] += sc_out[0][w] + G[0][y1 + 1][w];
#pragma unroll
        for (int x1 = 0; x1 < s; ++x1)
#pragma unroll
          for (int y1 = 0; y1 < s; ++y1)
#pragma unroll
            for (int w = 0; w < W; ++w) G[x1][y1][w] = Gn[x1][y1][w];
      }
    });

    // row side of the seed's adjoint, channel by channel
    for (int q = 0; q < d; ++q) {
      const float xq = xc[pr * d + q], dxq = xc[(pr + 1) * d + q] - xq;
      float red[I];
      double g1 = 0.0, g0 = 0.0;
#pragma unroll
      for (int k = 0; k < I; ++k) red[k] = 0.f;
      float lq[I];
#pragma unroll
      for (int s = 0; s < I; ++s) lq[s] = lam(s, q);
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const float xw = x[jjw[w] * d + q], dxw = x[(jjw[w] + 1) * d + q] - xw;
        float dl, a1, a0;
        rs_seed<RBF>(xq, dxq, xw, dxw, dl, a1, a0);
        if (!valid[w]) dl = a1 = a0 = 0.f;
        float E = 0.f;
#pragma unroll
        for (int s = 0; s < I; ++s) {
          red[s] = __builtin_fmaf(Dh[s][w], dl, red[s]);
          E = __builtin_fmaf(lq[s], Dh[s][w], E);
        }
        g1 = __builtin_fma((double)E, (double)a1, g1);
        g0 = __builtin_fma((double)E, (double)a0, g0);
      }
      if (!ones) group_incl_scan_n<64, I>(red);  // lane 63: the wave's totals
      g1 = rs_wave_incl_scan_d(g1);
      g0 = rs_wave_incl_scan_d(g0);
      if (lane == 63) {
        if (!a.direct) {
          if (!ones) {
#pragma unroll
            for (int s = 0; s < I; ++s) gzl[s * d + q] += red[s];
          }
          gxl[((pr + 1) & 1) * d + q] += g1;
          gxl[(pr & 1) * d + q] += g0;
        } else {
          if (!ones) {
#pragma unroll
            for (int s = 0; s < I; ++s) unsafeAtomicAdd(a.gZ + ((long long)(r0 + s) * T + tt) * d + q, red[s]);
          }
          unsafeAtomicAdd(gxn + (long long)(pr + 1) * d + q, (float)(2.0 * g1));
          unsafeAtomicAdd(gxn + (long long)pr * d + q, (float)(2.0 * g0));
        }
      }
    }
    if (!a.direct) {
      // point pr + 1 has both its rows: out it goes (the symmetric column side doubles it), the slot is point pr - 1's
      __syncthreads();
      double *done = gxl + ((pr + 1) & 1) * d;
      for (int e = lane; e < d; e += 64) {
        unsafeAtomicAdd(gxn + (long long)(pr + 1) * d + e, (float)(2.0 * done[e]));
        done[e] = 0.0;
      }
      __syncthreads();
    }
  }

  if (!a.direct) {
    for (int e = lane; e < d; e += 64) unsafeAtomicAdd(gxn + e, (float)(2.0 * gxl[e]));  // point 0
    if (!ones)
      for (int e = lane; e < I * d; e += 64)
        unsafeAtomicAdd(a.gZ + ((long long)(r0 + e / d) * T + tt) * d + e % d, gzl[e]);
  }
}

// the instantiations of one level (sig_rescaled_bwd_inst.hip): W = 1 / 2 / 4 (level <= 4) columns per lane
template <int I>
int rescaled_bwd_launch_level(const RsBwdArgs &a, hipStream_t s);

}  // namespace gpsig
