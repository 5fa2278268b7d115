// Planar and quadratic sky subtraction on a [D, T] TOD (maria_amd/sky_polynomial.py): at every sample a
// low-order polynomial in the detectors' focal-plane positions, P [D][K] with K <= 6, is fitted across the rows of a
// group and subtracted.  The transpose of the regression of mrx_regress.hip: the templates run along the rows.
//   term(d, t)  = (double)x[d][t] - (double)model[d][t]                      (plain (double)x without a model)
//   r[g][i][t]  = sum over the participating rows d of group g with flags[d][t] == 0 of (u[d] * P[d][i]) * (term - off[d])
//   N[g][ij][t] = sum over the same rows of (v[d] * P[d][i]) * P[d][j], i <= j;   hits[g][t] = their number
//   c[g][.][t]  = the solution of N c = r by a scaled Cholesky factorisation (the operation order: include/mrx.h)
//   y[d][t]     = x[d][t] + sign * (float)(e[d] + h[d] * (sum over i, in order, of c[g][i][t] * P[d][i]))
// The file is built without FMA contraction: every operation above is one float64 rounding.
//
// Both kernels are resident grids over (group g, tile of 256 * OWN samples) items, as column_mean_kernel is: a workgroup
// walks ALL rows 0 .. D - 1 in ascending order, a row of another group is skipped before any of its samples is read (a
// scalar branch), and four rows' loads are in flight.  A sample's sums, its K x K system and its solve live in ONE thread:
// the order of the additions is the ascending row order of the group, whatever else shares the call.  The products that do
// not depend on t (u P_i, v P_i P_j) are computed once per row.
//
// The fit is compiled per K, so the triangle and the Cholesky factor unroll into registers, and per "flags given": without
// flags N and hits are the same for every sample, and a thread keeps ONE copy of them (the same additions in the same
// order: the bits of the per-sample sum).  A thread owns OWN consecutive samples: 4, but 2 at K = 5 and 6 with flags (27
// float64 accumulators a sample at K = 6), read and written by load_own<OWN> and store_own<OWN> (mrx_tod_dev.h).
#include "mrx_internal.h"
#include "mrx_tod_dev.h"

#include <algorithm>

namespace {

using mrx_tod::kThreads;
using mrx_tod::load_own;
using mrx_tod::store_own;

constexpr int kRows = 4;  // rows of a group a thread has in flight
constexpr int kMaxGroups = 16;
constexpr int kMaxTerms = 6;

enum : int { kWideX = 1, kWideM = 2, kWideF = 4, kWideY = 8 };

constexpr int own_of(int K, bool flags) { return K <= 4 || !flags ? 4 : 2; }

struct FitShape {
  size_t ld_x, ld_m, ld_f, ld_c;
  int D, T;
  unsigned min_n;  // max(min_hits, K)
  double rcond;
  int wide, tiles;
  long long n_items;
};

// The scaled Cholesky factor of one sample's system (include/mrx.h): n the upper triangle of N row after row.  L[i][k],
// k < i, q = 1 / L_ii and s = 1 / sqrt(N_ii); false where a diagonal entry is not > 0 or a pivot is below rcond
template <int K>
__device__ __forceinline__ bool factor(const double (&n)[K * (K + 1) / 2], double rcond, double (&L)[K][K], double (&qd)[K], double (&s)[K]) {
  bool good = true;
  double M[K][K];  // the upper triangle, M[i][j] with i <= j
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const double nii = n[i * K - i * (i - 1) / 2];
    good = good && nii > 0.0;
    s[i] = 1.0 / sqrt(nii);
  }
  int a = 0;
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int j = i; j < K; ++j, ++a) M[i][j] = (n[a] * s[i]) * s[j];
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    double p = M[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) p = p - L[j][k] * L[j][k];
    good = good && p >= rcond;  // a NaN compares false
    L[j][j] = sqrt(p);
    qd[j] = 1.0 / L[j][j];
#pragma unroll
    for (int i = j + 1; i < K; ++i) {
      double w = M[j][i];
#pragma unroll
      for (int k = 0; k < j; ++k) w = w - L[i][k] * L[j][k];
      L[i][j] = w * qd[j];
    }
  }
  return good;
}

template <int K, bool FLAGS>
__global__ __launch_bounds__(kThreads) void column_fit_kernel(const float* __restrict__ x, const float* __restrict__ model,
                                                              const unsigned char* __restrict__ flags, const int* __restrict__ group,
                                                              const double* __restrict__ P, const double* __restrict__ u,
                                                              const double* __restrict__ v, const double* __restrict__ off,
                                                              double* __restrict__ c_out, unsigned char* __restrict__ ok,
                                                              unsigned* __restrict__ hits, double* __restrict__ N, double* __restrict__ r_out,
                                                              const FitShape A) {
  constexpr int OWN = own_of(K, FLAGS);
  constexpr int NP = K * (K + 1) / 2;  // the upper triangle, row after row
  constexpr int NS = FLAGS ? OWN : 1;  // copies of N and hits a thread keeps
  constexpr int kTile = kThreads * OWN;
  const int T = A.T, D = A.D;
  for (long long item = blockIdx.x; item < A.n_items; item += gridDim.x) {
    const int g = (int)(item / A.tiles);
    const int q = (int)(item - (long long)g * A.tiles) * kTile + OWN * (int)threadIdx.x;
    if (q >= T) continue;  // nothing below synchronises the workgroup
    double rs[K][OWN], ns[NS][NP];
    unsigned hs[NS];
#pragma unroll
    for (int k = 0; k < OWN; ++k) {
#pragma unroll
      for (int i = 0; i < K; ++i) rs[i][k] = 0.0;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      hs[s] = 0u;
#pragma unroll
      for (int a = 0; a < NP; ++a) ns[s][a] = 0.0;
    }
    for (int d0 = 0; d0 < D; d0 += kRows) {
      bool in[kRows];
      float xv[kRows][OWN], mv[kRows][OWN];
      unsigned char fv[kRows][OWN];
#pragma unroll
      for (int r = 0; r < kRows; ++r) {  // the loads of up to four rows of the group go out together
        const int d = d0 + r;
        in[r] = d < D && (unsigned)(group ? group[d] : 0) == (unsigned)g && v[d] > 0.0;
        if (in[r]) {
          load_own<OWN>(x + (size_t)d * A.ld_x, q, T, A.wide & kWideX, xv[r]);
          if (model) load_own<OWN>(model + (size_t)d * A.ld_m, q, T, A.wide & kWideM, mv[r]);
          if (FLAGS) load_own<OWN>(flags + (size_t)d * A.ld_f, q, T, A.wide & kWideF, fv[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        if (in[r]) {
          const int d = d0 + r;
          const double ud = u[d], vd = v[d], od = off ? off[d] : 0.0;
          double p[K], up[K], vp[NP];  // uniform: once per row
#pragma unroll
          for (int i = 0; i < K; ++i) {
            p[i] = P[(size_t)d * K + i];
            up[i] = ud * p[i];
          }
          int a = 0;
#pragma unroll
          for (int i = 0; i < K; ++i) {
            const double vpi = vd * p[i];
#pragma unroll
            for (int j = i; j < K; ++j, ++a) vp[a] = vpi * p[j];
          }
#pragma unroll
          for (int k = 0; k < OWN; ++k) {
            const double term = model ? (double)xv[r][k] - (double)mv[r][k] : (double)xv[r][k];
            const double tm = term - od;
            const bool keep = !FLAGS || fv[r][k] == 0;
#pragma unroll
            for (int i = 0; i < K; ++i) {
              const double val = up[i] * tm;
              if (keep) rs[i][k] = rs[i][k] + val;  // selected, never multiplied: what a flagged sample holds is nothing
            }
            if (FLAGS && keep) {
              hs[k] += 1u;
#pragma unroll
              for (int b = 0; b < NP; ++b) ns[k][b] = ns[k][b] + vp[b];
            }
          }
          if (!FLAGS) {
            hs[0] += 1u;
#pragma unroll
            for (int b = 0; b < NP; ++b) ns[0][b] = ns[0][b] + vp[b];
          }
        }
      }
    }
    double L[K][K], qd[K], sc[K];
    bool good = false;
#pragma unroll
    for (int k = 0; k < OWN; ++k) {
      constexpr int kAll = 0;
      const int s = FLAGS ? k : kAll;
      if (FLAGS || k == 0) {
        good = factor<K>(ns[s], A.rcond, L, qd, sc);
        good = good && hs[s] >= A.min_n;
      }
      double z[K], c[K];
#pragma unroll
      for (int i = 0; i < K; ++i) {
        double w = rs[i][k] * sc[i];
#pragma unroll
        for (int j = 0; j < i; ++j) w = w - L[i][j] * z[j];
        z[i] = w * qd[i];
      }
#pragma unroll
      for (int i = K - 1; i >= 0; --i) {
        double w = z[i];
#pragma unroll
        for (int j = i + 1; j < K; ++j) w = w - L[j][i] * c[j];
        c[i] = w * qd[i];
      }
      if (q + k < T) {
        const size_t t = (size_t)q + k;
#pragma unroll
        for (int i = 0; i < K; ++i) c_out[((size_t)g * K + i) * A.ld_c + t] = good ? c[i] * sc[i] : 0.0;
        ok[(size_t)g * T + t] = good ? 1 : 0;
        if (hits) hits[(size_t)g * T + t] = hs[s];
        if (N) {
#pragma unroll
          for (int b = 0; b < NP; ++b) N[((size_t)g * NP + b) * T + t] = ns[s][b];
        }
        if (r_out) {
#pragma unroll
          for (int i = 0; i < K; ++i) r_out[((size_t)g * K + i) * T + t] = rs[i][k];
        }
      }
    }
  }
}

// Items 0 .. G * tiles - 1: (group, tile); from G * tiles on (out of place only): the rows of no group, copied.
// x and y may be the same buffer: a thread reads its samples before it writes them, and no other thread touches them
__global__ __launch_bounds__(kThreads) void column_apply_kernel(const float* x, size_t ld_x, int D, int T, const int* __restrict__ group, int G,
                                                                const double* __restrict__ P, int K, const double* __restrict__ c, size_t ld_c,
                                                                const double* __restrict__ e, const double* __restrict__ h, int sign, float* y,
                                                                size_t ld_y, int wide, int tiles, long long n_items) {
  constexpr int OWN = mrx_tod::kOwn;
  constexpr int kTile = mrx_tod::kTileSamples;
  for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int g = (int)(item / tiles);
    const int q = (int)(item - (long long)g * tiles) * kTile + OWN * (int)threadIdx.x;
    if (q >= T) continue;
    const bool fitted = g < G;
    double cv[kMaxTerms][OWN];
#pragma unroll
    for (int i = 0; i < kMaxTerms; ++i) {
#pragma unroll
      for (int k = 0; k < OWN; ++k) cv[i][k] = fitted && i < K && q + k < T ? c[((size_t)g * K + i) * ld_c + q + k] : 0.0;
    }
    for (int d0 = 0; d0 < D; d0 += kRows) {
      bool in[kRows];
      float xv[kRows][OWN];
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        const int d = d0 + r;
        const unsigned gd = d < D ? (unsigned)(group ? group[d] : 0) : 0u;
        in[r] = d < D && (fitted ? gd == (unsigned)g : gd >= (unsigned)G);
        if (in[r]) load_own<OWN>(x + (size_t)d * ld_x, q, T, wide & kWideX, xv[r]);
      }
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        if (in[r]) {
          const int d = d0 + r;
          if (fitted) {
            const double ed = e ? e[d] : 0.0, hd = h[d];
            double s[OWN];
#pragma unroll
            for (int k = 0; k < OWN; ++k) s[k] = 0.0;
#pragma unroll
            for (int i = 0; i < kMaxTerms; ++i) {
              if (i < K) {
                const double pi = P[(size_t)d * K + i];
#pragma unroll
                for (int k = 0; k < OWN; ++k) s[k] = s[k] + cv[i][k] * pi;
              }
            }
#pragma unroll
            for (int k = 0; k < OWN; ++k) {
              const float f = (float)(ed + hd * s[k]);
              xv[r][k] = sign < 0 ? xv[r][k] - f : xv[r][k] + f;
            }
          }
          store_own<OWN>(y + (size_t)d * ld_y, q, T, wide & kWideY, xv[r]);
        }
      }
    }
  }
}

template <int K, bool FLAGS>
void launch_fit(mrx_ctx* ctx, const float* x, const float* model, const uint8_t* flags, const int32_t* group, int G, const double* P,
                const double* u, const double* v, const double* off, double* c, uint8_t* ok, uint32_t* hits, double* N, double* r, FitShape A) {
  constexpr int OWN = own_of(K, FLAGS);
  A.wide = (mrx_aligned(x, A.ld_x * 4, 4 * OWN) ? kWideX : 0) | (model && mrx_aligned(model, A.ld_m * 4, 4 * OWN) ? kWideM : 0) |
           (FLAGS && mrx_aligned(flags, A.ld_f, OWN) ? kWideF : 0);
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, G, A.T, kThreads * OWN);  // items: (group, tile)
  A.tiles = g.tiles_per_row;
  A.n_items = g.n_tiles;
  hipLaunchKernelGGL((column_fit_kernel<K, FLAGS>), dim3(g.blocks), dim3(kThreads), 0, ctx->stream, x, model, flags, group, P, u, v, off, c, ok,
                     hits, N, r, A);
}

}  // namespace

extern "C" {

int mrx_tod_column_fit(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m, const uint8_t* d_flags, size_t ld_f,
                       int D, int T, const int32_t* d_group, int G, const double* d_P, int K, const double* d_u, const double* d_v,
                       const double* d_off, int min_hits, double rcond, double* d_c, size_t ld_c, uint8_t* d_ok, uint32_t* d_hits, double* d_N,
                       double* d_r) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_P && d_u && d_v && d_c && d_ok, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, G >= 1 && G <= kMaxGroups, "G must be in 1 .. 16");
  MRX_REQUIRE(ctx, K >= 1 && K <= kMaxTerms, "K must be in 1 .. 6");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && (!d_model || ld_m >= (size_t)T) && (!d_flags || ld_f >= (size_t)T) && ld_c >= (size_t)T,
              "ld_x, ld_m, ld_f or ld_c smaller than T");
  MRX_REQUIRE(ctx, rcond >= 0.0 && rcond < 1.0, "rcond must be in [0, 1)");
  MRX_REQUIRE(ctx, min_hits >= 1, "min_hits must be >= 1");
  const FitShape A{ld_x, ld_m, ld_f, ld_c, D, T, (unsigned)std::max(min_hits, K), rcond, 0, 0, 0};
#define MRX_FIT(KK)                                                                                                              \
  (d_flags ? launch_fit<KK, true>(ctx, d_x, d_model, d_flags, d_group, G, d_P, d_u, d_v, d_off, d_c, d_ok, d_hits, d_N, d_r, A) \
           : launch_fit<KK, false>(ctx, d_x, d_model, d_flags, d_group, G, d_P, d_u, d_v, d_off, d_c, d_ok, d_hits, d_N, d_r, A))
  switch (K) {
    case 1: MRX_FIT(1); break;
    case 2: MRX_FIT(2); break;
    case 3: MRX_FIT(3); break;
    case 4: MRX_FIT(4); break;
    case 5: MRX_FIT(5); break;
    default: MRX_FIT(6); break;
  }
#undef MRX_FIT
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_column_apply(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const int32_t* d_group, int G, const double* d_P, int K,
                         const double* d_c, size_t ld_c, const double* d_e, const double* d_h, int sign, float* d_y, size_t ld_y) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_P && d_c && d_h && d_y, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, G >= 1 && G <= kMaxGroups, "G must be in 1 .. 16");
  MRX_REQUIRE(ctx, K >= 1 && K <= kMaxTerms, "K must be in 1 .. 6");
  MRX_REQUIRE(ctx, sign == 1 || sign == -1, "sign must be -1 or +1");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && ld_y >= (size_t)T && ld_c >= (size_t)T, "ld_x, ld_y or ld_c smaller than T");
  MRX_REQUIRE(ctx, d_y != d_x || ld_y == ld_x, "in place (d_y == d_x) needs ld_y == ld_x");
  const bool copies = d_y != d_x && d_group;  // the rows of no group: there are none without d_group, and in place they stay
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, G + (copies ? 1 : 0), T, mrx_tod::kTileSamples);  // items: (group, tile)
  const int wide = (mrx_aligned(d_x, ld_x * 4, 16) ? kWideX : 0) | (mrx_aligned(d_y, ld_y * 4, 16) ? kWideY : 0);
  hipLaunchKernelGGL(column_apply_kernel, dim3(g.blocks), dim3(kThreads), 0, ctx->stream, d_x, ld_x, D, T, d_group, G, d_P, K, d_c, ld_c, d_e, d_h,
                     sign, d_y, ld_y, wide, g.tiles_per_row, g.n_tiles);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // extern "C"
