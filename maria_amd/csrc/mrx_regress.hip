// Common-mode removal as a flag-aware template regression on a [D, T] TOD (maria_amd/regress.py):
//   term(d, t)  = (double)x[d][t] - (double)model[d][t]                      (plain (double)x without a model)
//   S[g][t]     = sum over rows d of group g with flags[d][t] == 0 of u[d] * (term(d, t) - off[d]),   W[g][t] = sum of v[d]
//   mean[g][t]  = W > 0 ? (float)(S / W) : 0
//   N[d][i][j]  = sum over t with flags[d][t] == 0 of (double)B[g][i][t] * (double)B[g][j][t]
//   r[d][i]     = sum over the same t of (double)B[g][i][t] * term(d, t),    hits[d] = their number
//   y[d][t]     = x[d][t] + sign * (float)(sum over i, in order, of a[d][i] * (double)B[g][i][t])
// The file is built without FMA contraction: every operation above is one float64 rounding.
//
// Sample ownership is the same in all three kernels: the tile and a thread's own four samples of mrx_tod_dev.h.
//
// mrx_tod_column_mean.  A workgroup takes (group g, tile of 1024 samples) and walks ALL rows 0 .. D - 1 in ascending
// order; a row of another group is skipped before any of its samples is read (the group is uniform: a scalar branch),
// so a row is read by the workgroups of its own group only.  A sample's two sums live in one thread: the order of the
// additions is the ascending row order of the group, whatever else shares the call.  Four rows are in flight.
//
// mrx_tod_regress_normal.  A workgroup takes one row and walks its tiles in ascending order; a thread adds its samples
// into K (K + 1) / 2 + K float64 accumulators in registers (the upper triangle of N, and r), the 64 lanes of a wave meet
// (mrx_tod_dev.h: wave_sum_all), the four waves in LDS, wave 0 first.  The order is a function of T alone.  The kernel is
// compiled for K classes 2, 4 and 8; a flagged sample enters as a row of zeros (selected, never multiplied by x).
//
// mrx_tod_regress_apply.  A streaming pass over (row, tile); the row's K coefficients are uniform.
#include "mrx_internal.h"
#include "mrx_tod_dev.h"

#include <algorithm>

namespace {

using namespace mrx_tod;  // the 256-thread, four-sample tile, kWave

constexpr int kRows = 4;  // rows of a group a thread of the column mean has in flight
constexpr int kMaxGroups = 16;
constexpr int kMaxTemplates = 8;

enum : int { kWideX = 1, kWideM = 2, kWideF = 4, kWideB = 8, kWideY = 16 };

__global__ __launch_bounds__(kThreads) void column_mean_kernel(const float* __restrict__ x, size_t ld_x, const float* __restrict__ model,
                                                               size_t ld_m, const unsigned char* __restrict__ flags, size_t ld_f, int D, int T,
                                                               const int* __restrict__ group, const double* __restrict__ u,
                                                               const double* __restrict__ v, const double* __restrict__ off,
                                                               double* __restrict__ S, double* __restrict__ W, float* __restrict__ mean,
                                                               size_t ld_c, int wide, int tiles, long long n_items) {
  for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int g = (int)(item / tiles);
    const int q = (int)(item - (long long)g * tiles) * kTileSamples + kOwn * (int)threadIdx.x;
    if (q >= T) continue;  // nothing below synchronises the workgroup
    double s[kOwn], w[kOwn];
#pragma unroll
    for (int k = 0; k < kOwn; ++k) s[k] = w[k] = 0.0;
    for (int d0 = 0; d0 < D; d0 += kRows) {
      bool in[kRows];
      float xv[kRows][kOwn], mv[kRows][kOwn];
      unsigned char fv[kRows][kOwn];
#pragma unroll
      for (int r = 0; r < kRows; ++r) {  // the loads of up to four rows of the group go out together
        const int d = d0 + r;
        in[r] = d < D && (unsigned)(group ? group[d] : 0) == (unsigned)g;
        if (in[r]) {
          load_own<kOwn>(x + (size_t)d * ld_x, q, T, wide & kWideX, xv[r]);
          if (model) load_own<kOwn>(model + (size_t)d * ld_m, q, T, wide & kWideM, mv[r]);
          load_own_or_none<kOwn>(flags ? flags + (size_t)d * ld_f : nullptr, q, T, wide & kWideF, fv[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        if (in[r]) {
          const int d = d0 + r;
          const double ud = u[d], vd = v[d], od = off ? off[d] : 0.0;
#pragma unroll
          for (int k = 0; k < kOwn; ++k) {
            const double term = model ? (double)xv[r][k] - (double)mv[r][k] : (double)xv[r][k];
            const double val = ud * (term - od);
            if (fv[r][k] == 0) {
              s[k] = s[k] + val;
              w[k] = w[k] + vd;
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kOwn; ++k) {
      if (q + k < T) {
        if (S) S[(size_t)g * T + q + k] = s[k];
        if (W) W[(size_t)g * T + q + k] = w[k];
        if (mean) mean[(size_t)g * ld_c + q + k] = w[k] > 0.0 ? (float)(s[k] / w[k]) : 0.0f;
      }
    }
  }
}

template <int KC>  // the templates a thread holds sums for: K <= KC
__global__ __launch_bounds__(kThreads) void regress_normal_kernel(const float* __restrict__ x, size_t ld_x, const float* __restrict__ model,
                                                                  size_t ld_m, const unsigned char* __restrict__ flags, size_t ld_f, int T,
                                                                  const int* __restrict__ group, int G, const float* __restrict__ B,
                                                                  size_t ld_b, int K, double* __restrict__ N, double* __restrict__ r,
                                                                  unsigned* __restrict__ hits, int wide) {
  constexpr int NP = KC * (KC + 1) / 2;  // the upper triangle, row after row
  constexpr int NA = NP + KC;
  __shared__ double part[kWaves][NA];
  __shared__ unsigned hpart[kWaves];
  const size_t d = blockIdx.x;
  const int tid = threadIdx.x;
  const int gd = group ? group[d] : 0;
  if ((unsigned)gd >= (unsigned)G) {  // the whole workgroup: the row is in no group
    if (tid < K * K) N[d * K * K + tid] = 0.0;
    if (tid < K) r[d * K + tid] = 0.0;
    if (tid == 0 && hits) hits[d] = 0u;
    return;
  }
  const float* const xr = x + d * ld_x;
  const float* const mr = model ? model + d * ld_m : nullptr;
  const unsigned char* const fr = flags ? flags + d * ld_f : nullptr;
  const float* const Bg = B + (size_t)gd * K * ld_b;
  double acc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = 0.0;
  unsigned n = 0;
  for (int q = kOwn * tid; q < T; q += kTileSamples) {
    float xv[kOwn], mv[kOwn], bv[KC][kOwn];
    unsigned char fv[kOwn];
    load_own<kOwn>(xr, q, T, wide & kWideX, xv);
    if (mr) load_own<kOwn>(mr, q, T, wide & kWideM, mv);
    load_own_or_none<kOwn>(fr, q, T, wide & kWideF, fv);
#pragma unroll
    for (int i = 0; i < KC; ++i) {
      if (i < K) {
        load_own<kOwn>(Bg + (size_t)i * ld_b, q, T, wide & kWideB, bv[i]);
      } else {
#pragma unroll
        for (int k = 0; k < kOwn; ++k) bv[i][k] = 0.0f;
      }
    }
#pragma unroll
    for (int k = 0; k < kOwn; ++k) {
      const bool keep = fv[k] == 0;
      const double term = keep ? (mr ? (double)xv[k] - (double)mv[k] : (double)xv[k]) : 0.0;
      double b[KC];
#pragma unroll
      for (int i = 0; i < KC; ++i) b[i] = keep ? (double)bv[i][k] : 0.0;
      n += keep ? 1u : 0u;
      int a = 0;
#pragma unroll
      for (int i = 0; i < KC; ++i) {
#pragma unroll
        for (int j = i; j < KC; ++j, ++a) acc[a] = acc[a] + b[i] * b[j];
      }
#pragma unroll
      for (int i = 0; i < KC; ++i) acc[NP + i] = acc[NP + i] + b[i] * term;
    }
  }
  wave_sum_all(acc, n);
  const int wave = tid / kWave;
  if ((tid & (kWave - 1)) == 0) {
#pragma unroll
    for (int a = 0; a < NA; ++a) part[wave][a] = acc[a];
    hpart[wave] = n;
  }
  __syncthreads();
  auto total = [&](int a) { return ((part[0][a] + part[1][a]) + part[2][a]) + part[3][a]; };
  static_assert(kWaves == 4, "total() adds four waves");
  if (tid < KC * KC) {
    const int i = tid / KC, j = tid - i * KC;
    const int lo = min(i, j), hi = max(i, j);
    if (i < K && j < K) N[(d * K + i) * K + j] = total(lo * KC - lo * (lo - 1) / 2 + (hi - lo));
  } else if (tid < KC * KC + KC) {
    const int i = tid - KC * KC;
    if (i < K) r[d * K + i] = total(NP + i);
  } else if (tid == KC * KC + KC && hits) {
    hits[d] = hpart[0] + hpart[1] + hpart[2] + hpart[3];
  }
}

// x and y may be the same buffer: a thread reads its samples before it writes them, and no other thread touches them
__global__ __launch_bounds__(kThreads) void regress_apply_kernel(const float* x, size_t ld_x, int T, const int* __restrict__ group, int G,
                                                                 const float* __restrict__ B, size_t ld_b, int K,
                                                                 const double* __restrict__ a, int sign, float* y, size_t ld_y, int wide,
                                                                 int tiles_per_row, long long n_tiles) {
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / tiles_per_row;
    const int q = (int)(tile - row * tiles_per_row) * kTileSamples + kOwn * (int)threadIdx.x;
    if (q >= T) continue;
    const int gd = group ? group[row] : 0;
    float v[kOwn];
    load_own<kOwn>(x + (size_t)row * ld_x, q, T, wide & kWideX, v);
    if ((unsigned)gd < (unsigned)G) {
      const float* const Bg = B + (size_t)gd * K * ld_b;
      const double* const ar = a + (size_t)row * K;
      double s[kOwn];
#pragma unroll
      for (int k = 0; k < kOwn; ++k) s[k] = 0.0;
#pragma unroll
      for (int i = 0; i < kMaxTemplates; ++i) {
        if (i < K) {
          float bv[kOwn];
          load_own<kOwn>(Bg + (size_t)i * ld_b, q, T, wide & kWideB, bv);
          const double ai = ar[i];
#pragma unroll
          for (int k = 0; k < kOwn; ++k) s[k] = s[k] + ai * (double)bv[k];
        }
      }
#pragma unroll
      for (int k = 0; k < kOwn; ++k) {
        const float f = (float)s[k];
        v[k] = sign < 0 ? v[k] - f : v[k] + f;
      }
    }
    store_own<kOwn>(y + (size_t)row * ld_y, q, T, wide & kWideY, v);
  }
}

int wide_inputs(const float* x, size_t ld_x, const float* model, size_t ld_m, const uint8_t* flags, size_t ld_f) {
  return (mrx_aligned(x, ld_x * 4, 16) ? kWideX : 0) | (model && mrx_aligned(model, ld_m * 4, 16) ? kWideM : 0) |
         (flags && mrx_aligned(flags, ld_f, 4) ? kWideF : 0);
}

template <int KC>
void launch_normal(mrx_ctx* ctx, const float* x, size_t ld_x, const float* model, size_t ld_m, const uint8_t* flags, size_t ld_f, int D, int T,
                   const int32_t* group, int G, const float* B, size_t ld_b, int K, double* N, double* r, uint32_t* hits, int wide) {
  hipLaunchKernelGGL(regress_normal_kernel<KC>, dim3((unsigned)D), dim3(kThreads), 0, ctx->stream, x, ld_x, model, ld_m, flags, ld_f, T, group, G,
                     B, ld_b, K, N, r, hits, wide);
}

}  // namespace

extern "C" {

int mrx_tod_column_mean(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m, const uint8_t* d_flags, size_t ld_f,
                        int D, int T, const int32_t* d_group, int G, const double* d_u, const double* d_v, const double* d_off, double* d_S,
                        double* d_W, float* d_mean, size_t ld_c) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_u && d_v, "null pointer");
  MRX_REQUIRE(ctx, d_S || d_W || d_mean, "no output: d_S, d_W and d_mean are all null");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, G >= 1 && G <= kMaxGroups, "G must be in 1 .. 16");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && (!d_model || ld_m >= (size_t)T) && (!d_flags || ld_f >= (size_t)T) && (!d_mean || ld_c >= (size_t)T),
              "ld_x, ld_m, ld_f or ld_c smaller than T");
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, G, T, kTileSamples);  // items: (group, tile)
  hipLaunchKernelGGL(column_mean_kernel, dim3(g.blocks), dim3(kThreads), 0, ctx->stream, d_x, ld_x, d_model, ld_m, d_flags, ld_f, D, T, d_group, d_u,
                     d_v, d_off, d_S, d_W, d_mean, ld_c, wide_inputs(d_x, ld_x, d_model, ld_m, d_flags, ld_f), g.tiles_per_row, g.n_tiles);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_regress_normal(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m, const uint8_t* d_flags, size_t ld_f,
                           int D, int T, const int32_t* d_group, int G, const float* d_B, size_t ld_b, int K, double* d_N, double* d_r,
                           uint32_t* d_hits) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_B && d_N && d_r, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, G >= 1 && G <= kMaxGroups, "G must be in 1 .. 16");
  MRX_REQUIRE(ctx, K >= 1 && K <= kMaxTemplates, "K must be in 1 .. 8");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && (!d_model || ld_m >= (size_t)T) && (!d_flags || ld_f >= (size_t)T) && ld_b >= (size_t)T,
              "ld_x, ld_m, ld_f or ld_b smaller than T");
  const int wide = wide_inputs(d_x, ld_x, d_model, ld_m, d_flags, ld_f) | (mrx_aligned(d_B, ld_b * 4, 16) ? kWideB : 0);
  if (K <= 2)
    launch_normal<2>(ctx, d_x, ld_x, d_model, ld_m, d_flags, ld_f, D, T, d_group, G, d_B, ld_b, K, d_N, d_r, d_hits, wide);
  else if (K <= 4)
    launch_normal<4>(ctx, d_x, ld_x, d_model, ld_m, d_flags, ld_f, D, T, d_group, G, d_B, ld_b, K, d_N, d_r, d_hits, wide);
  else
    launch_normal<8>(ctx, d_x, ld_x, d_model, ld_m, d_flags, ld_f, D, T, d_group, G, d_B, ld_b, K, d_N, d_r, d_hits, wide);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_regress_apply(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const int32_t* d_group, int G, const float* d_B,
                          size_t ld_b, int K, const double* d_a, int sign, float* d_y, size_t ld_y) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_B && d_a && d_y, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, G >= 1 && G <= kMaxGroups, "G must be in 1 .. 16");
  MRX_REQUIRE(ctx, K >= 1 && K <= kMaxTemplates, "K must be in 1 .. 8");
  MRX_REQUIRE(ctx, sign == 1 || sign == -1, "sign must be -1 or +1");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && ld_y >= (size_t)T && ld_b >= (size_t)T, "ld_x, ld_y or ld_b smaller than T");
  MRX_REQUIRE(ctx, d_y != d_x || ld_y == ld_x, "in place (d_y == d_x) needs ld_y == ld_x");
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, D, T, kTileSamples);
  const int wide = (mrx_aligned(d_x, ld_x * 4, 16) ? kWideX : 0) | (mrx_aligned(d_B, ld_b * 4, 16) ? kWideB : 0) |
                   (mrx_aligned(d_y, ld_y * 4, 16) ? kWideY : 0);
  hipLaunchKernelGGL(regress_apply_kernel, dim3(g.blocks), dim3(kThreads), 0, ctx->stream, d_x, ld_x, T, d_group, G, d_B, ld_b, K, d_a, sign, d_y,
                     ld_y, wide, g.tiles_per_row, g.n_tiles);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // extern "C"
