// Narrow spectral lines of a [D, T] TOD: an amplitude and a phase per (row, segment) at a frequency of the row's own, the
// carriers evaluated in the kernels (maria_amd/lines.py).  Segment s of d_bound [S + 1] is [lo, hi), both
// clamped to 0 .. T, n = hi - lo; the basis of row d has K = n_poly + 2 L functions (n_poly 0 .. 2, L 1 .. 3):
//   u(t)        = n > 1 ? (double)(2 (t - lo) - (n - 1)) / (double)(n - 1) : 0.0       (mrx_subscan.hip's, the same bits)
//   B_0 = 1.0, B_1 = u                                                                  (the first n_poly of them)
//   theta       = nu[d][l] * (double)t,  t counted from the START OF THE ROW;  q = theta - rint(theta)   (exact)
//   B_{n_poly + 2 l} = cospi(2.0 * q),  B_{n_poly + 2 l + 1} = sinpi(2.0 * q)
//   term(d, t)  = (double)x[d][t] - (double)model[d][t]                      (plain (double)x without a model)
//   N[d][s][i][j] = sum over the segment's t with flags[d][t] == 0 of B_i * B_j,   r[d][s][i] = of B_i * term(d, t)
//   y[d][t]     = x[d][t] + sign * (float)(sum over i = n_poly .. K - 1, in order, of a[d][s][i] * B_i)
// The file is built without FMA contraction: every operation above is one float64 rounding (cospi and sinpi are the
// device library's).  theta is ONE rounding of an exact product, so the phase of sample t does not depend on the segment
// it falls in; its reduction q is exact (|theta - rint(theta)| <= 1/2 is a float64 on theta's own grid), and 2 q is exact.
//
// mrx_tod_line_normal.  mrx_tod_segment_normal's shape: one wave takes one (row, segment) and owns all of its sums; lane o
// adds the samples lo + o, lo + o + 64, .. in ascending order into K (K + 1) / 2 + K float64 accumulators in registers,
// then the 64 lanes meet and store (mrx_tod_dev.h: rhs_add, wave_sum_all, store_normal_by_lane).  The order is a function of lo and hi alone.  A flagged sample enters as a row of zeros (selected, never
// multiplied).  The four waves of a workgroup take four consecutive (row, segment) pairs and share nothing.  Compiled
// for every (n_poly, L).
//
// mrx_tod_line_apply.  mrx_tod_segment_apply's streaming pass over (row, tile), a thread its own four samples, the
// segment of a sample by find_segment (mrx_tod_dev.h).
#include "mrx_internal.h"
#include "mrx_tod_dev.h"

#include <algorithm>

namespace {

using namespace mrx_tod;  // the 256-thread, four-sample tile, kWave

constexpr int kMaxLines = 3;
constexpr int kMaxPoly = 2;
constexpr int kFlight = 2;  // samples of a lane whose loads go out together

enum : int { kWideX = 1, kWideY = 2 };

// the two carriers of a line of nu cycles a sample at sample t of the row
__device__ __forceinline__ void carrier(double nu, int t, double& c, double& s) {
  const double theta = nu * (double)t;
  const double q = theta - rint(theta);
  c = cospi(2.0 * q);
  s = sinpi(2.0 * q);
}

template <int NPOLY, int NL>
__global__ __launch_bounds__(kThreads) void line_normal_kernel(const float* __restrict__ x, size_t ld_x, const float* __restrict__ model, size_t ld_m,
                                                               const unsigned char* __restrict__ flags, size_t ld_f, int T,
                                                               const int* __restrict__ bound, int S, const double* __restrict__ nu,
                                                               double* __restrict__ N, double* __restrict__ r, unsigned* __restrict__ hits,
                                                               long long n_items) {
  constexpr int K = NPOLY + 2 * NL;
  constexpr int NP = K * (K + 1) / 2;  // the upper triangle, row after row
  constexpr int NA = NP + K;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  for (long long item = (long long)blockIdx.x * kWaves + wave; item < n_items; item += (long long)gridDim.x * kWaves) {
    const long long d = item / S;
    const int s = (int)(item - d * S);
    const int lo = clamp_bound(bound[s], T), hi = clamp_bound(bound[s + 1], T);
    const int n = hi - lo;  // <= 0: empty, the loop below does not run
    const double span = (double)(n - 1);
    const float* const xr = x + (size_t)d * ld_x;
    const float* const mr = model ? model + (size_t)d * ld_m : nullptr;
    const unsigned char* const fr = flags ? flags + (size_t)d * ld_f : nullptr;
    double f[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) f[l] = nu[(size_t)d * NL + l];
    double acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0.0;
    unsigned cnt = 0;
    for (int k0 = lane; k0 < n; k0 += kFlight * kWave) {
      float xv[kFlight], mv[kFlight];
      unsigned char fv[kFlight];
#pragma unroll
      for (int e = 0; e < kFlight; ++e) {
        const int k = k0 + e * kWave;
        const bool in = k < n;
        xv[e] = in ? xr[lo + k] : 0.0f;
        mv[e] = in && mr ? mr[lo + k] : 0.0f;
        fv[e] = in ? (fr ? fr[lo + k] : (unsigned char)0) : (unsigned char)1;
      }
#pragma unroll
      for (int e = 0; e < kFlight; ++e) {
        const int k = k0 + e * kWave;
        const bool keep = fv[e] == 0;
        double B[K], b[K];
        if (NPOLY > 0) B[0] = 1.0;
        if (NPOLY > 1) B[1] = n > 1 ? (2.0 * (double)k - span) / span : 0.0;
#pragma unroll
        for (int l = 0; l < NL; ++l) carrier(f[l], lo + k, B[NPOLY + 2 * l], B[NPOLY + 2 * l + 1]);
#pragma unroll
        for (int i = 0; i < K; ++i) b[i] = keep ? B[i] : 0.0;
        const double term = keep ? (mr ? (double)xv[e] - (double)mv[e] : (double)xv[e]) : 0.0;
        cnt += keep ? 1u : 0u;
        // (written out, on a row selected here: mrx_tod_dev.h says why)
        int a = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
#pragma unroll
          for (int j = i; j < K; ++j, ++a) acc[a] = acc[a] + b[i] * b[j];
        }
        rhs_add<K>(acc + NP, B, keep, term);
      }
    }
    wave_sum_all(acc, cnt);
    store_normal_by_lane<K>(acc, lane, N + (size_t)item * (K * K), r + (size_t)item * K);
    if (lane == 0 && hits) hits[item] = cnt;
  }
}

// x and y may be the same buffer: a thread reads its samples before it writes them, and no other thread touches them
template <int NL>
__global__ __launch_bounds__(kThreads) void line_apply_kernel(const float* x, size_t ld_x, int T, const int* __restrict__ bound, int S,
                                                              const double* __restrict__ nu, int n_poly, const double* __restrict__ a, int sign,
                                                              float* y, size_t ld_y, int wide, int tiles_per_row, long long n_tiles) {
  const int K = n_poly + 2 * NL;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / tiles_per_row;
    const int q = (int)(tile - row * tiles_per_row) * kTileSamples + kOwn * (int)threadIdx.x;
    if (q >= T) continue;
    float v[kOwn];
    load_own<kOwn>(x + (size_t)row * ld_x, q, T, wide & kWideX, v);
    double f[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) f[l] = nu[(size_t)row * NL + l];
    int s = -1, lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < kOwn; ++k) {
      const int t = q + k;
      if (t >= T) break;
      if (!(t >= lo && t < hi)) s = find_segment(bound, S, T, t, lo, hi);
      if (s < 0) continue;  // in no segment: copied
      const double* const as = a + ((size_t)row * S + s) * K + n_poly;
      double sum = 0.0;
#pragma unroll
      for (int l = 0; l < NL; ++l) {
        double c, sn;
        carrier(f[l], t, c, sn);
        sum = sum + as[2 * l] * c;
        sum = sum + as[2 * l + 1] * sn;
      }
      const float g = (float)sum;
      v[k] = sign < 0 ? v[k] - g : v[k] + g;
    }
    store_own<kOwn>(y + (size_t)row * ld_y, q, T, wide & kWideY, v);
  }
}

template <int NPOLY, int NL>
void launch_normal(mrx_ctx* ctx, const float* x, size_t ld_x, const float* model, size_t ld_m, const uint8_t* flags, size_t ld_f, int T,
                   const int32_t* bound, int S, const double* nu, double* N, double* r, uint32_t* hits, long long n_items) {
  hipLaunchKernelGGL((line_normal_kernel<NPOLY, NL>), dim3(mrx_resident_blocks(ctx, (n_items + kWaves - 1) / kWaves)), dim3(kThreads), 0, ctx->stream,
                     x, ld_x, model, ld_m, flags, ld_f, T, bound, S, nu, N, r, hits, n_items);
}

template <int NL>
void launch_apply(mrx_ctx* ctx, const float* x, size_t ld_x, int T, const int32_t* bound, int S, const double* nu, int n_poly, const double* a,
                  int sign, float* y, size_t ld_y, int wide, const mrx_tile_grid_t& g) {
  hipLaunchKernelGGL(line_apply_kernel<NL>, dim3(g.blocks), dim3(kThreads), 0, ctx->stream, x, ld_x, T, bound, S, nu, n_poly, a, sign, y, ld_y, wide,
                     g.tiles_per_row, g.n_tiles);
}

}  // namespace

extern "C" {

int mrx_tod_line_normal(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m, const uint8_t* d_flags, size_t ld_f, int D,
                        int T, const int32_t* d_bound, int S, const double* d_nu, int L, int n_poly, double* d_N, double* d_r, uint32_t* d_hits) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_bound && d_nu && d_N && d_r, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, S >= 1, "need S >= 1 segments");
  MRX_REQUIRE(ctx, L >= 1 && L <= kMaxLines, "L must be in 1 .. 3");
  MRX_REQUIRE(ctx, n_poly >= 0 && n_poly <= kMaxPoly, "n_poly must be in 0 .. 2");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && (!d_model || ld_m >= (size_t)T) && (!d_flags || ld_f >= (size_t)T), "ld_x, ld_m or ld_f smaller than T");
  const long long n_items = (long long)D * S;
#define MRX_LINE_NORMAL(p, l) \
  case 3 * p + (l - 1):       \
    launch_normal<p, l>(ctx, d_x, ld_x, d_model, ld_m, d_flags, ld_f, T, d_bound, S, d_nu, d_N, d_r, d_hits, n_items); \
    break
  switch (3 * n_poly + (L - 1)) {
    MRX_LINE_NORMAL(0, 1);
    MRX_LINE_NORMAL(0, 2);
    MRX_LINE_NORMAL(0, 3);
    MRX_LINE_NORMAL(1, 1);
    MRX_LINE_NORMAL(1, 2);
    MRX_LINE_NORMAL(1, 3);
    MRX_LINE_NORMAL(2, 1);
    MRX_LINE_NORMAL(2, 2);
    default:
      MRX_LINE_NORMAL(2, 3);
  }
#undef MRX_LINE_NORMAL
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_line_apply(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const int32_t* d_bound, int S, const double* d_nu, int L,
                       int n_poly, const double* d_a, int sign, float* d_y, size_t ld_y) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_bound && d_nu && d_a && d_y, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, S >= 1, "need S >= 1 segments");
  MRX_REQUIRE(ctx, L >= 1 && L <= kMaxLines, "L must be in 1 .. 3");
  MRX_REQUIRE(ctx, n_poly >= 0 && n_poly <= kMaxPoly, "n_poly must be in 0 .. 2");
  MRX_REQUIRE(ctx, sign == 1 || sign == -1, "sign must be -1 or +1");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && ld_y >= (size_t)T, "ld_x or ld_y smaller than T");
  MRX_REQUIRE(ctx, d_y != d_x || ld_y == ld_x, "in place (d_y == d_x) needs ld_y == ld_x");
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, D, T, kTileSamples);
  const int wide = (mrx_aligned(d_x, ld_x * 4, 16) ? kWideX : 0) | (mrx_aligned(d_y, ld_y * 4, 16) ? kWideY : 0);
  switch (L) {
    case 1:
      launch_apply<1>(ctx, d_x, ld_x, T, d_bound, S, d_nu, n_poly, d_a, sign, d_y, ld_y, wide, g);
      break;
    case 2:
      launch_apply<2>(ctx, d_x, ld_x, T, d_bound, S, d_nu, n_poly, d_a, sign, d_y, ld_y, wide, g);
      break;
    default:
      launch_apply<3>(ctx, d_x, ld_x, T, d_bound, S, d_nu, n_poly, d_a, sign, d_y, ld_y, wide, g);
  }
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // extern "C"
