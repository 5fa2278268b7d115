// The subscan polynomial filter of a [D, T] TOD: a Legendre fit per (row, segment), the basis evaluated in the kernels
// (maria_amd/subscans.py).  Segment s of d_bound [S + 1] is [lo, hi), both clamped to 0 .. T, L = hi - lo:
//   u(t)        = L > 1 ? (double)(2 (t - lo) - (L - 1)) / (double)(L - 1) : 0.0
//   P_0 = 1, P_1 = u, P_{n+1} = ((((double)(2 n + 1) * u) * P_n) - ((double)n * P_{n-1})) * c_n,  c_n = 1.0 / (double)(n + 1)
//   term(d, t)  = (double)x[d][t] - (double)model[d][t]                      (plain (double)x without a model)
//   N[d][s][i][j] = sum over the segment's t with flags[d][t] == 0 of P_i * P_j,   r[d][s][i] = of P_i * term(d, t)
//   y[d][t]     = x[d][t] + sign * (float)(sum over i, in order, of a[d][s][i] * P_i)
// The file is built without FMA contraction: every operation above is one float64 rounding.  The numerator of u is formed
// in float64 from the int32 offset: every value involved is an integer below 2^32, so it is the integer numerator exactly.
//
// mrx_tod_segment_normal.  One wave takes one (row, segment) and owns all of its sums: lane o adds the samples lo + o,
// lo + o + 64, .. in ascending order into K (K + 1) / 2 + K float64 accumulators in registers, then the 64 lanes meet and
// store (mrx_tod_dev.h: rhs_add, wave_sum_all, store_normal_by_lane).  The order is a function of L alone.  A flagged
// sample enters as a row of zeros (selected, never multiplied by x).  The four waves of a workgroup take four consecutive
// (row, segment) pairs and share nothing: no LDS, no barrier.  The kernel is compiled for every K = 1 .. 8.
//
// mrx_tod_segment_apply.  A streaming pass over (row, tile), a thread its own four samples (mrx_tod_dev.h).  A thread
// finds its sample's segment by find_segment and keeps it while the following samples stay inside.
//
// mrx_tod_segment_project.  The filter with its flags fixed, F = I - T A T^t M or its transpose, in place: the sums of the
// first entry, a K x K product with the caller's frozen A = N^-1, and the subtraction of the second, one wave a (row,
// segment) for all three.  Its comment is above its kernel.
#include "mrx_internal.h"
#include "mrx_tod_dev.h"

#include <algorithm>

namespace {

using namespace mrx_tod;  // the 256-thread, four-sample tile, kWave

constexpr int kMaxOrder = 8;  // K: the polynomials P_0 .. P_{K - 1}
constexpr int kFlight = 2;    // samples of a lane whose loads go out together

enum : int { kWideX = 1, kWideY = 2 };

// P_0 .. P_{K - 1} at u; the loop unrolls, so that c_n is a constant rounded once
template <int K>
__device__ __forceinline__ void legendre(double u, double (&P)[K]) {
  P[0] = 1.0;
  if (K > 1) P[1] = u;
#pragma unroll
  for (int n = 1; n + 1 < K; ++n) P[n + 1] = ((((double)(2 * n + 1) * u) * P[n]) - ((double)n * P[n - 1])) * (1.0 / (double)(n + 1));
}

template <int K>
__global__ __launch_bounds__(kThreads) void segment_normal_kernel(const float* __restrict__ x, size_t ld_x, const float* __restrict__ model,
                                                                  size_t ld_m, const unsigned char* __restrict__ flags, size_t ld_f, int T,
                                                                  const int* __restrict__ bound, int S, double* __restrict__ N,
                                                                  double* __restrict__ r, unsigned* __restrict__ hits, long long n_items) {
  constexpr int NP = K * (K + 1) / 2;  // the upper triangle, row after row
  constexpr int NA = NP + K;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  for (long long item = (long long)blockIdx.x * kWaves + wave; item < n_items; item += (long long)gridDim.x * kWaves) {
    const long long d = item / S;
    const int s = (int)(item - d * S);
    const int lo = clamp_bound(bound[s], T), hi = clamp_bound(bound[s + 1], T);
    const int L = hi - lo;  // <= 0: empty, the loop below does not run
    const double span = (double)(L - 1);
    const float* const xr = x + (size_t)d * ld_x;
    const float* const mr = model ? model + (size_t)d * ld_m : nullptr;
    const unsigned char* const fr = flags ? flags + (size_t)d * ld_f : nullptr;
    double acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0.0;
    unsigned n = 0;
    for (int k0 = lane; k0 < L; k0 += kFlight * kWave) {
      float xv[kFlight], mv[kFlight];
      unsigned char fv[kFlight];
#pragma unroll
      for (int e = 0; e < kFlight; ++e) {
        const int k = k0 + e * kWave;
        const bool in = k < L;
        xv[e] = in ? xr[lo + k] : 0.0f;
        mv[e] = in && mr ? mr[lo + k] : 0.0f;
        fv[e] = in ? (fr ? fr[lo + k] : (unsigned char)0) : (unsigned char)1;
      }
#pragma unroll
      for (int e = 0; e < kFlight; ++e) {
        const int k = k0 + e * kWave;
        const bool keep = fv[e] == 0;
        const double u = L > 1 ? (2.0 * (double)k - span) / span : 0.0;
        double P[K], b[K];
        legendre<K>(u, P);
#pragma unroll
        for (int i = 0; i < K; ++i) b[i] = keep ? P[i] : 0.0;
        const double term = keep ? (mr ? (double)xv[e] - (double)mv[e] : (double)xv[e]) : 0.0;
        n += keep ? 1u : 0u;
        // (written out, on a row selected here: mrx_tod_dev.h says why)
        int a = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
#pragma unroll
          for (int j = i; j < K; ++j, ++a) acc[a] = acc[a] + b[i] * b[j];
        }
        rhs_add<K>(acc + NP, P, keep, term);
      }
    }
    wave_sum_all(acc, n);
    store_normal_by_lane<K>(acc, lane, N + (size_t)item * (K * K), r + (size_t)item * K);
    if (lane == 0 && hits) hits[item] = n;
  }
}

// x and y may be the same buffer: a thread reads its samples before it writes them, and no other thread touches them
__global__ __launch_bounds__(kThreads) void segment_apply_kernel(const float* x, size_t ld_x, int T, const int* __restrict__ bound, int S, int K,
                                                                 const double* __restrict__ a, int sign, float* y, size_t ld_y, int wide,
                                                                 int tiles_per_row, long long n_tiles) {
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / tiles_per_row;
    const int q = (int)(tile - row * tiles_per_row) * kTileSamples + kOwn * (int)threadIdx.x;
    if (q >= T) continue;
    float v[kOwn];
    load_own<kOwn>(x + (size_t)row * ld_x, q, T, wide & kWideX, v);
    int s = -1, lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < kOwn; ++k) {
      const int t = q + k;
      if (t >= T) break;
      if (!(t >= lo && t < hi)) s = find_segment(bound, S, T, t, lo, hi);
      if (s < 0) continue;  // in no segment: copied
      const int L = hi - lo;
      const double span = (double)(L - 1);
      const double u = L > 1 ? (2.0 * (double)(t - lo) - span) / span : 0.0;
      const double* const as = a + ((size_t)row * S + s) * K;
      double pm = 0.0, p = 1.0, sum = 0.0;  // P_{i - 1}, P_i
#pragma unroll
      for (int i = 0; i < kMaxOrder; ++i) {
        if (i < K) {
          sum = sum + as[i] * p;
          const double next = i == 0 ? u : ((((double)(2 * i + 1) * u) * p) - ((double)i * pm)) * (1.0 / (double)(i + 1));
          pm = p, p = next;
        }
      }
      const float f = (float)sum;
      v[k] = sign < 0 ? v[k] - f : v[k] + f;
    }
    store_own<kOwn>(y + (size_t)row * ld_y, q, T, wide & kWideY, v);
  }
}

// The frozen projector of a (row, segment), in place: r = sum P x (pass 1), a = A r, x -= (float)(sum a_i P_i) (pass 2).
// Pass 1 is segment_normal_kernel's r, operation for operation (its kFlight loop, its selects, the same rhs_add and
// wave_sum_all), over the unflagged samples (forward) or over all of them (transposed); pass 2 is segment_apply_kernel's expression on every
// sample (forward) or on the unflagged ones (transposed), each lane on the samples it read in pass 1: lo + lane,
// lo + lane + 64, ..  Pass 2 reads its samples from global memory a second time: a segment is a few KiB that one wave
// has just streamed, and nobody else writes it.  A pair that is not ok, or is empty, touches no sample.
template <int K>
__global__ __launch_bounds__(kThreads) void segment_project_kernel(float* x, size_t ld_x, const unsigned char* __restrict__ flags, size_t ld_f, int T,
                                                                   const int* __restrict__ bound, int S, const double* __restrict__ A,
                                                                   const unsigned char* __restrict__ ok, int transpose, double* __restrict__ a_out,
                                                                   long long n_items) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  for (long long item = (long long)blockIdx.x * kWaves + wave; item < n_items; item += (long long)gridDim.x * kWaves) {
    const long long d = item / S;
    const int s = (int)(item - d * S);
    const int lo = clamp_bound(bound[s], T), hi = clamp_bound(bound[s + 1], T);
    const int L = hi - lo;
    if (L <= 0 || ok[item] == 0) {  // the same for the whole wave
      if (a_out && lane < K) a_out[(size_t)item * K + lane] = 0.0;
      continue;
    }
    const double span = (double)(L - 1);
    float* const xr = x + (size_t)d * ld_x;
    const unsigned char* const fr = flags ? flags + (size_t)d * ld_f : nullptr;
    const unsigned char* const f1 = transpose ? nullptr : fr;  // the mask of pass 1
    const unsigned char* const f2 = transpose ? fr : nullptr;  // the mask of pass 2
    double acc[K];
#pragma unroll
    for (int i = 0; i < K; ++i) acc[i] = 0.0;
    for (int k0 = lane; k0 < L; k0 += kFlight * kWave) {
      float xv[kFlight];
      unsigned char fv[kFlight];
#pragma unroll
      for (int e = 0; e < kFlight; ++e) {
        const int k = k0 + e * kWave;
        const bool in = k < L;
        xv[e] = in ? xr[lo + k] : 0.0f;
        fv[e] = in ? (f1 ? f1[lo + k] : (unsigned char)0) : (unsigned char)1;
      }
#pragma unroll
      for (int e = 0; e < kFlight; ++e) {
        const int k = k0 + e * kWave;
        const bool keep = fv[e] == 0;
        const double u = L > 1 ? (2.0 * (double)k - span) / span : 0.0;
        double P[K];
        legendre<K>(u, P);
        const double term = keep ? (double)xv[e] : 0.0;
        rhs_add<K>(acc, P, keep, term);
      }
    }
    wave_sum_all(acc);
    // every lane holds every r_i and forms every a_i: the same bits in all of them
    const double* const As = A + (size_t)item * (K * K);
    double a[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      double sum = 0.0;
#pragma unroll
      for (int j = 0; j < K; ++j) sum = sum + As[i * K + j] * acc[j];
      a[i] = sum;
    }
    if (a_out) {
      int me = lane;
      asm volatile("" : "+v"(me));
      double va = 0.0;
#pragma unroll
      for (int i = 0; i < K; ++i) va = me == i ? a[i] : va;
      if (lane < K) a_out[(size_t)item * K + lane] = va;
    }
    for (int k0 = lane; k0 < L; k0 += kFlight * kWave) {
      float xv[kFlight];
      bool on[kFlight];
#pragma unroll
      for (int e = 0; e < kFlight; ++e) {
        const int k = k0 + e * kWave;
        on[e] = k < L && (f2 ? f2[lo + k] == 0 : true);
        xv[e] = on[e] ? xr[lo + k] : 0.0f;
      }
#pragma unroll
      for (int e = 0; e < kFlight; ++e) {
        const int k = k0 + e * kWave;
        const double u = L > 1 ? (2.0 * (double)k - span) / span : 0.0;
        double P[K];
        legendre<K>(u, P);
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < K; ++i) sum = sum + a[i] * P[i];
        if (on[e]) xr[lo + k] = xv[e] - (float)sum;
      }
    }
  }
}

template <int K>
void launch_project(mrx_ctx* ctx, float* x, size_t ld_x, const uint8_t* flags, size_t ld_f, int T, const int32_t* bound, int S, const double* A,
                    const uint8_t* ok, int transpose, double* a, long long n_items) {
  hipLaunchKernelGGL(segment_project_kernel<K>, dim3(mrx_resident_blocks(ctx, (n_items + kWaves - 1) / kWaves)), dim3(kThreads), 0, ctx->stream, x, ld_x,
                     flags, ld_f, T, bound, S, A, ok, transpose, a, n_items);
}

template <int K>
void launch_normal(mrx_ctx* ctx, const float* x, size_t ld_x, const float* model, size_t ld_m, const uint8_t* flags, size_t ld_f, int T,
                   const int32_t* bound, int S, double* N, double* r, uint32_t* hits, long long n_items) {
  hipLaunchKernelGGL(segment_normal_kernel<K>, dim3(mrx_resident_blocks(ctx, (n_items + kWaves - 1) / kWaves)), dim3(kThreads), 0, ctx->stream, x, ld_x,
                     model, ld_m, flags, ld_f, T, bound, S, N, r, hits, n_items);
}

}  // namespace

extern "C" {

int mrx_tod_segment_normal(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m, const uint8_t* d_flags, size_t ld_f,
                           int D, int T, const int32_t* d_bound, int S, int K, double* d_N, double* d_r, uint32_t* d_hits) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_bound && d_N && d_r, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, S >= 1, "need S >= 1 segments");
  MRX_REQUIRE(ctx, K >= 1 && K <= kMaxOrder, "K must be in 1 .. 8");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && (!d_model || ld_m >= (size_t)T) && (!d_flags || ld_f >= (size_t)T), "ld_x, ld_m or ld_f smaller than T");
  const long long n_items = (long long)D * S;
#define MRX_SEGMENT_NORMAL(k) \
  case k:                     \
    launch_normal<k>(ctx, d_x, ld_x, d_model, ld_m, d_flags, ld_f, T, d_bound, S, d_N, d_r, d_hits, n_items); \
    break
  switch (K) {
    MRX_SEGMENT_NORMAL(1);
    MRX_SEGMENT_NORMAL(2);
    MRX_SEGMENT_NORMAL(3);
    MRX_SEGMENT_NORMAL(4);
    MRX_SEGMENT_NORMAL(5);
    MRX_SEGMENT_NORMAL(6);
    MRX_SEGMENT_NORMAL(7);
    default:
      MRX_SEGMENT_NORMAL(8);
  }
#undef MRX_SEGMENT_NORMAL
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_segment_apply(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const int32_t* d_bound, int S, int K, const double* d_a,
                          int sign, float* d_y, size_t ld_y) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_bound && d_a && d_y, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, S >= 1, "need S >= 1 segments");
  MRX_REQUIRE(ctx, K >= 1 && K <= kMaxOrder, "K must be in 1 .. 8");
  MRX_REQUIRE(ctx, sign == 1 || sign == -1, "sign must be -1 or +1");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && ld_y >= (size_t)T, "ld_x or ld_y smaller than T");
  MRX_REQUIRE(ctx, d_y != d_x || ld_y == ld_x, "in place (d_y == d_x) needs ld_y == ld_x");
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, D, T, kTileSamples);
  const int wide = (mrx_aligned(d_x, ld_x * 4, 16) ? kWideX : 0) | (mrx_aligned(d_y, ld_y * 4, 16) ? kWideY : 0);
  hipLaunchKernelGGL(segment_apply_kernel, dim3(g.blocks), dim3(kThreads), 0, ctx->stream, d_x, ld_x, T, d_bound, S, K, d_a, sign, d_y, ld_y, wide,
                     g.tiles_per_row, g.n_tiles);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_segment_project(mrx_ctx* ctx, float* d_x, size_t ld_x, const uint8_t* d_flags, size_t ld_f, int D, int T, const int32_t* d_bound, int S,
                            int K, const double* d_A, const uint8_t* d_ok, int transpose, double* d_a) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_bound && d_A && d_ok, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, S >= 1, "need S >= 1 segments");
  MRX_REQUIRE(ctx, K >= 1 && K <= kMaxOrder, "K must be in 1 .. 8");
  MRX_REQUIRE(ctx, transpose == 0 || transpose == 1, "transpose must be 0 or 1");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && (!d_flags || ld_f >= (size_t)T), "ld_x or ld_f smaller than T");
  const long long n_items = (long long)D * S;
#define MRX_SEGMENT_PROJECT(k) \
  case k:                      \
    launch_project<k>(ctx, d_x, ld_x, d_flags, ld_f, T, d_bound, S, d_A, d_ok, transpose, d_a, n_items); \
    break
  switch (K) {
    MRX_SEGMENT_PROJECT(1);
    MRX_SEGMENT_PROJECT(2);
    MRX_SEGMENT_PROJECT(3);
    MRX_SEGMENT_PROJECT(4);
    MRX_SEGMENT_PROJECT(5);
    MRX_SEGMENT_PROJECT(6);
    MRX_SEGMENT_PROJECT(7);
    default:
      MRX_SEGMENT_PROJECT(8);
  }
#undef MRX_SEGMENT_PROJECT
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // extern "C"
