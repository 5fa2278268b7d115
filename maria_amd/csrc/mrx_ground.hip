// Templates synchronous with a per-sample key, and their removal, on a [D, T] TOD (maria_amd/ground.py):
//   kept(d, k)     = { t in bin k : 0 <= t < T, flags[d][t] == 0 }
//   hits[d][k]     = |kept(d, k)|
//   sum[d][k]      = sum over kept(d, k) of ((double)x[d][t] - (double)model[d][t])
//   template[d][k] = hits >= max(min_hits, 1) ? (float)(sum / hits) : 0
//   y[d][t]        = x[d][t] + sign * template[d][bin[t]]                       (bin[t] outside 0 .. K - 1: y = x)
// The key is the boresight azimuth's bin for ground pickup; the kernels know only bin lists and bin indices.
//
// Reduction.  One wave takes one (row, bin); the four waves of a workgroup take four neighbouring bins of one row, so
// that the short runs of consecutive samples neighbouring bins own meet in the same cache lines.  Lane l adds the list
// entries l, l + 64, .. of its bin, in that order, into a float64 accumulator of its own; the 64 accumulators meet in
// wave_sum_all (mrx_tod_dev.h).  The order of every addition is a function of the bin's list alone: the
// result is the same on every call and does not depend on the other rows of the launch.  No atomics.
// A list entry outside [0, T) is skipped by an unsigned comparison before any address is formed from it, and the list
// bounds read from d_start are clamped into [0, n_order]: bad lists give wrong sums, never a read outside the arrays.
// The gather moves 4 bytes a lane (+ 4 of the list, which stays in L2): bound by the number of loads in flight, not by
// HBM (DESIGN 3.21 has the times).
//
// Application.  A workgroup takes kTileSamples consecutive samples of a row, a thread four consecutive ones: 16-byte
// loads of x and of the bins and a 16-byte store of y where the pointers and pitches allow, single words otherwise.  The
// template row (<= 16 KB) is read through the cache; the bin varies slowly along a scan.  A bin outside [0, K) is found
// by an unsigned comparison and no template entry is read for it.
#include "mrx_internal.h"
#include "mrx_tod_dev.h"

#include <algorithm>

namespace {

using namespace mrx_tod;  // the 256-thread, four-sample tile, kWave; kWaves neighbouring bins of one row a workgroup reduces

constexpr int kUnroll = 4;      // list entries a lane has in flight
constexpr int kMaxBins = 4096;  // maria_amd.ground.MAX_BINS

__global__ __launch_bounds__(kThreads) void bin_reduce_kernel(const float* __restrict__ x, size_t ld_x, const float* __restrict__ model,
                                                              size_t ld_m, const unsigned char* __restrict__ flags, size_t ld_f, int T,
                                                              const int* __restrict__ order, int n_order, const int* __restrict__ start,
                                                              int K, unsigned min_hits, double* __restrict__ sum, unsigned* __restrict__ hits,
                                                              float* __restrict__ tmpl, int groups_per_row, long long n_groups) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  for (long long group = blockIdx.x; group < n_groups; group += gridDim.x) {
    const long long row = group / groups_per_row;
    const int k = (int)(group - row * groups_per_row) * kWaves + wave;
    if (k >= K) continue;  // the whole wave: nothing below synchronises the workgroup
    const int lo = min(max(start[k], 0), n_order);
    const int hi = min(max(start[k + 1], lo), n_order);
    const float* const xr = x + (size_t)row * ld_x;
    const float* const mr = model ? model + (size_t)row * ld_m : nullptr;
    const unsigned char* const fr = flags ? flags + (size_t)row * ld_f : nullptr;
    double acc = 0.0;
    unsigned n = 0;
    for (int i0 = lo + lane; i0 < hi; i0 += kWave * kUnroll) {
      int t[kUnroll];
      bool keep[kUnroll];
      float v[kUnroll], m[kUnroll];
      unsigned char f[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int i = i0 + u * kWave;
        t[u] = i < hi ? order[i] : -1;
        keep[u] = (unsigned)t[u] < (unsigned)T;
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {  // the three loads of a sample wait for its index only, not for each other
        const int s = keep[u] ? t[u] : 0;  // sample 0 exists: the loads do not branch
        f[u] = fr ? fr[s] : (unsigned char)0;
        v[u] = xr[s];
        m[u] = mr ? mr[s] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (keep[u] && f[u] == 0) {
          acc += mr ? (double)v[u] - (double)m[u] : (double)v[u];
          ++n;
        }
      }
    }
    wave_sum_all(acc, n);
    if (lane == 0) {
      const size_t o = (size_t)row * K + k;
      if (sum) sum[o] = acc;
      if (hits) hits[o] = n;
      if (tmpl) tmpl[o] = n >= min_hits ? (float)(acc / (double)n) : 0.0f;
    }
  }
}

__device__ __forceinline__ float shifted(float v, int b, const float* tr, int K, int sign) {
  if ((unsigned)b >= (unsigned)K) return v;
  const float g = tr[b];
  return sign < 0 ? v - g : v + g;
}

// x and y may be the same buffer: a thread reads its samples before it writes them, and no other thread touches them
__global__ __launch_bounds__(kThreads) void bin_apply_kernel(const float* x, size_t ld_x, int T, const int* __restrict__ bin,
                                                             const float* __restrict__ tmpl, int K, int sign, float* y, size_t ld_y,
                                                             int wide, int tiles_per_row, long long n_tiles) {
  const int o = threadIdx.x;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / tiles_per_row;
    const int j0 = (int)(tile - row * tiles_per_row) * kTileSamples;
    const float* const xr = x + (size_t)row * ld_x;
    float* const yr = y + (size_t)row * ld_y;
    const float* const tr = tmpl + (size_t)row * K;
    const int q = j0 + kOwn * o;
    if (wide && q + kOwn <= T) {
      const float4 v = *reinterpret_cast<const float4*>(xr + q);
      const int4 b = *reinterpret_cast<const int4*>(bin + q);
      float4 r;
      r.x = shifted(v.x, b.x, tr, K, sign);
      r.y = shifted(v.y, b.y, tr, K, sign);
      r.z = shifted(v.z, b.z, tr, K, sign);
      r.w = shifted(v.w, b.w, tr, K, sign);
      *reinterpret_cast<float4*>(yr + q) = r;
    } else if (wide) {  // the row's last, partial word
      for (int u = 0; u < kOwn; ++u)
        if (q + u < T) yr[q + u] = shifted(xr[q + u], bin[q + u], tr, K, sign);
    } else {  // single words, neighbouring lanes neighbouring samples
#pragma unroll
      for (int u = 0; u < kOwn; ++u) {
        const int t = j0 + o + u * kThreads;
        if (t < T) yr[t] = shifted(xr[t], bin[t], tr, K, sign);
      }
    }
  }
}

}  // namespace

extern "C" {

int mrx_tod_bin_reduce(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m, const uint8_t* d_flags,
                       size_t ld_f, int D, int T, const int32_t* d_order, int n_order, const int32_t* d_start, int K, int min_hits,
                       double* d_sum, uint32_t* d_hits, float* d_template) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_order && d_start, "null pointer");
  MRX_REQUIRE(ctx, d_sum || d_hits || d_template, "no output: d_sum, d_hits and d_template are all null");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, K >= 1 && K <= kMaxBins, "K must be in 1 .. 4096");
  MRX_REQUIRE(ctx, n_order >= 0 && n_order <= T, "n_order must be in 0 .. T");
  MRX_REQUIRE(ctx, min_hits >= 0, "min_hits must be >= 0");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && (!d_model || ld_m >= (size_t)T) && (!d_flags || ld_f >= (size_t)T),
              "ld_x, ld_m or ld_f smaller than T");
  const int groups_per_row = (K + kWaves - 1) / kWaves;
  const long long n_groups = (long long)D * groups_per_row;
  hipLaunchKernelGGL(bin_reduce_kernel, dim3(mrx_resident_blocks(ctx, n_groups)), dim3(kThreads), 0, ctx->stream, d_x, ld_x, d_model, ld_m,
                     d_flags, ld_f, T, d_order, n_order, d_start, K, (unsigned)std::max(min_hits, 1), d_sum, d_hits, d_template,
                     groups_per_row, n_groups);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_bin_apply(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const int32_t* d_bin, const float* d_template, int K,
                      int sign, float* d_y, size_t ld_y) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_bin && d_template && d_y, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, K >= 1 && K <= kMaxBins, "K must be in 1 .. 4096");
  MRX_REQUIRE(ctx, sign == 1 || sign == -1, "sign must be -1 or +1");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && ld_y >= (size_t)T, "ld_x or ld_y smaller than T");
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, D, T, kTileSamples);
  const int wide = mrx_aligned(d_x, ld_x * 4, 16) && mrx_aligned(d_y, ld_y * 4, 16) && mrx_aligned(d_bin, 0, 16) ? 1 : 0;
  hipLaunchKernelGGL(bin_apply_kernel, dim3(g.blocks), dim3(kThreads), 0, ctx->stream, d_x, ld_x, T, d_bin, d_template, K, sign, d_y, ld_y, wide,
                     g.tiles_per_row, g.n_tiles);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // extern "C"
