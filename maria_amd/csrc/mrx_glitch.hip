// Glitch flagging and gap filling of a [D, T] TOD (maria_amd/flagging.py):
//   med[d][t]   = median of x[d][clamp(t + i, 0, T - 1)], -h <= i <= h      (scipy.ndimage.median_filter, mode="nearest")
//   r[d][t]     = x[d][t] - med[d][t]                                        (one float32 subtraction)
//   detection   : |r[d][s]| > thresh[d]
//   flags[d][t] = 1 at a detection, else 2 where a detection s has t - grow_after <= s <= t + grow_before, else 0
//   gap fill    : every maximal run of nonzero flags becomes the line through the means of the <= n_fit unflagged
//                 samples on either side of it.
//
// Residual and flags.  A workgroup takes kTileSamples consecutive samples of one row and stages them, with a halo of
// h (+ the grow reach) samples a side, in LDS as float32; the index is clamped into the row, so the loads do not branch
// and the window of a sample near a row end holds the end sample as often as the edge rule says.  The median is a
// selection by rank counted straight from LDS: element i of a window has the stable rank
//   #{j < i: w[j] <= w[i]} + #{j > i: w[j] < w[i]},
// a permutation of 0 .. 2h whatever ties there are, and the element of rank h is the median.  Thread o takes the samples
// o, o + kThreads, ..: neighbouring lanes read neighbouring words at every (i, j), no bank conflict, and the window is
// never a per-thread array (a runtime h would put one in scratch).  (2h + 1)^2 LDS reads and compares a sample: the
// kernel is bound by them, not by memory, from h = 2 on (DESIGN 3.20 has the times).
// The flag kernel computes the detections of tile + grow reach the same way and keeps them as a bit mask in LDS (a wave
// covers 64 consecutive positions: its ballot is one word).  Then thread o owns the four consecutive samples 4 o .. 4 o + 3
// of the tile: a sample's grown flag is a test of <= 129 consecutive bits (three words), and the four flags go out as one
// 4-byte word where pointer and pitch allow, as bytes otherwise.  The row's count is one integer atomic a tile.
//
// Gap fill.  Threads scan the flags (four consecutive bytes a thread); the thread that finds the start of a run
// (flag[t] && (t == 0 || !flag[t - 1])) walks to the run's end, forms the two anchors and fills the run.  Only flagged
// samples are written and only unflagged ones read, so the pass works in place without a race.  A run costs its length in
// one thread: right for sparse flags, slow (bounded by T) for a row that is mostly flagged.
#include "mrx_internal.h"

#include <algorithm>

namespace {

constexpr int kTileSamples = 1024;  // maria_amd.flagging.TILE_SAMPLES
constexpr int kThreads = 256;
constexpr int kOwn = kTileSamples / kThreads;  // consecutive samples a thread writes flags for
constexpr int kMaxHalf = 15;
constexpr int kMaxGrow = 64;
constexpr int kMaxFit = 16;
constexpr int kMaxWindow = kTileSamples + 2 * (kMaxHalf + kMaxGrow);          // staged samples
constexpr int kStage = (kMaxWindow + kThreads - 1) / kThreads;                  // loads a thread has in flight
constexpr int kMaxDet = kTileSamples + 2 * kMaxGrow;                            // positions with a detection bit
constexpr int kDetWords = (kMaxDet + kThreads - 1) / kThreads * kThreads / 64;  // whole rounds of the workgroup

static_assert(kOwn == 4, "the flag store is one 4-byte word a thread");

// win[m] = x[clamp(s0 + m, 0, T - 1)], m < W <= kMaxWindow
__device__ __forceinline__ void stage_window(const float* __restrict__ xr, int T, long long s0, int W, float* win) {
  const int o = threadIdx.x;
  float v[kStage];
#pragma unroll
  for (int u = 0; u < kStage; ++u)  // always a sample of the row: the loads do not branch
    v[u] = xr[min(max(s0 + o + u * kThreads, 0LL), (long long)T - 1)];
#pragma unroll
  for (int u = 0; u < kStage; ++u)
    if (o + u * kThreads < W) win[o + u * kThreads] = v[u];
}

// the median of w[0 .. 2h]: the element whose stable rank is h
__device__ __forceinline__ float window_median(const float* w, int h) {
  const int n = 2 * h + 1;
  float med = w[h];
  for (int i = 0; i < n; ++i) {
    const float vi = w[i];
    int rank = 0;
    for (int j = 0; j < i; ++j) rank += (w[j] <= vi) ? 1 : 0;
    for (int j = i + 1; j < n; ++j) rank += (w[j] < vi) ? 1 : 0;
    if (rank == h) med = vi;
  }
  return med;
}

__global__ __launch_bounds__(kThreads) void median_residual_kernel(const float* __restrict__ x, size_t ld_x, int T, int h,
                                                                   float* __restrict__ r, size_t ld_r, int tiles_per_row,
                                                                   long long n_tiles) {
  __shared__ float win[kMaxWindow];
  const int o = threadIdx.x;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / tiles_per_row;
    const int j0 = (int)(tile - row * tiles_per_row) * kTileSamples;
    __syncthreads();  // the previous tile's reads of the window are done
    stage_window(x + (size_t)row * ld_x, T, (long long)j0 - h, kTileSamples + 2 * h, win);
    __syncthreads();
    for (int p = o; p < kTileSamples; p += kThreads) {  // win[p + h] is sample j0 + p
      const float res = win[p + h] - window_median(win + p, h);
      if (j0 + p < T) r[(size_t)row * ld_r + j0 + p] = res;
    }
  }
}

// is any bit of [lo, lo + n) set?  n <= 129: at most three words
__device__ __forceinline__ bool any_bit(const unsigned long long* bits, int lo, int n) {
  const int hi = lo + n - 1;
  bool any = false;
  for (int w = lo >> 6; w <= (hi >> 6); ++w) {
    unsigned long long m = bits[w];
    if (w == (lo >> 6)) m &= ~0ULL << (lo & 63);
    if (w == (hi >> 6)) m &= ~0ULL >> (63 - (hi & 63));
    any |= m != 0;
  }
  return any;
}

__global__ __launch_bounds__(kThreads) void glitch_flag_kernel(const float* __restrict__ x, size_t ld_x, int T, int h,
                                                               const float* __restrict__ thresh, int grow_before, int grow_after,
                                                               unsigned char* __restrict__ flags, size_t ld_f, int words,
                                                               unsigned* __restrict__ count, int tiles_per_row, long long n_tiles) {
  __shared__ float win[kMaxWindow];
  __shared__ unsigned long long bits[kDetWords];
  __shared__ unsigned tile_count;
  const int o = threadIdx.x;
  // detection position p is sample j0 - grow_after + p: sample t looks at the positions t - j0 .. t - j0 + reach - 1
  const int reach = grow_after + grow_before + 1;
  const int n_det = kTileSamples + reach - 1;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / tiles_per_row;
    const int j0 = (int)(tile - row * tiles_per_row) * kTileSamples;
    const float limit = thresh[row];
    __syncthreads();  // the previous tile's reads of the window, the bits and the count are done
    if (o == 0) tile_count = 0;
    stage_window(x + (size_t)row * ld_x, T, (long long)j0 - grow_after - h, n_det + 2 * h, win);
    __syncthreads();
    for (int p0 = 0; p0 < n_det; p0 += kThreads) {  // whole rounds: every lane of a wave takes part in the ballot
      const int p = p0 + o;
      const long long s = (long long)j0 - grow_after + p;
      bool det = false;
      if (p < n_det) {  // win[p + h] is sample s (clamped); a position outside the row detects nothing
        const float res = win[p + h] - window_median(win + p, h);
        det = s >= 0 && s < T && fabsf(res) > limit;
      }
      const unsigned long long mask = __ballot(det);
      if ((o & 63) == 0) bits[p >> 6] = mask;
    }
    __syncthreads();
    const int q = kOwn * o;  // the thread's first sample of the tile
    unsigned word = 0, n_set = 0;
#pragma unroll
    for (int u = 0; u < kOwn; ++u) {
      const int pc = q + u + grow_after;  // the sample's own position
      const unsigned f = ((bits[pc >> 6] >> (pc & 63)) & 1ULL) ? 1u : any_bit(bits, q + u, reach) ? 2u : 0u;
      word |= f << (8 * u);
      n_set += (f != 0 && j0 + q + u < T) ? 1u : 0u;
    }
    unsigned char* const fr = flags + (size_t)row * ld_f + j0 + q;
    if (words && j0 + q + kOwn <= T) {
      *reinterpret_cast<unsigned*>(fr) = word;
    } else {
#pragma unroll
      for (int u = 0; u < kOwn; ++u)
        if (j0 + q + u < T) fr[u] = (unsigned char)(word >> (8 * u));
    }
    if (count) {
      if (n_set) atomicAdd(&tile_count, n_set);
      __syncthreads();
      if (o == 0 && tile_count) atomicAdd(count + row, tile_count);
    }
  }
}

__global__ __launch_bounds__(kThreads) void gap_fill_kernel(float* __restrict__ x, size_t ld_x, int T,
                                                            const unsigned char* __restrict__ flags, size_t ld_f, int words, int n_fit,
                                                            unsigned* __restrict__ filled, int tiles_per_row, long long n_tiles) {
  const int o = threadIdx.x;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / tiles_per_row;
    const int t0 = (int)(tile - row * tiles_per_row) * kTileSamples + kOwn * o;
    if (t0 >= T) continue;
    const unsigned char* const fr = flags + (size_t)row * ld_f;
    float* const xr = x + (size_t)row * ld_x;
    unsigned word = 0;
    if (words && t0 + kOwn <= T) {
      word = *reinterpret_cast<const unsigned*>(fr + t0);
    } else {
      for (int u = 0; u < kOwn; ++u)
        if (t0 + u < T) word |= (unsigned)fr[t0 + u] << (8 * u);
    }
    if (!word) continue;
    bool before = t0 > 0 && fr[t0 - 1] != 0;
    for (int u = 0; u < kOwn; ++u) {
      const bool here = ((word >> (8 * u)) & 0xFFu) != 0;
      if (here && !before) {  // the run [a, b) starts here
        const int a = t0 + u;
        int b = a + 1;
        while (b < T && fr[b]) ++b;
        if (a > 0 || b < T) {  // a row flagged from end to end stays as it is
          double yL = 0.0, tL = 0.0, yR = 0.0, tR = 0.0;
          int nL = 0, nR = 0;
          for (int k = max(0, a - n_fit); k < a; ++k)
            if (!fr[k]) { yL += (double)xr[k]; tL += (double)k; ++nL; }
          for (int k = b; k < min(T, b + n_fit); ++k)
            if (!fr[k]) { yR += (double)xr[k]; tR += (double)k; ++nR; }
          if (nL) { yL /= nL; tL /= nL; }
          if (nR) { yR /= nR; tR /= nR; }
          if (a == 0) {
            for (int t = a; t < b; ++t) xr[t] = (float)yR;
          } else if (b == T) {
            for (int t = a; t < b; ++t) xr[t] = (float)yL;
          } else {
            for (int t = a; t < b; ++t) xr[t] = (float)(yL + (yR - yL) * ((double)t - tL) / (tR - tL));
          }
          if (filled) atomicAdd(filled + row, (unsigned)(b - a));
        }
      }
      before = here;
    }
  }
}

}  // namespace

extern "C" {

int mrx_tod_median_residual(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, int half_window, float* d_r, size_t ld_r) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_r, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && ld_r >= (size_t)T, "ld_x or ld_r smaller than T");
  MRX_REQUIRE(ctx, half_window >= 1 && half_window <= kMaxHalf, "half_window must be in 1 .. 15");
  MRX_REQUIRE(ctx, (const void*)d_r != (const void*)d_x, "d_r must not be d_x");
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, D, T, kTileSamples);
  hipLaunchKernelGGL(median_residual_kernel, dim3(g.blocks), dim3(kThreads), 0, ctx->stream, d_x, ld_x, T, half_window, d_r, ld_r,
                     g.tiles_per_row, g.n_tiles);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_glitch_flag(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, int half_window, const float* d_thresh,
                        int grow_before, int grow_after, uint8_t* d_flags, size_t ld_f, uint32_t* d_count) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_thresh && d_flags, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && ld_f >= (size_t)T, "ld_x or ld_f smaller than T");
  MRX_REQUIRE(ctx, half_window >= 1 && half_window <= kMaxHalf, "half_window must be in 1 .. 15");
  MRX_REQUIRE(ctx, grow_before >= 0 && grow_before <= kMaxGrow && grow_after >= 0 && grow_after <= kMaxGrow,
              "grow_before and grow_after must be in 0 .. 64");
  if (d_count) MRX_HIP(ctx, hipMemsetAsync(d_count, 0, (size_t)D * sizeof(uint32_t), ctx->stream));
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, D, T, kTileSamples);
  hipLaunchKernelGGL(glitch_flag_kernel, dim3(g.blocks), dim3(kThreads), 0, ctx->stream, d_x, ld_x, T, half_window, d_thresh,
                     grow_before, grow_after, d_flags, ld_f, (int)mrx_aligned(d_flags, ld_f, 4), d_count, g.tiles_per_row, g.n_tiles);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_gap_fill(mrx_ctx* ctx, float* d_x, size_t ld_x, int D, int T, const uint8_t* d_flags, size_t ld_f, int n_fit,
                     uint32_t* d_filled) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_flags, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && ld_f >= (size_t)T, "ld_x or ld_f smaller than T");
  MRX_REQUIRE(ctx, n_fit >= 1 && n_fit <= kMaxFit, "n_fit must be in 1 .. 16");
  if (d_filled) MRX_HIP(ctx, hipMemsetAsync(d_filled, 0, (size_t)D * sizeof(uint32_t), ctx->stream));
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, D, T, kTileSamples);
  hipLaunchKernelGGL(gap_fill_kernel, dim3(g.blocks), dim3(kThreads), 0, ctx->stream, d_x, ld_x, T, d_flags, ld_f,
                     (int)mrx_aligned(d_flags, ld_f, 4), n_fit, d_filled, g.tiles_per_row, g.n_tiles);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // extern "C"
