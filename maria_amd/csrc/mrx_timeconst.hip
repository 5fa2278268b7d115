// Detector time constants of a [D, T] TOD: the one-pole lag of every row and its exact inverse (maria_amd/time_constants.py,
// DESIGN 3.25).  Row d has the pole a = d_a[d] = exp(-1 / (fs tau)); a row whose a is not in (0, 1) is copied.
//   lag       g = 1.0 - a;   y64[0] = init ? (double)x[0] : g * (double)x[0];   y64[t] = a * y64[t - 1] + g * (double)x[t]
//   inverse   r = 1.0 / (1.0 - a);   x[0] = init ? y[0] : (float)((double)y[0] * r)
//             x[t] = (float)(((double)y[t] - a * (double)y[t - 1]) * r)
// The file is built without FMA contraction: every operation above is one float64 rounding.
//
// The lag.  A workgroup owns a row and walks it in the tiles of mrx_tod_dev.h, a thread its own four samples (q is 64 bits:
// the last tile of a row may pass 2^31).  One step of the recurrence is the affine map s -> a s + g x; a run of
// k steps is s -> a^k s + B with B the run's result from a zero state, so that with one pole a row the scan carries the
// B alone and the powers a^4, a^8 .. a^256 are made once a row by squaring, in float64.  Per tile: the thread runs its
// four samples from a zero state (B), the wave scans the 64 B by shuffles (step d: B += a^(4 d) B[lane - d]), the four
// wave totals meet in LDS, every thread chains them on to the float64 carry of the previous tile (s = a^256 s + W_k, in
// order: the state in front of its wave, and after the last one the next tile's carry, which never leaves its
// register), forms the state in front of its own samples, a^(4 lane) * (the wave's) + (the lanes' before it), and runs
// the recurrence itself from there: the float32 results are those of y = a y + g x from a state that is exact to
// float64 rounding.  The wave totals alternate between two LDS slots, so a tile costs one barrier.  The next tile's
// samples are loaded before the scan of the current one (the compiler still waits for them with the current tile's: its
// accesses sit behind branches it cannot count; eight workgroups a CU hide that).  Tiles are counted from
// sample 0 and a sample past T enters as 0: every bit of a row is a function of its samples, a, T and init.  No atomics,
// no word from another workgroup.
//
// The inverse.  A workgroup takes a chunk of consecutive tiles of a row and walks it the same way.  The sample in front
// of a thread's first one is the neighbouring lane's last (a shuffle), the neighbouring wave's last (LDS, the same two
// slots and one barrier) or, for thread 0, the last sample of the previous tile, which the workgroup has kept from
// that tile; at the start of a chunk that is not the start of the row it is read from the input.  In place a chunk is
// the whole row: a thread then reads nothing but its own samples, each before it writes it.
#include "mrx_internal.h"
#include "mrx_tod_dev.h"

#include <algorithm>

namespace {

using namespace mrx_tod;  // the 256-thread, four-sample tile, kWave

constexpr int kScanSteps = 6;    // shuffle distances 1 .. 32
constexpr int kChunkTiles = 16;  // tiles of a work item of the inverse out of place

enum : int { kWideX = 1, kWideY = 2 };

static_assert(kWave == 1 << kScanSteps && kOwn == 4, "64 lanes of four samples");

// x and y may be the same buffer (same pitch): a thread reads its samples before it writes them, and no other thread
// touches them
__global__ __launch_bounds__(kThreads) void onepole_kernel(const float* x, size_t ld_x, int T, const double* __restrict__ pole, int init, float* y,
                                                           size_t ld_y, int wide) {
  __shared__ double wave_total[2][kWaves];
  const int o = threadIdx.x, lane = o & (kWave - 1), wave = o / kWave;
  const size_t row = blockIdx.x;
  const float* const xr = x + row * ld_x;
  float* const yr = y + row * ld_y;
  const int n_tiles = (int)(((long long)T + kTileSamples - 1) / kTileSamples);
  const bool wide_x = (wide & kWideX) != 0, wide_y = (wide & kWideY) != 0;
  const double a = pole[row];
  float v[kOwn], nv[kOwn] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!(a > 0.0 && a < 1.0)) {  // no lag, or no pole at all (NaN compares false): the row is copied.  The same for every thread
    if (x == y) return;
    for (int tile = 0; tile < n_tiles; ++tile) {
      const long long q = (long long)tile * kTileSamples + kOwn * o;
      load_own<kOwn>(xr, q, T, wide_x, v);
      store_own<kOwn>(yr, q, T, wide_y, v);
    }
    return;
  }
  const double g = 1.0 - a;
  double pw[kScanSteps];  // a^4, a^8 .. a^128: what 1, 2 .. 32 threads multiply a state by
  {
    const double a2 = a * a;
    pw[0] = a2 * a2;
#pragma unroll
    for (int s = 1; s < kScanSteps; ++s) pw[s] = pw[s - 1] * pw[s - 1];
  }
  const double a_wave = pw[kScanSteps - 1] * pw[kScanSteps - 1];  // a^256
  double a_lane = 1.0;                                            // a^(4 lane)
#pragma unroll
  for (int s = 0; s < kScanSteps; ++s) a_lane = ((lane >> s) & 1) ? a_lane * pw[s] : a_lane;
  double carry = 0.0;  // y64 of the last sample of the previous tile
  load_own<kOwn>(xr, (long long)kOwn * o, T, wide_x, v);
  for (int tile = 0; tile < n_tiles; ++tile) {  // n_tiles follows from T: every thread of the workgroup makes every round
    const long long q = (long long)tile * kTileSamples + kOwn * o;
    if (tile + 1 < n_tiles) load_own<kOwn>(xr, q + kTileSamples, T, wide_x, nv);  // in flight over this tile's scan
    const bool steady = init != 0 && q == 0;  // sample 0 has seen x[0] for ever: y64[0] = x[0]
    double gx[kOwn];
#pragma unroll
    for (int k = 0; k < kOwn; ++k) gx[k] = g * (double)v[k];
    double b = steady ? (double)v[0] : gx[0];  // the four samples from a zero state
#pragma unroll
    for (int k = 1; k < kOwn; ++k) b = a * b + gx[k];
    double incl = b;
#pragma unroll
    for (int s = 0; s < kScanSteps; ++s) {
      const double up = __shfl_up(incl, 1 << s, kWave);
      if (lane >= (1 << s)) incl = pw[s] * up + incl;
    }
    double before = __shfl_up(incl, 1, kWave);  // the lanes before this one, from a zero state
    if (lane == 0) before = 0.0;
    if (lane == kWave - 1) wave_total[tile & 1][wave] = incl;
    __syncthreads();
    double s = carry, s_wave = carry;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      s_wave = k == wave ? s : s_wave;
      s = a_wave * s + wave_total[tile & 1][k];
    }
    carry = s;
    double state = a_lane * s_wave + before;  // y64 of sample q - 1
    float out[kOwn];
    state = steady ? (double)v[0] : a * state + gx[0];
    out[0] = (float)state;
#pragma unroll
    for (int k = 1; k < kOwn; ++k) {
      state = a * state + gx[k];
      out[k] = (float)state;
    }
    store_own<kOwn>(yr, q, T, wide_y, out);
#pragma unroll
    for (int k = 0; k < kOwn; ++k) v[k] = nv[k];
  }
}

// y: the lagged rows (the input), x: the result.  They may be the same buffer (same pitch) where chunk_tiles covers the row.
__global__ __launch_bounds__(kThreads) void onepole_inverse_kernel(const float* y, size_t ld_y, int T, const double* __restrict__ pole, int init,
                                                                   float* x, size_t ld_x, int wide, int tiles_per_row, int chunk_tiles,
                                                                   int chunks_per_row, long long n_items) {
  __shared__ float wave_last[2][kWaves];
  const int o = threadIdx.x, lane = o & (kWave - 1), wave = o / kWave;
  const bool wide_y = (wide & kWideY) != 0, wide_x = (wide & kWideX) != 0;
  int slot = 0;
  for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
    const long long row = item / chunks_per_row;
    const int tile_lo = (int)(item - row * chunks_per_row) * chunk_tiles;
    const int tile_hi = min(tiles_per_row, tile_lo + chunk_tiles);
    const float* const yr = y + (size_t)row * ld_y;
    float* const xr = x + (size_t)row * ld_x;
    const double a = pole[row];
    const bool lagged = a > 0.0 && a < 1.0;  // the same for every thread
    if (!lagged && x == y) continue;
    const double r = lagged ? 1.0 / (1.0 - a) : 1.0;
    // the sample in front of the chunk (tile_lo > 0: out of place, where nobody writes the input)
    float edge = tile_lo > 0 ? yr[(long long)tile_lo * kTileSamples - 1] : 0.0f;
    float v[kOwn], nv[kOwn] = {0.0f, 0.0f, 0.0f, 0.0f}, out[kOwn];
    load_own<kOwn>(yr, (long long)tile_lo * kTileSamples + kOwn * o, T, wide_y, v);
    for (int tile = tile_lo; tile < tile_hi; ++tile) {
      const long long q = (long long)tile * kTileSamples + kOwn * o;
      if (tile + 1 < tile_hi) load_own<kOwn>(yr, q + kTileSamples, T, wide_y, nv);
      if (lagged) {
        float prev = __shfl_up(v[kOwn - 1], 1, kWave);
        if (lane == kWave - 1) wave_last[slot][wave] = v[kOwn - 1];
        __syncthreads();
        if (lane == 0) prev = wave > 0 ? wave_last[slot][wave - 1] : edge;
        edge = wave_last[slot][kWaves - 1];  // sample q0 + 1023 of a tile that has a successor
        slot ^= 1;
        out[0] = q == 0 ? (init != 0 ? v[0] : (float)((double)v[0] * r)) : (float)(((double)v[0] - a * (double)prev) * r);
#pragma unroll
        for (int k = 1; k < kOwn; ++k) out[k] = (float)(((double)v[k] - a * (double)v[k - 1]) * r);
      } else {
#pragma unroll
        for (int k = 0; k < kOwn; ++k) out[k] = v[k];
      }
      store_own<kOwn>(xr, q, T, wide_x, out);
#pragma unroll
      for (int k = 0; k < kOwn; ++k) v[k] = nv[k];
    }
  }
}

// what both entries refuse; nullptr: nothing
const char* refusal(const float* d_in, size_t ld_in, int D, int T, const double* d_a, int init, const float* d_out, size_t ld_out) {
  if (!d_in || !d_a || !d_out) return "null pointer";
  if (D < 1 || T < 1) return "need D >= 1 rows of T >= 1 samples";
  if (ld_in < (size_t)T || ld_out < (size_t)T) return "ld_x or ld_y smaller than T";
  if (init != 0 && init != 1) return "init must be 0 (zero state) or 1 (steady state)";
  if (d_out == d_in && ld_out != ld_in) return "in place needs the same pitch on both sides";
  return nullptr;
}

}  // namespace

extern "C" {

int mrx_tod_onepole(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const double* d_a, int init, float* d_y, size_t ld_y) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  const char* const bad = refusal(d_x, ld_x, D, T, d_a, init, d_y, ld_y);
  MRX_REQUIRE(ctx, !bad, bad);
  const int wide = (mrx_aligned(d_x, ld_x * 4, 16) ? kWideX : 0) | (mrx_aligned(d_y, ld_y * 4, 16) ? kWideY : 0);
  hipLaunchKernelGGL(onepole_kernel, dim3((unsigned)D), dim3(kThreads), 0, ctx->stream, d_x, ld_x, T, d_a, init, d_y, ld_y, wide);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_onepole_inverse(mrx_ctx* ctx, const float* d_y, size_t ld_y, int D, int T, const double* d_a, int init, float* d_x, size_t ld_x) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  const char* const bad = refusal(d_y, ld_y, D, T, d_a, init, d_x, ld_x);
  MRX_REQUIRE(ctx, !bad, bad);
  const int tiles_per_row = (int)(((long long)T + kTileSamples - 1) / kTileSamples);
  const int chunk_tiles = d_x == d_y ? tiles_per_row : std::min(tiles_per_row, kChunkTiles);  // in place: a workgroup a row
  const int chunks_per_row = (tiles_per_row + chunk_tiles - 1) / chunk_tiles;
  const long long n_items = (long long)D * chunks_per_row;
  const unsigned blocks = mrx_resident_blocks(ctx, n_items);  // as many as stay resident
  const int wide = (mrx_aligned(d_y, ld_y * 4, 16) ? kWideY : 0) | (mrx_aligned(d_x, ld_x * 4, 16) ? kWideX : 0);
  hipLaunchKernelGGL(onepole_inverse_kernel, dim3(blocks), dim3(kThreads), 0, ctx->stream, d_y, ld_y, T, d_a, init, d_x, ld_x, wide,
                     tiles_per_row, chunk_tiles, chunks_per_row, n_items);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // extern "C"
