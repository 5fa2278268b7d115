// Jumps (sudden, persistent changes of a row's baseline) of a [D, T] TOD: find them, measure them, take them out
// (maria_amd/jumps.py).  With w = window, g = gap, m = min_count, and a sample VALID if it is inside the row
// and its flag is 0:
//   step statistic  s[d][t] = mean of the valid samples of [t + g, t + g + w) - mean of those of [t - g - w, t - g),
//                   0 where either side has fewer than m of them
//   peak            |s[t]| > thresh[d], |s[u]| < |s[t]| on [t - sep, t), |s[u]| <= |s[t]| on (t, t + sep]
//   height          the same difference of means at a listed jump, the windows clipped at the neighbouring jumps
//   fix             y[t] = x[t] - the sum of the heights of the jumps at or before t
//
// Statistic.  A workgroup takes kTileSamples consecutive samples of a row and stages them with a halo of w + g samples a
// side into LDS as float32, four samples a thread (one 16-byte load where pointer and pitch allow it); a sample that is
// flagged or outside the row is staged as NaN (inputs are finite, so NaN is free to mean "not valid").  Thread o then
// owns the kChunk consecutive staged elements from kChunk * o: it adds them up in float64 with their count, the waves
// scan the threads' totals with shuffles, the four wave totals are carried through LDS, and the thread writes the
// inclusive prefix sums of values and counts of its elements.  Element 0 is an empty one in front of the first sample,
// so prefix[b] - prefix[a] is the sum of the staged samples a .. b - 1: a sample's two sums and two counts are four LDS
// reads each, whatever w is.  The results go through LDS once more so that a thread stores four consecutive samples.
//
// Finder.  The workgroup stages |s| of tile + grow reach + sep a side (-1 outside the row: below every |s|), builds the
// running maxima M_k[i] = max |s|[i .. i + 2^k) by doubling between two LDS buffers up to 2^k <= sep, and reads the maximum of
// the sep samples before and after a position as two overlapping M_k each: log2(sep) passes over the staged samples in
// place of 2 sep reads a sample.  The peaks are kept as a bit mask in LDS and grown as mrx_glitch.hip grows detections.
//
// Height: one wave a row walks the row's jumps; the lanes stride over a window and the wave adds their float64 partial
// sums up (mrx_tod_dev.h: wave_sum_all), an order that depends on the list alone.  Fix: a thread owns four consecutive samples, finds
// the number of jumps at or before its first by bisection of the row's list and walks on from there.
#include "mrx_internal.h"
#include "mrx_tod_dev.h"

#include <algorithm>

namespace {

using namespace mrx_tod;  // the 256-thread, four-sample tile (kTileSamples is maria_amd.jumps.TILE_SAMPLES), kWave

constexpr int kMaxWindow = 256;                // maria_amd.jumps.MAX_WINDOW
constexpr int kMaxGap = 64;                    // maria_amd.jumps.MAX_GAP
constexpr int kMaxSep = 512;                   // maria_amd.jumps.MAX_SEP
constexpr int kMaxGrow = 64;

constexpr int kStatSamples = kTileSamples + 2 * (kMaxWindow + kMaxGap);  // staged samples of the statistic
constexpr int kChunk = (kStatSamples + 1 + kThreads - 1) / kThreads;     // prefix elements a thread owns
constexpr int kStatElems = kChunk * kThreads;
constexpr int kStatStage = (kStatSamples + 3 + 3) / 4 * 4;  // floats staged: up to 3 in front to start on a quad

constexpr int kFindSamples = kTileSamples + 2 * kMaxGrow + 2 * kMaxSep;
constexpr int kFindStage = (kFindSamples + 3 + 3) / 4 * 4;
constexpr int kMaxDet = kTileSamples + 2 * kMaxGrow;                            // positions with a peak bit
constexpr int kDetRounds = (kMaxDet + kThreads - 1) / kThreads;                 // positions a thread tests
constexpr int kDetWords = kDetRounds * kThreads / 64;

static_assert(kTileSamples == 1024, "maria_amd.jumps.TILE_SAMPLES");
static_assert(kTileSamples <= kStatStage, "the statistic's results reuse the staging array");
static_assert((kTileSamples - 1) / 64 + 2 < kDetWords, "any_bit reads three words from a sample's own");

// dst[4 q + i] = sample sA + 4 q + i of the row for q < n_quads (sA a multiple of 4, possibly negative): `fill` where the
// sample is outside [0, T) or its flag is nonzero, else the value (kAbs: its magnitude).  A quad inside the row is one
// 16-byte load (flags: one 4-byte load) where wide_x (wide_f) says pointer and pitch allow it.
template <bool kAbs>
__device__ __forceinline__ void stage_quads(const float* __restrict__ xr, const unsigned char* __restrict__ fr, int T, long long sA,
                                            int n_quads, int wide_x, int wide_f, float fill, float* dst) {
  for (int q = threadIdx.x; q < n_quads; q += kThreads) {
    const long long s = sA + 4LL * q;
    const bool inside = s >= 0 && s + 4 <= (long long)T;
    float v[4];
    unsigned f = 0;
    if (inside && wide_x) {
      const float4 w = *reinterpret_cast<const float4*>(xr + s);
      v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = (unsigned long long)(s + i) < (unsigned long long)T ? xr[s + i] : fill;
    }
    if (fr) {
      if (inside && wide_f) {
        f = *reinterpret_cast<const unsigned*>(fr + s);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if ((unsigned long long)(s + i) < (unsigned long long)T) f |= (unsigned)fr[s + i] << (8 * i);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool out = (unsigned long long)(s + i) >= (unsigned long long)T || ((f >> (8 * i)) & 0xFFu) != 0;
      v[i] = out ? fill : (kAbs ? fabsf(v[i]) : v[i]);
    }
    *reinterpret_cast<float4*>(dst + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

__global__ __launch_bounds__(kThreads) void step_stat_kernel(const float* __restrict__ x, size_t ld_x, const unsigned char* __restrict__ flags,
                                                             size_t ld_f, int T, int w, int g, int min_count, float* __restrict__ s_out,
                                                             size_t ld_s, int wide_x, int wide_f, int wide_s, int tiles_per_row,
                                                             long long n_tiles) {
  __shared__ __attribute__((aligned(16))) float vals[kStatStage];
  __shared__ double psum[kStatElems];
  __shared__ int pcnt[kStatElems];
  __shared__ double wave_sum[kWaves];
  __shared__ int wave_cnt[kWaves];
  const int o = threadIdx.x, lane = o & 63, wave = o >> 6;
  const int halo = w + g;
  const int W = kTileSamples + 2 * halo;  // staged samples; prefix elements 0 .. W
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / tiles_per_row;
    const int j0 = (int)(tile - row * tiles_per_row) * kTileSamples;
    const long long s0 = (long long)j0 - halo;  // prefix element e >= 1 is sample s0 + e - 1
    const long long sA = s0 & ~3LL;
    const int off = (int)(s0 - sA);
    __syncthreads();  // the previous tile's reads of vals, psum and pcnt are done
    stage_quads<false>(x + (size_t)row * ld_x, flags ? flags + (size_t)row * ld_f : nullptr, T, sA, (off + W + 3) / 4, wide_x, wide_f,
                       __builtin_nanf(""), vals);
    __syncthreads();
    // the thread's own elements, then the scan of the threads' totals
    double loc[kChunk], run = 0.0;
    int lc[kChunk], cnt = 0;
#pragma unroll
    for (int u = 0; u < kChunk; ++u) {
      const int e = kChunk * o + u;
      const float v = (e >= 1 && e <= W) ? vals[e - 1 + off] : __builtin_nanf("");
      const bool ok = v == v;
      run += ok ? (double)v : 0.0;
      cnt += ok ? 1 : 0;
      loc[u] = run, lc[u] = cnt;
    }
    double incl = run;
    int incl_c = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double a = __shfl_up(incl, d);
      const int c = __shfl_up(incl_c, d);
      if (lane >= d) incl += a, incl_c += c;
    }
    double before = __shfl_up(incl, 1);
    int before_c = __shfl_up(incl_c, 1);
    if (lane == 0) before = 0.0, before_c = 0;
    if (lane == 63) wave_sum[wave] = incl, wave_cnt[wave] = incl_c;
    __syncthreads();
    double carry = 0.0;
    int carry_c = 0;
    for (int k = 0; k < wave; ++k) carry += wave_sum[k], carry_c += wave_cnt[k];
    before += carry, before_c += carry_c;
#pragma unroll
    for (int u = 0; u < kChunk; ++u) psum[kChunk * o + u] = before + loc[u], pcnt[kChunk * o + u] = before_c + lc[u];
    __syncthreads();
    // sample j0 + p: L is the elements p .. p + w - 1 past element p, R those past element p + w + 2 g
#pragma unroll
    for (int u = 0; u < kOwn; ++u) {
      const int p = o + u * kThreads;
      const int a = p + w, b = p + w + 2 * g, c = b + w;
      const int nL = pcnt[a] - pcnt[p], nR = pcnt[c] - pcnt[b];
      float res = 0.0f;
      if (nL >= min_count && nR >= min_count) {
        const double mL = (psum[a] - psum[p]) / (double)nL;
        const double mR = (psum[c] - psum[b]) / (double)nR;
        res = (float)(mR - mL);
      }
      vals[p] = res;  // every read of the staged samples was before the last barrier
    }
    __syncthreads();
    const int q = kOwn * o;
    float* const sr = s_out + (size_t)row * ld_s + j0 + q;
    if (wide_s && j0 + q + kOwn <= T) {
      *reinterpret_cast<float4*>(sr) = *reinterpret_cast<const float4*>(vals + q);
    } else {
#pragma unroll
      for (int u = 0; u < kOwn; ++u)
        if (j0 + q + u < T) sr[u] = vals[q + u];
    }
  }
}

// the lowest k bits set, 0 <= k <= 64
__device__ __forceinline__ unsigned long long low_bits(int k) { return k >= 64 ? ~0ULL : (1ULL << k) - 1ULL; }

// is any bit of [lo, lo + n) set?  1 <= n <= 129: three words, read without a branch (lo + 191 is inside the mask)
__device__ __forceinline__ bool any_bit(const unsigned long long* bits, int lo, int n) {
  const int w = lo >> 6, b = lo & 63;
  const int n0 = min(n, 64 - b), n1 = min(n - n0, 64), n2 = n - n0 - n1;
  return (((bits[w] >> b) & low_bits(n0)) | (bits[w + 1] & low_bits(n1)) | (bits[w + 2] & low_bits(n2))) != 0;
}

__global__ __launch_bounds__(kThreads) void jump_find_kernel(const float* __restrict__ s, size_t ld_s, int T, const float* __restrict__ thresh,
                                                             int sep, int grow_before, int grow_after, unsigned char* __restrict__ flags,
                                                             size_t ld_f, int wide_s, int words, unsigned* __restrict__ count,
                                                             int tiles_per_row, long long n_tiles) {
  __shared__ __attribute__((aligned(16))) float amax[2][kFindStage];
  __shared__ unsigned long long bits[kDetWords];
  __shared__ unsigned tile_count;
  const int o = threadIdx.x;
  // peak position p is sample j0 - grow_after + p: sample t looks at the positions t - j0 .. t - j0 + reach - 1
  const int reach = grow_after + grow_before + 1;
  const int n_det = kTileSamples + reach - 1;
  const int W = n_det + 2 * sep;  // staged samples
  int K = 0;                      // 2^K <= sep < 2^(K + 1)
  while ((2 << K) <= sep) ++K;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / tiles_per_row;
    const int j0 = (int)(tile - row * tiles_per_row) * kTileSamples;
    const float limit = thresh[row];
    const long long s0 = (long long)j0 - grow_after - sep;  // position p is staged element p + sep + off
    const long long sA = s0 & ~3LL;
    const int off = (int)(s0 - sA);
    const int n_stage = (off + W + 3) / 4 * 4;
    __syncthreads();  // the previous tile's reads of the maxima, the bits and the count are done
    if (o == 0) tile_count = 0;
    stage_quads<true>(s + (size_t)row * ld_s, nullptr, T, sA, n_stage / 4, wide_s, 0, -1.0f, amax[0]);
    __syncthreads();
    float own[kDetRounds];
#pragma unroll
    for (int r = 0; r < kDetRounds; ++r) {
      const int p = o + r * kThreads;
      own[r] = p < n_det ? amax[0][p + sep + off] : 0.0f;
    }
    for (int k = 0; k < K; ++k) {  // amax[(k + 1) & 1][i] = max of the 2^(k + 1) samples from i on
      const float* const from = amax[k & 1];
      float* const to = amax[(k + 1) & 1];
      const int step = 1 << k;
      for (int i = o; i < n_stage; i += kThreads) to[i] = i + step < n_stage ? fmaxf(from[i], from[i + step]) : from[i];
      __syncthreads();
    }
    const float* const mk = amax[K & 1];
    const int span = 1 << K;
#pragma unroll
    for (int r = 0; r < kDetRounds; ++r) {  // whole rounds: every lane of a wave takes part in the ballot
      const int p = o + r * kThreads;
      const long long t = (long long)j0 - grow_after + p;
      bool peak = false;
      if (p < n_det && t >= 0 && t < T) {
        const int i = p + sep + off;
        const float a = own[r];
        const float left = fmaxf(mk[i - sep], mk[i - span]);            // [i - sep, i)
        const float right = fmaxf(mk[i + 1], mk[i + sep - span + 1]);  // (i, i + sep]
        peak = a > limit && left < a && right <= a;
      }
      const unsigned long long mask = __ballot(peak);
      if ((o & 63) == 0) bits[p >> 6] = mask;
    }
    __syncthreads();
    const int q = kOwn * o;  // the thread's first sample of the tile
    unsigned word = 0, n_peaks = 0;
#pragma unroll
    for (int u = 0; u < kOwn; ++u) {
      const int pc = q + u + grow_after;  // the sample's own position
      const unsigned f = ((bits[pc >> 6] >> (pc & 63)) & 1ULL) ? 1u : any_bit(bits, q + u, reach) ? 2u : 0u;
      word |= f << (8 * u);
      n_peaks += (f == 1 && j0 + q + u < T) ? 1u : 0u;
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
      if (n_peaks) atomicAdd(&tile_count, n_peaks);
      __syncthreads();
      if (o == 0 && tile_count) atomicAdd(count + row, tile_count);
    }
  }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// sum and count of the valid samples of [a, b) of a row, the same in every lane of the wave
__device__ __forceinline__ void wave_window(const float* __restrict__ xr, const unsigned char* __restrict__ fr, int a, int b, double* sum,
                                            int* n) {
  double acc = 0.0;
  int cnt = 0;
  for (int u = a + (int)(threadIdx.x & 63); u < b; u += 64) {
    if (!fr || fr[u] == 0) acc += (double)xr[u], ++cnt;
  }
  wave_sum_all(acc, cnt);
  *sum = acc, *n = cnt;
}

__global__ __launch_bounds__(kThreads) void jump_height_kernel(const float* __restrict__ x, size_t ld_x, const unsigned char* __restrict__ flags,
                                                               size_t ld_f, int D, int T, const int* __restrict__ row_start,
                                                               const int* __restrict__ pos, int n, int w, int g, int min_count,
                                                               double* __restrict__ height, unsigned char* __restrict__ ok) {
  const int row = blockIdx.x * kWaves + (int)(threadIdx.x >> 6);
  if (row >= D) return;
  const float* const xr = x + (size_t)row * ld_x;
  const unsigned char* const fr = flags ? flags + (size_t)row * ld_f : nullptr;
  const int js = clampi(row_start[row], 0, n), je = clampi(row_start[row + 1], 0, n);
  for (int j = js; j < je; ++j) {
    const int p = clampi(pos[j], 0, T - 1);
    int lo = max(0, p - g - w), hi = min(T, p + g + w);
    if (j > js) lo = max(lo, clampi(pos[j - 1], 0, T - 1) + g);
    if (j + 1 < je) hi = min(hi, clampi(pos[j + 1], 0, T - 1) - g);
    double sL, sR;
    int nL, nR;
    wave_window(xr, fr, lo, p - g, &sL, &nL);
    wave_window(xr, fr, p + g, hi, &sR, &nR);
    if ((threadIdx.x & 63) == 0) {
      const bool good = nL >= min_count && nR >= min_count;
      height[j] = good ? sR / (double)nR - sL / (double)nL : 0.0;
      ok[j] = good ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(kThreads) void jump_fix_kernel(const float* x, size_t ld_x, int T, const int* __restrict__ row_start,
                                                            const int* __restrict__ pos, const double* __restrict__ cum, int n, float* y,
                                                            size_t ld_y, int wide, int tiles_per_row, long long n_tiles) {
  const int o = threadIdx.x;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / tiles_per_row;
    const int t0 = (int)(tile - row * tiles_per_row) * kTileSamples + kOwn * o;
    if (t0 >= T) continue;
    const int js = clampi(row_start[row], 0, n), je = max(js, clampi(row_start[row + 1], 0, n));
    if (js == je && x == y) continue;  // in place, and no jump in the row
    int a = 0, b = je - js;  // k = the number of the row's jumps at or before t0
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (pos[js + mid] <= t0) a = mid + 1; else b = mid;
    }
    int k = a;
    float v[kOwn];
    load_own<kOwn>(x + (size_t)row * ld_x, t0, T, wide, v);
#pragma unroll
    for (int u = 0; u < kOwn; ++u) {
      while (js + k < je && pos[js + k] <= t0 + u) ++k;
      if (k > 0) v[u] = (float)((double)v[u] - cum[js + k - 1]);
    }
    store_own<kOwn>(y + (size_t)row * ld_y, t0, T, wide, v);
  }
}

const char* bad_window(int window, int gap, int min_count) {
  if (window < 2 || window > kMaxWindow) return "window must be in 2 .. 256";
  if (gap < 0 || gap > kMaxGap) return "gap must be in 0 .. 64";
  if (min_count < 1 || min_count > window) return "min_count must be in 1 .. window";
  return nullptr;
}

}  // namespace

extern "C" {

int mrx_tod_step_stat(mrx_ctx* ctx, const float* d_x, size_t ld_x, const uint8_t* d_flags, size_t ld_f, int D, int T, int window, int gap,
                      int min_count, float* d_s, size_t ld_s) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_s, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && ld_s >= (size_t)T && (!d_flags || ld_f >= (size_t)T), "ld_x, ld_f or ld_s smaller than T");
  const char* const bad = bad_window(window, gap, min_count);
  MRX_REQUIRE(ctx, !bad, bad);
  MRX_REQUIRE(ctx, (const void*)d_s != (const void*)d_x, "d_s must not be d_x");
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, D, T, kTileSamples, 5);
  hipLaunchKernelGGL(step_stat_kernel, dim3(g.blocks), dim3(kThreads), 0, ctx->stream, d_x, ld_x, d_flags, ld_f, T, window, gap, min_count,
                     d_s, ld_s, (int)mrx_aligned(d_x, ld_x * 4, 16), (int)(d_flags && mrx_aligned(d_flags, ld_f, 4)),
                     (int)mrx_aligned(d_s, ld_s * 4, 16), g.tiles_per_row, g.n_tiles);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_jump_find(mrx_ctx* ctx, const float* d_s, size_t ld_s, int D, int T, const float* d_thresh, int sep, int grow_before,
                      int grow_after, uint8_t* d_flags, size_t ld_f, uint32_t* d_count) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_s && d_thresh && d_flags, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, ld_s >= (size_t)T && ld_f >= (size_t)T, "ld_s or ld_f smaller than T");
  MRX_REQUIRE(ctx, sep >= 1 && sep <= kMaxSep, "sep must be in 1 .. 512");
  MRX_REQUIRE(ctx, grow_before >= 0 && grow_before <= kMaxGrow && grow_after >= 0 && grow_after <= kMaxGrow,
              "grow_before and grow_after must be in 0 .. 64");
  if (d_count) MRX_HIP(ctx, hipMemsetAsync(d_count, 0, (size_t)D * sizeof(uint32_t), ctx->stream));
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, D, T, kTileSamples);
  hipLaunchKernelGGL(jump_find_kernel, dim3(g.blocks), dim3(kThreads), 0, ctx->stream, d_s, ld_s, T, d_thresh, sep, grow_before, grow_after,
                     d_flags, ld_f, (int)mrx_aligned(d_s, ld_s * 4, 16), (int)mrx_aligned(d_flags, ld_f, 4), d_count, g.tiles_per_row,
                     g.n_tiles);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_jump_height(mrx_ctx* ctx, const float* d_x, size_t ld_x, const uint8_t* d_flags, size_t ld_f, int D, int T,
                        const int32_t* d_row_start, const int32_t* d_pos, int n, int window, int gap, int min_count, double* d_height,
                        uint8_t* d_ok) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_row_start, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, n >= 0, "n must be >= 0");
  MRX_REQUIRE(ctx, n == 0 || (d_pos && d_height && d_ok), "null pointer");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && (!d_flags || ld_f >= (size_t)T), "ld_x or ld_f smaller than T");
  const char* const bad = bad_window(window, gap, min_count);
  MRX_REQUIRE(ctx, !bad, bad);
  if (n == 0) return MRX_OK;
  hipLaunchKernelGGL(jump_height_kernel, dim3((unsigned)((D + kWaves - 1) / kWaves)), dim3(kThreads), 0, ctx->stream, d_x, ld_x, d_flags, ld_f,
                     D, T, d_row_start, d_pos, n, window, gap, min_count, d_height, d_ok);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_jump_fix(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const int32_t* d_row_start, const int32_t* d_pos,
                     const double* d_cum, int n, float* d_y, size_t ld_y) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_y && d_row_start, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, n >= 0, "n must be >= 0");
  MRX_REQUIRE(ctx, n == 0 || (d_pos && d_cum), "null pointer");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && ld_y >= (size_t)T, "ld_x or ld_y smaller than T");
  MRX_REQUIRE(ctx, (const void*)d_y != (const void*)d_x || ld_y == ld_x, "in place (d_y == d_x) needs ld_y == ld_x");
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, D, T, kTileSamples);
  hipLaunchKernelGGL(jump_fix_kernel, dim3(g.blocks), dim3(kThreads), 0, ctx->stream, d_x, ld_x, T, d_row_start, d_pos, d_cum, n, d_y, ld_y,
                     (int)(mrx_aligned(d_x, ld_x * 4, 16) && mrx_aligned(d_y, ld_y * 4, 16)), g.tiles_per_row, g.n_tiles);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // extern "C"
