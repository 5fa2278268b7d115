// A rotating half-wave plate in the time domain (maria_amd/hwp.py).
//
// mrx_tod_demodulate: the lock-in decimator of a [D, T] TOD against the carrier c[t] = (cos 4 chi, sin 4 chi),
//   y_t[d][j] =     sum_i hT[H + i]               x[d][j q + i] / sum_i hT[H + i]
//   y_q[d][j] = 2 * sum_i hP[H + i] c[j q + i][0] x[d][j q + i] / sum_i hP[H + i]
//   y_u[d][j] = 2 * sum_i hP[H + i] c[j q + i][1] x[d][j q + i] / sum_i hP[H + i],   -H <= i <= H,  0 <= j q + i < T,
// in one pass over x.  The structure is mrx_decimate.hip's: a workgroup takes kTileOutputs consecutive outputs of one
// row, thread o the output j0 + o, and stages the W = (kTileOutputs - 1) q + n_taps samples from j0 q - H on in LDS,
// de-interleaved by phase (sample m of the window at (m mod q) P + m / q), so that tap k = c q + r of output o reads word
// r P + o + c: neighbouring lanes neighbouring words.  New here: while staging, the carrier's two values at the sample
// are read (they are the same for every row: L2), and THREE windows are written, x as it is (float32: the conversion to
// float64 is exact and happens at the read), and the float64 products c[.][0] x and c[.][1] x, rounded once.  A tap then
// costs three LDS reads and three float64 FMAs, its two coefficients hT[k] and hP[k] scalar loads.  The sums run over
// k ascending: y_t is mrx_tod_decimate's sum operation by operation, and the denominators are the same prefix-sum
// differences, built in the same order (chunks of kPrefixChunk taps, as that kernel's 256 threads sum them).
//
// The tile is 128 outputs (the decimator's 256 would need 184 KB at q = 32 with 1025 taps): 20 bytes a window sample,
// P made odd (the staging writes of neighbouring lanes are P words apart).  LDS a workgroup: 2 x 1026 doubles of prefix
// sums + 20 q P bytes: 47.3 KB at q = 8 with 523 taps (3 workgroups a CU), 119.5 KB at the worst shape (1 a CU).
//
// mrx_tod_hwp_modulate: out = float32( i + c cos 4 chi + s sin 4 chi ) as fma(s, sin, fma(c, cos, i)) in float64, one
// rounding to float32; a streaming pass, a thread its own four samples (mrx_tod_dev.h), in place where d_out == d_i.
#include "mrx_internal.h"
#include "mrx_tod_dev.h"

#include <algorithm>

namespace {

constexpr int kTileOutputs = 128;  // maria_amd.hwp.TILE_OUTPUTS
constexpr int kThreads = kTileOutputs;
constexpr int kMaxTaps = 1025;
constexpr int kMaxFactor = 32;
constexpr int kPrefixChunks = 256;                                              // mrx_decimate.hip: its threads
constexpr int kPrefixChunk = (kMaxTaps + kPrefixChunks - 1) / kPrefixChunks;    // ... and the taps each of them sums
constexpr int kPrefixDoubles = kMaxTaps + 1;
constexpr int kStage = 4;  // window samples a thread loads before it writes them to LDS

// pre[i] = h[0] + .. + h[i - 1], i <= n_taps, by the additions of mrx_decimate.hip in their order: chunk c's sum, the
// sums of the chunks before it one by one, then its taps one by one.  part: kPrefixChunks doubles of scratch.
__device__ __forceinline__ void build_prefix(const double* __restrict__ taps, int n_taps, double* pre, double* part) {
  const int o = threadIdx.x;
  for (int c = o; c < kPrefixChunks; c += kThreads) {
    const int k0 = c * kPrefixChunk;
    double s = 0.0;
    for (int i = 0; i < kPrefixChunk; ++i)
      if (k0 + i < n_taps) s += taps[k0 + i];
    part[c] = s;
  }
  __syncthreads();
  if (o == 0) pre[0] = 0.0;
  for (int c = o; c < kPrefixChunks; c += kThreads) {
    const int k0 = c * kPrefixChunk;
    if (k0 >= n_taps) break;
    double run = 0.0;
    for (int t = 0; t < c; ++t) run += part[t];
    for (int i = 0; i < kPrefixChunk; ++i) {
      if (k0 + i < n_taps) {
        run += taps[k0 + i];
        pre[k0 + i + 1] = run;
      }
    }
  }
  __syncthreads();  // part is free again
}

template <bool kWantT>
__global__ __launch_bounds__(kThreads) void tod_demodulate_kernel(const float* __restrict__ x, size_t ld_x, int T, int q, unsigned q_magic,
                                                                  const double* __restrict__ carrier, const double* __restrict__ taps_t,
                                                                  const double* __restrict__ taps_p, int n_taps, float* __restrict__ yt,
                                                                  float* __restrict__ yq, float* __restrict__ yu, size_t ld_y, int T_out,
                                                                  int P, int tiles_per_row, long long n_tiles) {
  extern __shared__ double lds[];
  double* const pre_t = lds;                   // prefix sums of hT
  double* const pre_p = lds + kPrefixDoubles;  // ... of hP
  double* const win_c = lds + 2 * kPrefixDoubles;  // [q][P]: x cos
  double* const win_s = win_c + q * P;             // [q][P]: x sin
  float* const win_x = reinterpret_cast<float*>(win_s + q * P);  // [q][P]: x
  const int o = threadIdx.x;
  const int H = (n_taps - 1) / 2;
  const int W = (kTileOutputs - 1) * q + n_taps;

  if (kWantT) build_prefix(taps_t, n_taps, pre_t, win_c);  // (q P >= 2 kTileOutputs doubles of scratch, before any window)
  build_prefix(taps_p, n_taps, pre_p, win_c);

  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / tiles_per_row;
    const int j0 = (int)(tile - row * tiles_per_row) * kTileOutputs;
    const float* const xr = x + (size_t)row * ld_x;
    const long long s0 = (long long)j0 * q - H;  // the window's first sample
    __syncthreads();                             // the previous tile's reads of the windows are done
    for (int m0 = o; m0 < W; m0 += kStage * kThreads) {
      float v[kStage];
      double vc[kStage], vs[kStage];
#pragma unroll
      for (int u = 0; u < kStage; ++u) {  // always a sample of the row: the loads do not branch
        const long long s = min(max(s0 + m0 + u * kThreads, 0LL), (long long)T - 1);
        v[u] = xr[s];
        vc[u] = carrier[2 * s];
        vs[u] = carrier[2 * s + 1];
      }
#pragma unroll
      for (int u = 0; u < kStage; ++u) {
        const int m = m0 + u * kThreads;
        const long long s = s0 + m;
        const int c = (int)__umulhi((unsigned)m, q_magic);  // m / q (m < 2^16)
        if (m < W) {
          const bool in = s >= 0 && s < T;
          const int w = (m - c * q) * P + c;
          const double xd = (double)v[u];
          win_x[w] = in ? v[u] : 0.0f;
          win_c[w] = in ? vc[u] * xd : 0.0;
          win_s[w] = in ? vs[u] * xd : 0.0;
        }
      }
    }
    __syncthreads();
    const float* const xo = win_x + o;
    const double* const co = win_c + o;
    const double* const so = win_s + o;
    double at = 0.0, aq = 0.0, au = 0.0;
#pragma unroll 2  // (four taps of both sets in scalar registers at a time push the kernel past its 102 and into spills)
    for (int k = 0, r = 0, w = 0; k < n_taps; ++k) {  // tap k = c q + r: word w = r P + c (+ o)
      const double hp = taps_p[k];
      if (kWantT) at = fma(taps_t[k], (double)xo[w], at);
      aq = fma(hp, co[w], aq);
      au = fma(hp, so[w], au);
      w += P;
      if (++r == q) {
        r = 0;
        w -= q * P - 1;
      }
    }
    const int j = j0 + o;
    if (j < T_out) {
      const long long first = (long long)j * q;  // input sample of tap H
      const int lo = (int)max(0LL, (long long)H - first);
      const int hi = (int)min((long long)n_taps - 1, (long long)H + (T - 1) - first);
      const size_t at_y = (size_t)row * ld_y + j;
      const double den_p = pre_p[hi + 1] - pre_p[lo];
      if (kWantT) yt[at_y] = (float)(at / (pre_t[hi + 1] - pre_t[lo]));
      yq[at_y] = (float)(2.0 * aq / den_p);
      yu[at_y] = (float)(2.0 * au / den_p);
    }
  }
}

// the modulation's tile is mrx_tod_dev.h's.  This file is built WITH contraction: it takes the loads and stores only
constexpr int kModThreads = mrx_tod::kThreads;
constexpr int kOwn = mrx_tod::kOwn;
constexpr int kModTile = mrx_tod::kTileSamples;
using mrx_tod::load_own;
using mrx_tod::store_own;

enum : int { kWideI = 1, kWideC = 2, kWideS = 4, kWideOut = 8, kWideCarrier = 16 };

// out and vi may be the same buffer: a thread reads its samples before it writes them, and no other thread touches them
__global__ __launch_bounds__(kModThreads) void tod_hwp_modulate_kernel(const float* vi, const float* __restrict__ vc,
                                                                       const float* __restrict__ vs, size_t ld_in, int T,
                                                                       const double* __restrict__ carrier, float* out, size_t ld_out,
                                                                       int wide, int tiles_per_row, long long n_tiles) {
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / tiles_per_row;
    const int t = (int)(tile - row * tiles_per_row) * kModTile + kOwn * (int)threadIdx.x;
    if (t >= T) continue;
    float a[kOwn], b[kOwn], c[kOwn];
    load_own<kOwn>(vi + (size_t)row * ld_in, t, T, wide & kWideI, a);
    load_own<kOwn>(vc + (size_t)row * ld_in, t, T, wide & kWideC, b);
    load_own<kOwn>(vs + (size_t)row * ld_in, t, T, wide & kWideS, c);
    double cs[2 * kOwn];
    if ((wide & kWideCarrier) && t + kOwn <= T) {
#pragma unroll
      for (int k = 0; k < kOwn; ++k) {
        const double2 w = *reinterpret_cast<const double2*>(carrier + 2 * (size_t)(t + k));
        cs[2 * k] = w.x, cs[2 * k + 1] = w.y;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 2 * kOwn; ++k) cs[k] = t + k / 2 < T ? carrier[2 * (size_t)t + k] : 0.0;
    }
    float r[kOwn];
#pragma unroll
    for (int k = 0; k < kOwn; ++k) r[k] = (float)fma((double)c[k], cs[2 * k + 1], fma((double)b[k], cs[2 * k], (double)a[k]));
    store_own<kOwn>(out + (size_t)row * ld_out, t, T, wide & kWideOut, r);
  }
}

}  // namespace

extern "C" {

int mrx_tod_demodulate(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, int q, const double* d_carrier, const double* d_taps_t,
                       const double* d_taps_p, int n_taps, float* d_t, float* d_q, float* d_u, size_t ld_y) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_carrier && d_taps_p && d_q && d_u && (!d_t || d_taps_t), "null pointer");
  MRX_REQUIRE(ctx, q >= 2 && q <= kMaxFactor, "q must be in 2 .. 32");
  MRX_REQUIRE(ctx, n_taps >= 1 && n_taps <= kMaxTaps && (n_taps & 1), "n_taps must be odd and in 1 .. 1025");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  const long long T_out = ((long long)T + q - 1) / q;
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && ld_y >= (size_t)T_out, "ld_x smaller than T or ld_y smaller than T_out");
  MRX_REQUIRE(ctx, (const void*)d_t != (const void*)d_x && (const void*)d_q != (const void*)d_x && (const void*)d_u != (const void*)d_x,
              "no output may be d_x");
  MRX_REQUIRE(ctx, d_q != d_u && d_t != d_q && d_t != d_u, "d_t, d_q and d_u must differ");
  const int tiles_per_row = (int)((T_out + kTileOutputs - 1) / kTileOutputs);
  const long long n_tiles = (long long)D * tiles_per_row;
  const int P = (kTileOutputs - 1 + (n_taps + q - 1) / q) | 1;
  const size_t lds = (size_t)2 * kPrefixDoubles * sizeof(double) + (size_t)q * P * (2 * sizeof(double) + sizeof(float));
  // as many workgroups as stay resident (8 a CU at most, fewer where the windows are large); the rest of the tiles by stride
  const size_t lds_cu = ctx->lds_per_cu > 0 ? (size_t)ctx->lds_per_cu : 160 * 1024;
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, lds_cu / lds));
  const unsigned blocks = mrx_resident_blocks(ctx, n_tiles, per_cu);
  const unsigned q_magic = 0xFFFFFFFFu / (unsigned)q + 1u;  // floor(m q_magic / 2^32) = m / q for m < 2^32 / q
  if (d_t) {
    MRX_LDS_CAP(ctx, tod_demodulate_kernel<true>, lds);
    hipLaunchKernelGGL(tod_demodulate_kernel<true>, dim3(blocks), dim3(kThreads), lds, ctx->stream, d_x, ld_x, T, q, q_magic, d_carrier,
                       d_taps_t, d_taps_p, n_taps, d_t, d_q, d_u, ld_y, (int)T_out, P, tiles_per_row, n_tiles);
  } else {
    MRX_LDS_CAP(ctx, tod_demodulate_kernel<false>, lds);
    hipLaunchKernelGGL(tod_demodulate_kernel<false>, dim3(blocks), dim3(kThreads), lds, ctx->stream, d_x, ld_x, T, q, q_magic, d_carrier,
                       d_taps_t, d_taps_p, n_taps, d_t, d_q, d_u, ld_y, (int)T_out, P, tiles_per_row, n_tiles);
  }
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_hwp_modulate(mrx_ctx* ctx, const float* d_i, const float* d_c, const float* d_s, size_t ld_in, int D, int T,
                         const double* d_carrier, float* d_out, size_t ld_out) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_i && d_c && d_s && d_carrier && d_out, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, ld_in >= (size_t)T && ld_out >= (size_t)T, "ld_in or ld_out smaller than T");
  MRX_REQUIRE(ctx, (const void*)d_out != (const void*)d_c && (const void*)d_out != (const void*)d_s, "d_out must not be d_c or d_s");
  MRX_REQUIRE(ctx, d_out != d_i || ld_out == ld_in, "in place (d_out == d_i) needs ld_out == ld_in");
  const int wide = (mrx_aligned(d_i, ld_in * 4, 16) ? kWideI : 0) | (mrx_aligned(d_c, ld_in * 4, 16) ? kWideC : 0) |
                   (mrx_aligned(d_s, ld_in * 4, 16) ? kWideS : 0) | (mrx_aligned(d_out, ld_out * 4, 16) ? kWideOut : 0) |
                   (mrx_aligned(d_carrier, 0, 16) ? kWideCarrier : 0);
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, D, T, kModTile);
  hipLaunchKernelGGL(tod_hwp_modulate_kernel, dim3(g.blocks), dim3(kModThreads), 0, ctx->stream, d_i, d_c, d_s, ld_in, T, d_carrier, d_out, ld_out,
                     wide, g.tiles_per_row, g.n_tiles);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // extern "C"
