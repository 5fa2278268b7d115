// The anti-aliasing FIR decimator of a [D, T] TOD (maria_amd/downsample.py):
//   y[d][j] = ( sum_i h[H + i] x[d][j q + i] ) / ( sum_i h[H + i] ),   -H <= i <= H,  0 <= j q + i < T,
// a strided correlation whose taps outside the row are dropped and the rest renormalised.
//
// A workgroup takes kTileOutputs consecutive outputs of one row: thread o the output j0 + o.  It stages the
// W = (kTileOutputs - 1) q + n_taps samples from j0 q - H on in LDS, converted to float64 once (a sample is used by
// n_taps / q outputs) and zero outside [0, T), de-interleaved by phase: sample m of the window at (m mod q) P + m / q.
// Tap k = c q + r of output o then reads word r P + o + c: neighbouring lanes neighbouring words, no bank conflict at
// any q (read at stride q the window conflicts gcd(q, banks)-fold).  The tap's index is the same in every lane, so the
// taps are scalar loads and take no LDS bandwidth; per tap and wave that leaves one 8-byte LDS read and one float64 FMA.
// The sum runs over k ascending.  The denominator depends on j only: a prefix sum of the taps, built by the workgroup once
// in LDS, gives it as the difference of two entries.  Workgroups stride over the tiles (neighbours in the grid take
// neighbouring tiles of a row, the halo they share comes from L2), so the prefix sum is built once a workgroup.
#include "mrx_internal.h"

#include <algorithm>

namespace {

constexpr int kTileOutputs = 256;  // maria_amd.downsample.TILE_OUTPUTS
constexpr int kThreads = kTileOutputs;
constexpr int kMaxTaps = 1025;
constexpr int kMaxFactor = 32;
constexpr int kPrefixChunk = (kMaxTaps + kThreads - 1) / kThreads;  // taps a thread sums for the prefix
constexpr int kPrefixDoubles = kMaxTaps + 1;
constexpr int kStage = 8;  // window samples a thread loads before it writes them to LDS

__global__ __launch_bounds__(kThreads) void tod_decimate_kernel(const float* __restrict__ x, size_t ld_x, int T, int q, unsigned q_magic,
                                                                const double* __restrict__ taps, int n_taps, float* __restrict__ y,
                                                                size_t ld_y, int T_out, int tiles_per_row, long long n_tiles) {
  extern __shared__ double lds[];
  double* const pre = lds;                   // pre[i] = h[0] + .. + h[i - 1], i <= n_taps
  double* const win = lds + kPrefixDoubles;  // [q][P]
  double* const part = win;                  // the prefix sum's kThreads partial sums (q P >= 2 kThreads), before any window
  const int o = threadIdx.x;
  const int H = (n_taps - 1) / 2;
  const int P = kTileOutputs - 1 + (n_taps + q - 1) / q;
  const int W = (kTileOutputs - 1) * q + n_taps;

  {  // thread o sums its chunk of taps, adds the chunks before it, and writes its prefix entries
    const int k0 = o * kPrefixChunk;
    double s = 0.0;
    for (int i = 0; i < kPrefixChunk; ++i)
      if (k0 + i < n_taps) s += taps[k0 + i];
    part[o] = s;
    __syncthreads();
    double run = 0.0;
    for (int t = 0; t < o; ++t) run += part[t];
    if (o == 0) pre[0] = 0.0;
    for (int i = 0; i < kPrefixChunk; ++i) {
      if (k0 + i < n_taps) {
        run += taps[k0 + i];
        pre[k0 + i + 1] = run;
      }
    }
  }

  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / tiles_per_row;
    const int j0 = (int)(tile - row * tiles_per_row) * kTileOutputs;
    const float* const xr = x + (size_t)row * ld_x;
    const long long s0 = (long long)j0 * q - H;  // the window's first sample
    __syncthreads();                             // the previous tile's reads of the window (the first time: pre) are done
    for (int m0 = o; m0 < W; m0 += kStage * kThreads) {  // kStage loads in flight a thread
      float v[kStage];
#pragma unroll
      for (int u = 0; u < kStage; ++u)  // always a sample of the row: the loads do not branch
        v[u] = xr[min(max(s0 + m0 + u * kThreads, 0LL), (long long)T - 1)];
#pragma unroll
      for (int u = 0; u < kStage; ++u) {
        const int m = m0 + u * kThreads;
        const long long s = s0 + m;
        const int c = (int)__umulhi((unsigned)m, q_magic);  // m / q (m < 2^16)
        if (m < W) win[(m - c * q) * P + c] = (s >= 0 && s < T) ? (double)v[u] : 0.0;
      }
    }
    __syncthreads();
    const double* const wo = win + o;
    double acc = 0.0;
    for (int k = 0, r = 0, w = 0; k < n_taps; ++k) {  // tap k = c q + r: word w = r P + c (+ o)
      acc = fma(taps[k], wo[w], acc);
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
      const double den = pre[hi + 1] - pre[lo];
      y[(size_t)row * ld_y + j] = (float)(acc / den);
    }
  }
}

}  // namespace

extern "C" {

int mrx_tod_decimate(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, int q, const double* d_taps, int n_taps,
                     float* d_y, size_t ld_y) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_taps && d_y, "null pointer");
  MRX_REQUIRE(ctx, q >= 2 && q <= kMaxFactor, "q must be in 2 .. 32");
  MRX_REQUIRE(ctx, n_taps >= 1 && n_taps <= kMaxTaps && (n_taps & 1), "n_taps must be odd and in 1 .. 1025");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  const long long T_out = ((long long)T + q - 1) / q;
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && ld_y >= (size_t)T_out, "ld_x smaller than T or ld_y smaller than T_out");
  MRX_REQUIRE(ctx, (const void*)d_y != (const void*)d_x, "d_y must not be d_x");
  const int tiles_per_row = (int)((T_out + kTileOutputs - 1) / kTileOutputs);
  const long long n_tiles = (long long)D * tiles_per_row;
  const int P = kTileOutputs - 1 + (n_taps + q - 1) / q;
  const size_t lds = ((size_t)kPrefixDoubles + (size_t)q * P) * sizeof(double);
  MRX_LDS_CAP(ctx, tod_decimate_kernel, lds);
  // as many workgroups as stay resident (8 a CU at most, fewer where the window is large); the rest of the tiles by stride
  const size_t lds_cu = ctx->lds_per_cu > 0 ? (size_t)ctx->lds_per_cu : 160 * 1024;
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, lds_cu / lds));
  const unsigned blocks = mrx_resident_blocks(ctx, n_tiles, per_cu);
  const unsigned q_magic = 0xFFFFFFFFu / (unsigned)q + 1u;  // floor(m q_magic / 2^32) = m / q for m < 2^32 / q
  hipLaunchKernelGGL(tod_decimate_kernel, dim3(blocks), dim3(kThreads), lds, ctx->stream, d_x, ld_x, T, q, q_magic, d_taps, n_taps, d_y,
                     ld_y, (int)T_out, tiles_per_row, n_tiles);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // extern "C"
