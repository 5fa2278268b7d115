// The stationary inverse-noise filter of the correlated-noise GLS map (maria_amd/noise_filter.py):
//   y[d] = s ⊙ (k_d ⊛ (s ⊙ x[d])),
// the linear convolution of every row with a symmetric per-detector kernel of lags k_d[0..K], zero outside [0, T).
//
// Overlap-save with the in-LDS Stockham inverse transform of mrx_spectral.h, N = 4096 (K <= 512) or 8192 points: block b
// reads samples [b L - K, b L - K + N) and keeps the L = N - 2K outputs [b L, b L + L) that the circular product does not
// wrap into.  Two blocks of a row go through one complex transform, z = x_b + i x_{b+1}: the transfer function H (the DFT
// of the wrapped kernel) is real and even, so the real and imaginary parts of the result are the two filtered blocks.
// Only the inverse transform G is needed: with H even, G(H G z)[m] = N (k ⊛ z)[(-m) mod N], so the output is read
// index-reversed (H carries the 1 / N).
//
// One workgroup per row streams it along time.  A pair of blocks covers 2 L + 2 K samples; the 2 K it shares with the next
// pair stay in registers and the 2 L new ones are loaded during the previous pair's transforms, so each sample is read from
// HBM once and every load of a sample precedes the store that may overwrite it (outputs trail inputs by K): in place is
// safe.  H is built by the workgroup from the lags in a prologue transform and kept in registers (the transform's natural
// order gives each thread the same bins every time).
//
// The mode-aware GLS map (maria_amd/noise_modes.py) adds two pieces on the [D, T] TOD:
//   mrx_tod_noise_filter_modes: the filter of x[d] - sum_j U[d, j] b[j], a streaming subtraction (x read once, y written
//     once) followed by the filter in place.  The subtraction fused into the filter measured 2.7x the filter's
//     time at K = 2048, m = 10, the two passes 1.36x;
//   mrx_tod_mode_project: a[j, t] = sum_d U[d, j] x[d, t] in float64, a streaming reduction over the detectors.
#include "mrx_spectral.h"

#include <algorithm>
#include <climits>

namespace {

constexpr int kMaxLag = 2048;
constexpr int kMaxModes = 16;

__host__ __device__ constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }

template <int N>
struct NFilter {
  // N = 8192: 16 waves, the one workgroup a CU that 144 KiB of LDS admits, at <= 128 VGPRs (512 threads need 256 and spill);
  // N = 4096: 8 waves, two workgroups a CU, and every radix-8 butterfly of a pass has its thread
  static constexpr int kThreads = N == 8192 ? 1024 : 512;
  static constexpr int LOG2N = ilog2(N);
  static constexpr int EH = N / kThreads;      // bins of H a thread holds
  static constexpr int EX = 2 * N / kThreads;  // new samples of a pair a thread holds (2 L <= 2 N)
  // the transform's two images and the quarter twiddle table
  static constexpr size_t kLds = 2 * (size_t)N * 8 + (size_t)N / 4 * 8;
};

// x and y may be the same rows (in place): not restrict
template <int N>
__global__ __launch_bounds__(NFilter<N>::kThreads) void tod_noise_filter_kernel(const float* x, size_t ld_x, float* y, size_t ld_y, int T,
                                                                    const double* __restrict__ lags, int K,
                                                                    const float* __restrict__ sw, size_t ld_w) {
  using F = NFilter<N>;
  constexpr int kThreads = F::kThreads, EH = F::EH, EX = F::EX, LOG2N = F::LOG2N;
  extern __shared__ float2 lds[];
  float2* const img_a = lds;
  float2* const img_b = lds + N;
  float2* const tw = lds + 2 * N;
  const int t = threadIdx.x;
  const size_t d = blockIdx.x;
  const float* const xr = x + d * ld_x;
  float* const yr = y + d * ld_y;
  const float* const sr = sw ? sw + d * ld_w : nullptr;
  const double* const kr = lags + d * (size_t)(K + 1);
  const int L = N - 2 * K;  // outputs a block (>= 2 K: a pair's shared samples are among its new ones)
  const int n_pairs = (int)(((long long)T + 2 * L - 1) / (2 * L));
  mrx_dev::fill_twiddles<kThreads>(tw, N);

  // prologue: H = G(wrapped kernel) / N, real and even; thread t keeps bins i kThreads + t
  for (int j = t; j < N; j += kThreads) {
    const int a = j <= N / 2 ? j : N - j;
    img_a[j] = make_float2(a <= K ? (float)(kr[a] * (1.0 / N)) : 0.0f, 0.0f);
  }
  __syncthreads();
  float h[EH];
  {
    const float2* hr = mrx_dev::fft_lds_inverse<8, N, kThreads>(img_a, img_b, tw, N, LOG2N);
#pragma unroll
    for (int i = 0; i < EH; ++i) h[i] = hr[i * kThreads + t].x;
  }

  // pair p: U[u] = s x at sample 2 p L - K + u, u < 2 L + 2 K; z[j] = U[j] + i U[L + j].  Thread t holds the new samples
  // v = i kThreads + t < 2 L, counted from the pair's end (u = 2 K + 2 L - 1 - v), in nx: so the 2 K it shares with the
  // next pair are v < 2 K, the first KC slots of every thread, and are carried in cy.  The factor s is read when it is
  // applied, not ahead (a held copy spills at N = 8192; in the mapper it is one row shared by every detector, or none).
  constexpr int KC = (2 * (N == 8192 ? kMaxLag : 512) + kThreads - 1) / kThreads;
  float nx[EX], cy[KC];
  auto load_new = [&](int p) {
    const int s_end = 2 * p * L + K + 2 * L - 1;  // the sample at v = 0
#pragma unroll
    for (int i = 0; i < EX; ++i) {
      const int v = i * kThreads + t, s = s_end - v;
      nx[i] = (v < 2 * L && s < T) ? xr[s] : 0.0f;
    }
  };
  load_new(0);
  float* const z = reinterpret_cast<float*>(img_a);  // z[2 j] = Re, z[2 j + 1] = Im
  for (int p = 0; p < n_pairs; ++p) {
    __syncthreads();  // the previous pair's reads of its result are done
    if (p == 0) {     // U[0, 2 K): samples -K .. K - 1
      for (int c = t; c < 2 * K; c += kThreads) {
        const int s = c - K;
        z[2 * c] = (s >= 0 && s < T) ? xr[s] * (sr ? sr[s] : 1.0f) : 0.0f;
      }
    } else {  // the previous pair's U[2 L + c] = this pair's U[c], c = 2 K - 1 - v < 2 K (< L: only in the real part)
#pragma unroll
      for (int i = 0; i < KC; ++i) {
        const int v = i * kThreads + t;
        if (v < 2 * K) z[2 * (2 * K - 1 - v)] = cy[i];
      }
    }
    const int s_end = 2 * p * L + K + 2 * L - 1;
#pragma unroll
    for (int i = 0; i < EX; ++i) {
      const int v = i * kThreads + t;
      if (v < 2 * L) {
        const int u = 2 * K + 2 * L - 1 - v, s = s_end - v;
        const float val = (sr && s < T) ? nx[i] * sr[s] : nx[i];
        if (i < KC) cy[i] = val;
        if (u < N) z[2 * u] = val;
        if (u >= L) z[2 * (u - L) + 1] = val;
      }
    }
    // the next pair's new samples, in flight during the transforms (they lie past every output of this pair)
    if (p + 1 < n_pairs) load_new(p + 1);
    __syncthreads();
    float2* const r = mrx_dev::fft_lds_inverse<8, N, kThreads>(img_a, img_b, tw, N, LOG2N);
#pragma unroll
    for (int i = 0; i < EH; ++i) {
      const float2 v = r[i * kThreads + t];
      r[i * kThreads + t] = make_float2(v.x * h[i], v.y * h[i]);
    }
    __syncthreads();
    const float2* const res = mrx_dev::fft_lds_inverse<8, N, kThreads>(r, r == img_a ? img_b : img_a, tw, N, LOG2N);
    // outputs 2 p L + m: block 2 p (real part) for m < L, block 2 p + 1 (imaginary part) after; circular index m' + K
    const int o0 = 2 * p * L;
    for (int m = t; m < 2 * L; m += kThreads) {
      const int s = o0 + m;
      if (s >= T) break;
      const int second = m >= L;
      const int c = m - second * L + K;
      const float2 v = res[(N - c) & (N - 1)];
      const float o = second ? v.y : v.x;
      yr[s] = sr ? o * sr[s] : o;
    }
  }
}

template <int N>
int launch_noise_filter(mrx_ctx* ctx, const float* x, size_t ld_x, float* y, size_t ld_y, int D, int T, const double* lags, int K,
                        const float* sw, size_t ld_w) {
  MRX_LDS_CAP(ctx, tod_noise_filter_kernel<N>, NFilter<N>::kLds);
  hipLaunchKernelGGL(tod_noise_filter_kernel<N>, dim3((unsigned)D), dim3(NFilter<N>::kThreads), NFilter<N>::kLds, ctx->stream, x, ld_x, y, ld_y,
                     T, lags, K, sw, ld_w);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

// mrx_tod_mode_project: a workgroup takes kProjSamples samples of every row, its four waves a quarter of the rows each (row
// w, w + 4, ...), each lane two samples 64 apart (two 256-byte loads a row), with m float64 sums a sample in registers;
// the four partial sums of a sample meet in LDS.  T / 128 workgroups: 1875 at T = 240 000, about seven a CU.  The row of
// U a wave reads is uniform (scalar loads).
constexpr int kProjWaves = 4;
constexpr int kProjThreads = 64 * kProjWaves;
constexpr int kProjSamples = 128;
constexpr int kProjRows = 4;  // rows a wave has in flight

template <int MC>  // the sums a lane holds per sample: m <= MC
__global__ __launch_bounds__(kProjThreads) void tod_mode_project_kernel(const float* __restrict__ x, size_t ld_x, int D, int T,
                                                                        const double* __restrict__ U, int m, double* __restrict__ a) {
  __shared__ double part[kProjWaves][kProjSamples];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int t0 = blockIdx.x * kProjSamples;
  const int s0 = t0 + lane, s1 = t0 + 64 + lane;
  const bool ok0 = s0 < T, ok1 = s1 < T;
  double acc0[MC], acc1[MC];
#pragma unroll
  for (int j = 0; j < MC; ++j) acc0[j] = acc1[j] = 0.0;
  auto add_rows = [&](int d, int rows) {  // rows d, d + kProjWaves, ... (rows <= kProjRows, uniform)
    float v0[kProjRows], v1[kProjRows];
#pragma unroll
    for (int r = 0; r < kProjRows; ++r) {
      if (r < rows) {
        const float* const xr = x + (size_t)(d + r * kProjWaves) * ld_x;
        v0[r] = ok0 ? xr[s0] : 0.0f;
        v1[r] = ok1 ? xr[s1] : 0.0f;
      }
    }
#pragma unroll
    for (int r = 0; r < kProjRows; ++r) {
      if (r < rows) {
        const double* const ur = U + (size_t)(d + r * kProjWaves) * m;
        const double x0 = v0[r], x1 = v1[r];
#pragma unroll
        for (int j = 0; j < MC; ++j) {
          if (j < m) {
            const double u = ur[j];
            acc0[j] = fma(u, x0, acc0[j]);
            acc1[j] = fma(u, x1, acc1[j]);
          }
        }
      }
    }
  };
  int d = w;
  for (; d + (kProjRows - 1) * kProjWaves < D; d += kProjRows * kProjWaves) add_rows(d, kProjRows);
  if (d < D) add_rows(d, (D - 1 - d) / kProjWaves + 1);
#pragma unroll
  for (int j = 0; j < MC; ++j) {
    if (j < m) {
      part[w][lane] = acc0[j];
      part[w][64 + lane] = acc1[j];
      __syncthreads();
      if (threadIdx.x < kProjSamples) {
        const int s = t0 + threadIdx.x;
        double sum = 0.0;
#pragma unroll
        for (int q = 0; q < kProjWaves; ++q) sum += part[q][threadIdx.x];
        if (s < T) a[(size_t)j * T + s] = sum;
      }
      __syncthreads();
    }
  }
}

template <int MC>
int launch_mode_project(mrx_ctx* ctx, const float* x, size_t ld_x, int D, int T, const double* U, int m, double* a) {
  const unsigned blocks = (unsigned)(((long long)T + kProjSamples - 1) / kProjSamples);
  hipLaunchKernelGGL(tod_mode_project_kernel<MC>, dim3(blocks), dim3(kProjThreads), 0, ctx->stream, x, ld_x, D, T, U, m, a);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}


// mrx_tod_noise_filter_modes' first pass, y = x - U b: a workgroup takes 256 samples of kSubRows rows, each thread one
// sample with its m values of b in registers (read once for the rows), U's row uniform (scalar loads).  In place is safe:
// each element is read and then written by one thread.
constexpr int kSubThreads = 256;
constexpr int kSubRows = 32;

__global__ __launch_bounds__(kSubThreads) void tod_mode_subtract_kernel(const float* x, size_t ld_x, float* y, size_t ld_y, int D, int T,
                                                                        const double* __restrict__ U, int m, const float* __restrict__ b) {
  const int s = blockIdx.x * kSubThreads + threadIdx.x;
  if (s >= T) return;
  float bv[kMaxModes];
#pragma unroll
  for (int j = 0; j < kMaxModes; ++j) bv[j] = j < m ? b[(size_t)j * T + s] : 0.0f;
  for (int d0 = blockIdx.y * kSubRows; d0 < D; d0 += gridDim.y * kSubRows) {
    const int rows = min(kSubRows, D - d0);
    for (int r = 0; r < rows; ++r) {
      const size_t d = (size_t)(d0 + r);
      const double* const ur = U + d * m;
      float sub = 0.0f;
#pragma unroll
      for (int j = 0; j < kMaxModes; ++j)
        if (j < m) sub = fmaf((float)ur[j], bv[j], sub);
      y[d * ld_y + s] = x[d * ld_x + s] - sub;
    }
  }
}

}  // namespace

extern "C" {

int mrx_tod_noise_filter(mrx_ctx* ctx, const float* d_x, size_t ld_x, float* d_y, size_t ld_y, int D, int T,
                         const double* d_lags, int K, const float* d_sqrt_w, size_t ld_w) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_y && d_lags, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, T <= INT_MAX - 4 * 8192, "T too large for 32-bit sample indices");
  MRX_REQUIRE(ctx, K >= 0 && K <= kMaxLag, "K must be in 0 .. 2048");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && ld_y >= (size_t)T, "ld smaller than T");
  MRX_REQUIRE(ctx, d_x != d_y || ld_x == ld_y, "in place needs ld_y == ld_x");
  MRX_REQUIRE(ctx, !d_sqrt_w || ld_w == 0 || ld_w >= (size_t)T, "ld_w must be 0 or >= T");
  if (K <= 512) return launch_noise_filter<4096>(ctx, d_x, ld_x, d_y, ld_y, D, T, d_lags, K, d_sqrt_w, ld_w);
  return launch_noise_filter<8192>(ctx, d_x, ld_x, d_y, ld_y, D, T, d_lags, K, d_sqrt_w, ld_w);
}

int mrx_tod_noise_filter_modes(mrx_ctx* ctx, const float* d_x, size_t ld_x, float* d_y, size_t ld_y, int D, int T,
                               const double* d_lags, int K, const float* d_sqrt_w, size_t ld_w, const double* d_U, int m,
                               const float* d_b) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_y && d_lags, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, T <= INT_MAX - 4 * 8192, "T too large for 32-bit sample indices");
  MRX_REQUIRE(ctx, K >= 0 && K <= kMaxLag, "K must be in 0 .. 2048");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && ld_y >= (size_t)T, "ld smaller than T");
  MRX_REQUIRE(ctx, d_x != d_y || ld_x == ld_y, "in place needs ld_y == ld_x");
  MRX_REQUIRE(ctx, !d_sqrt_w || ld_w == 0 || ld_w >= (size_t)T, "ld_w must be 0 or >= T");
  MRX_REQUIRE(ctx, m >= 0 && m <= kMaxModes, "m must be in 0 .. 16");
  MRX_REQUIRE(ctx, m == 0 || (d_U && d_b), "null pointer");
  if (m == 0) return mrx_tod_noise_filter(ctx, d_x, ld_x, d_y, ld_y, D, T, d_lags, K, d_sqrt_w, ld_w);
  const unsigned row_groups = (unsigned)std::min((D + kSubRows - 1) / kSubRows, 65535);
  hipLaunchKernelGGL(tod_mode_subtract_kernel, dim3((unsigned)((T + kSubThreads - 1) / kSubThreads), row_groups), dim3(kSubThreads), 0,
                     ctx->stream, d_x, ld_x, d_y, ld_y, D, T, d_U, m, d_b);
  MRX_CHECK_LAUNCH(ctx);
  return mrx_tod_noise_filter(ctx, d_y, ld_y, d_y, ld_y, D, T, d_lags, K, d_sqrt_w, ld_w);
}

int mrx_tod_mode_project(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const double* d_U, int m, double* d_a) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_U && d_a, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, m >= 1 && m <= kMaxModes, "m must be in 1 .. 16");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T, "ld smaller than T");
  if (m <= 4) return launch_mode_project<4>(ctx, d_x, ld_x, D, T, d_U, m, d_a);
  if (m <= 8) return launch_mode_project<8>(ctx, d_x, ld_x, D, T, d_U, m, d_a);
  return launch_mode_project<16>(ctx, d_x, ld_x, D, T, d_U, m, d_a);
}


}  // extern "C"
