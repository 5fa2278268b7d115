// The Welch spectrum of every TOD row (maria_amd/noise_estimate.py::welch): scipy.signal.welch's defaults --
// periodic Hann window, half-segment overlap, each segment's mean removed, one-sided density, mean over segments.
//
// One workgroup per row streams the row once.  Two real segments are transformed as one complex sequence
// z = w (s1 - mean s1) + i w (s2 - mean s2); per bin the workgroup sums A_k = sum |Z_k|^2 over the pairs and combines once
// at the end, (A_k + A_{n-k}) / 2 = sum |X_k|^2 over the segments (an unpaired last segment has imaginary part 0).  The
// combine is symmetric in k, so the inverse Stockham passes of mrx_spectral.h serve as they are.
//
// Segment 2p starts at sample 2p h (h = n / 2), so pair p covers samples [2p h, 2p h + 3h) and its last half is the first
// half of pair p + 1.  A batch of G pairs (G n = C >= 2048 values: short segments are transformed G side by side,
// interleaved) reads the C samples after that shared half; the threads keep the half the next batch needs in registers
// (each thread always holds the same positions), so every sample is read from HBM once.  Segment means are summed in
// float64 per half segment (wave sums, then in a fixed order: reproducible bits).
#include "mrx_spectral.h"

#include <cmath>

namespace {

using mrx_dev::kBlock;

constexpr int kMinSeg = 256, kMaxSeg = 8192;
constexpr int kBatch = 2048;  // complex values a batch transforms at least

__host__ __device__ constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }

template <int N>
struct Welch {
  static constexpr int G = N >= kBatch ? 1 : kBatch / N;  // pairs a batch
  static constexpr int C = G * N;                         // new samples a batch = complex values of its transform
  static constexpr int E = C / kBlock;                    // of them a thread's
  static constexpr int H = N / 2;
  static constexpr int LJ = ilog2(G);
  static constexpr int LOG2N = ilog2(N);
  // two images of C float2 (the transform's ping-pong), the quarter twiddle table, the 64-sample sums, the half sums
  static constexpr size_t kLds = 2 * (size_t)C * 8 + (size_t)N / 4 * 8 + (size_t)C / 64 * 8 + (size_t)(2 * G + 1) * 8;
};

// psd[row][k] = norm (A_k + A_{N-k}) f_k, f_k = 1/2 at k = 0 and N/2 (one-sided), norm = 1 / (fs sum w^2 nseg)
template <int N>
__global__ __launch_bounds__(kBlock) void tod_welch_kernel(const float* __restrict__ x, size_t ld, int nseg, double norm,
                                                           float* __restrict__ psd) {
  using W = Welch<N>;
  constexpr int G = W::G, C = W::C, E = W::E, H = W::H, LJ = W::LJ, LOG2N = W::LOG2N;
  extern __shared__ float2 lds[];
  float2* const img_a = lds;
  float2* const img_b = lds + C;
  float2* const tw = lds + 2 * C;
  double* const part = reinterpret_cast<double*>(tw + N / 4);  // [C / 64]: sums of 64 consecutive new samples
  double* const hsum = part + C / 64;                          // [2G + 1]: the carried half, then the batch's 2G halves
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* const row = x + (size_t)blockIdx.x * ld;
  const long long s_end = (long long)(nseg - 1) * H + N;  // samples past the last segment are never read
  const int n_batches = ((nseg + 1) / 2 + G - 1) / G;
  mrx_dev::fill_twiddles<kBlock>(tw, N);

  // thread t holds new samples j = i kBlock + t of every batch: in segment 2 of pair j / N at j mod N, in segment 1 of
  // pair (j + H) / N at (j + H) mod N (pair G: segment 1 of the next batch's pair 0, carried in cy)
  float xv[E], cy[E];
  double acc[E];
#pragma unroll
  for (int i = 0; i < E; ++i) {
    cy[i] = 0.0f;
    acc[i] = 0.0;
  }
  // the periodic Hann window 1/2 - cos(2 pi k / N) / 2 from the twiddle table (float32, within an ulp of scipy's
  // float64 window rounded to float32; a table in registers spills at N = 8192)
  auto hann = [&](int k) { return 0.5f - 0.5f * mrx_dev::tw_at(tw, k, N / 4).x; };
  float* const z = reinterpret_cast<float*>(img_a);  // z[2 e] = Re, z[2 e + 1] = Im of element e = (k << LJ) | g
  // batch -1 only loads the first half segment (the carry of batch 0)
  for (int b = -1; b < n_batches; ++b) {
    const long long s0 = (long long)b * C + H;
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const long long s = s0 + i * kBlock + t;
      xv[i] = (s >= 0 && s < s_end) ? row[s] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < E; ++i) {
      double v = (double)xv[i];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) part[i * (kBlock / 64) + wave] = v;
    }
    __syncthreads();
    if (t < 2 * G) {
      double s = 0.0;
      for (int q = t * (H / 64); q < (t + 1) * (H / 64); ++q) s += part[q];
      hsum[1 + t] = s;
    }
    __syncthreads();
    if (b >= 0) {
      constexpr double inv_n = 1.0 / (double)N;
#pragma unroll
      for (int i = 0; i < E; ++i) {
        const int j = i * kBlock + t;
        const int g2 = j >> LOG2N, k2 = j & (N - 1);
        const bool ok2 = 2 * (b * G + g2) + 1 < nseg;
        const double m2 = (hsum[2 * g2 + 1] + hsum[2 * g2 + 2]) * inv_n;
        z[2 * ((k2 << LJ) | g2) + 1] = ok2 ? hann(k2) * (float)((double)xv[i] - m2) : 0.0f;
        const int j1 = j + H, g1 = j1 >> LOG2N, k1 = j1 & (N - 1);
        if (g1 < G) {
          const bool ok1 = 2 * (b * G + g1) < nseg;
          const double m1 = (hsum[2 * g1] + hsum[2 * g1 + 1]) * inv_n;
          z[2 * ((k1 << LJ) | g1)] = ok1 ? hann(k1) * (float)((double)xv[i] - m1) : 0.0f;
        } else {  // the previous batch's sample at this position: segment 1 of pair 0 (which exists: b < n_batches)
          const double m1 = (hsum[0] + hsum[1]) * inv_n;
          z[2 * (k1 << LJ)] = hann(k1) * (float)((double)cy[i] - m1);
        }
      }
      __syncthreads();
      const float2* res = mrx_dev::fft_lds_inverse_batched<8, (G == 1 ? N : 0), kBlock>(img_a, img_b, tw, N, LOG2N, LJ);
#pragma unroll
      for (int i = 0; i < E; ++i) {
        const float2 v = res[i * kBlock + t];
        acc[i] += (double)__builtin_fmaf(v.x, v.x, v.y * v.y);
      }
    }
#pragma unroll
    for (int i = 0; i < E; ++i)
      if (i * kBlock + t + H >= C) cy[i] = xv[i];
    // every read of hsum[0] of this batch preceded a barrier this thread has passed
    if (t == 0) hsum[0] = hsum[2 * G];
  }
  __syncthreads();
  double* const A = reinterpret_cast<double*>(img_a);  // C doubles: one image
#pragma unroll
  for (int i = 0; i < E; ++i) A[i * kBlock + t] = acc[i];
  __syncthreads();
  float* const out = psd + (size_t)blockIdx.x * (N / 2 + 1);
  for (int k = t; k <= N / 2; k += kBlock) {
    const int kk = (N - k) & (N - 1);
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < G; ++g) s += A[(k << LJ) | g] + A[(kk << LJ) | g];
    out[k] = (float)(s * norm * ((k == 0 || k == N / 2) ? 0.5 : 1.0));
  }
}

template <int N>
int launch_welch(mrx_ctx* ctx, const float* x, size_t ld, int D, int nseg, double norm, float* psd) {
  MRX_LDS_CAP(ctx, tod_welch_kernel<N>, Welch<N>::kLds);
  hipLaunchKernelGGL(tod_welch_kernel<N>, dim3((unsigned)D), dim3(kBlock), Welch<N>::kLds, ctx->stream, x, ld, nseg, norm, psd);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // namespace

extern "C" {

int mrx_tod_welch(mrx_ctx* ctx, const float* d_x, size_t ld, int D, int T, int nperseg, double fs, float* d_psd) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_psd, "null pointer");
  MRX_REQUIRE(ctx, D >= 1, "need D >= 1 rows");
  if (nperseg < kMinSeg || nperseg > kMaxSeg || (nperseg & (nperseg - 1)))
    return mrx_fail(ctx, MRX_ERR_UNSUPPORTED, "mrx_tod_welch: nperseg %d: a power of two in %d .. %d", nperseg, kMinSeg, kMaxSeg);
  MRX_REQUIRE(ctx, T >= nperseg, "T < nperseg: not one segment");
  MRX_REQUIRE(ctx, ld >= (size_t)T, "ld smaller than T");
  MRX_REQUIRE(ctx, fs > 0.0 && std::isfinite(fs), "fs must be finite and > 0");
  // scipy's density scale 1 / (fs sum w^2) of the float32 window, over the segment count
  double sw2 = 0.0;
  for (int k = 0; k < nperseg; ++k) {
    const double w = (double)(float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)k / (double)nperseg));
    sw2 += w * w;
  }
  const int nseg = (T - nperseg) / (nperseg / 2) + 1;
  const double norm = 1.0 / (fs * sw2 * (double)nseg);
  switch (nperseg) {
    case 256: return launch_welch<256>(ctx, d_x, ld, D, nseg, norm, d_psd);
    case 512: return launch_welch<512>(ctx, d_x, ld, D, nseg, norm, d_psd);
    case 1024: return launch_welch<1024>(ctx, d_x, ld, D, nseg, norm, d_psd);
    case 2048: return launch_welch<2048>(ctx, d_x, ld, D, nseg, norm, d_psd);
    case 4096: return launch_welch<4096>(ctx, d_x, ld, D, nseg, norm, d_psd);
    default: return launch_welch<8192>(ctx, d_x, ld, D, nseg, norm, d_psd);
  }
}

}  // extern "C"
