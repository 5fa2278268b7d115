// The destriper's prior on the baseline offsets: per detector d of a TOD with nb baselines, the weighted
// graph Laplacian T over its baselines (maria_amd/destripe_prior.py),
//   (T a)_b = sum_{k=1..K} w_k ( [b + k < nb] (a_b - a_{b+k}) + [b - k >= 0] (a_b - a_{b-k}) ),
// scaled by s_d.  Three float64 entry points, independent of the map:
//   mrx_baseline_prior_apply   y = hits a + s T a            a streaming stencil with a K-baseline halo in LDS
//   mrx_baseline_band_factor   LDL^T of diag(hits) + s T_Kp  one lane per detector, sequential along b, the active
//                                                            (Kp + 1) x (Kp + 1) window in LDS
//   mrx_baseline_band_solve    z = (diag(hits) + s T_Kp)^-1 r  one lane per detector, forward and back substitution
//                                                            with the band in registers
// The factor is stored by column, detector fastest: factor[(b (Kp + 1) + j) D + d] = L[b + j][b] for j >= 1 and 1 / D_b
// for j = 0, so that every step of a substitution reads Kp + 1 lines coalesced across the wave's 64 detectors.
#include "mrx_internal.h"

#include <vector>

namespace {

constexpr int kMaxLags = 64;   // K
constexpr int kMaxBand = 16;   // Kp
constexpr int kTile = 256;     // baselines a workgroup of the apply
constexpr int kLanes = 64;     // detectors a workgroup of the factor and the solve (one wave)

// y[d][b] = hits[d][b] a[d][b] + s_d (T a)[d][b]; one workgroup per (detector, tile of 256 baselines), the tile and its
// K-baseline halo on either side staged in LDS (zeros past the ends, never read: the masks leave those terms out)
__global__ __launch_bounds__(kTile) void prior_apply_kernel(int nb, int K, int tiles, const double* __restrict__ w,
                                                            const double* __restrict__ scale, const double* __restrict__ hits,
                                                            const double* __restrict__ a, double* __restrict__ y) {
  __shared__ double sa[kTile + 2 * kMaxLags];
  __shared__ double sw[kMaxLags];
  const int d = blockIdx.x / tiles;
  const int b0 = (blockIdx.x - d * tiles) * kTile;
  const double* row = a + (size_t)d * nb;
  for (int i = threadIdx.x; i < kTile + 2 * K; i += kTile) {
    const int b = b0 - K + i;
    sa[i] = (b >= 0 && b < nb) ? row[b] : 0.0;
  }
  if (threadIdx.x < K) sw[threadIdx.x] = w[threadIdx.x];
  __syncthreads();
  const int b = b0 + threadIdx.x;
  if (b >= nb) return;
  const double* c = sa + K + threadIdx.x;
  const double ab = c[0];
  double acc = 0.0;
  if (b >= K && b + K < nb) {  // every neighbour present (the interior)
    for (int k = 1; k <= K; ++k) acc = fma(sw[k - 1], (ab - c[k]) + (ab - c[-k]), acc);
  } else {
    for (int k = 1; k <= K; ++k) {
      const double t = (b + k < nb ? ab - c[k] : 0.0) + (b - k >= 0 ? ab - c[-k] : 0.0);
      acc = fma(sw[k - 1], t, acc);
    }
  }
  const size_t at = (size_t)d * nb + b;
  y[at] = fma(scale[d], acc, hits ? hits[at] * ab : 0.0);
}

// diag T_Kp at baseline p: the weights whose neighbour exists
__device__ __forceinline__ double laplacian_diagonal(const double* w, int Kp, int p, int nb) {
  double s = 0.0;
  for (int k = 1; k <= Kp; ++k) s += (p + k < nb ? w[k - 1] : 0.0) + (p - k >= 0 ? w[k - 1] : 0.0);
  return s;
}

// Banded LDL^T, right-looking: the window holds rows i .. i + Kp of the Schur complement, row p's upper band
// (p, p + j), j = 0 .. Kp, in ring slot p mod (Kp + 1); LDS layout [slot][j][lane] (lane-contiguous doubles: no bank
// conflicts).  Step i takes the pivot, writes column i and updates the rows below it; row i + Kp + 1 then enters, as A
// (no elimination has reached it yet), in row i's slot.
__global__ __launch_bounds__(kLanes) void band_factor_kernel(int D, int nb, int Kp, const double* __restrict__ w,
                                                            const double* __restrict__ scale, const double* __restrict__ hits,
                                                            double* __restrict__ factor, uint8_t* __restrict__ ok) {
  extern __shared__ double ring[];
  const int lane = threadIdx.x;
  const int d = blockIdx.x * kLanes + lane;
  if (d >= D) return;
  const int n = Kp + 1;
  const double s = Kp > 0 ? scale[d] : 0.0;
  const double* h = hits ? hits + (size_t)d * nb : nullptr;
  auto at = [&](int p, int j) -> double& { return ring[((p % n) * n + j) * kLanes + lane]; };
  auto enter = [&](int p) {
    at(p, 0) = (h ? h[p] : 0.0) + s * laplacian_diagonal(w, Kp, p, nb);
    for (int j = 1; j <= Kp; ++j) at(p, j) = p + j < nb ? -s * w[j - 1] : 0.0;
  };
  for (int p = 0; p < n && p < nb; ++p) enter(p);
  bool seen = false, good = true;
  const size_t step = (size_t)n * D;
  for (int i = 0; i < nb; ++i) {
    seen = seen || (h && h[i] > 0.0);
    const double piv = at(i, 0);
    if (!(piv > 0.0)) {
      good = false;
      break;
    }
    const double inv = 1.0 / piv;
    double* col = factor + (size_t)i * step + d;
    col[0] = inv;
    for (int r = 1; r <= Kp; ++r) {
      const double u = at(i, r);  // (p, p + r) of the window; 0 past the end
      col[(size_t)r * D] = u * inv;
      const double l = u * inv;
      for (int c = r; c <= Kp; ++c) at(i + r, c - r) -= l * at(i, c);
    }
    if (i + n < nb) enter(i + n);
  }
  ok[d] = (good && seen) ? 1 : 0;
}

// z = L^-T D^-1 L^-1 r for the detectors with ok = 1, else 0.  Forward: y_i = r_i - (pending sum of row i); column i
// then adds L[i + j][i] y_i to the pending sums of rows i + 1 .. i + Kp (registers, shifted each step).  Back:
// x_i = y_i / D_i - sum_j L[i + j][i] x_{i+j}, with the last Kp x in registers.  d_z may be d_r.
template <int KP>
__global__ __launch_bounds__(kLanes) void band_solve_kernel(int D, int nb, const double* __restrict__ factor,
                                                           const uint8_t* __restrict__ ok, const double* r, double* z) {
  const int d = blockIdx.x * kLanes + threadIdx.x;
  if (d >= D) return;
  const double* rr = r + (size_t)d * nb;
  double* zz = z + (size_t)d * nb;
  if (!ok[d]) {
    for (int i = 0; i < nb; ++i) zz[i] = 0.0;
    return;
  }
  const size_t step = (size_t)(KP + 1) * D;
  double pend[KP + 1];
#pragma unroll
  for (int j = 0; j <= KP; ++j) pend[j] = 0.0;
  for (int i = 0; i < nb; ++i) {
    const double* col = factor + (size_t)i * step + d;
    const double y = rr[i] - pend[0];
#pragma unroll
    for (int j = 0; j < KP; ++j) pend[j] = fma(col[(size_t)(j + 1) * D], y, pend[j + 1]);
    zz[i] = y * col[0];
  }
  double next[KP + 1];  // next[j]: x_{i + 1 + j}
#pragma unroll
  for (int j = 0; j <= KP; ++j) next[j] = 0.0;
  for (int i = nb - 1; i >= 0; --i) {
    const double* col = factor + (size_t)i * step + d;
    double x = zz[i];
#pragma unroll
    for (int j = 0; j < KP; ++j) x = fma(-col[(size_t)(j + 1) * D], next[j], x);
#pragma unroll
    for (int j = KP; j > 0; --j) next[j] = next[j - 1];
    next[0] = x;
    zz[i] = x;
  }
}

// scales >= 0 (NaN refused): one copy of D doubles to the host
int check_scales(mrx_ctx* ctx, int D, const double* d_scale) {
  std::vector<double> s((size_t)D);
  MRX_HIP(ctx, hipMemcpyAsync(s.data(), d_scale, (size_t)D * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  MRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < D; ++i)
    if (!(s[i] >= 0.0)) return mrx_fail(ctx, MRX_ERR_INVALID, "scale of detector %d is %g: must be >= 0", i, s[i]);
  return MRX_OK;
}

template <int KP>
void launch_solve(mrx_ctx* ctx, int D, int nb, const double* f, const uint8_t* ok, const double* r, double* z) {
  hipLaunchKernelGGL(band_solve_kernel<KP>, dim3(mrx_ceil_div(D, kLanes)), dim3(kLanes), 0, ctx->stream, D, nb, f, ok, r, z);
}

}  // namespace

extern "C" {

int mrx_baseline_prior_apply(mrx_ctx* ctx, int D, int nb, int K, const double* d_w, const double* d_scale,
                             const double* d_hits, const double* d_a, double* d_y) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  if (K < 1 || K > kMaxLags) return mrx_fail(ctx, MRX_ERR_INVALID, "K = %d lags: 1 .. %d", K, kMaxLags);
  MRX_REQUIRE(ctx, D >= 0 && nb >= 1, "need D >= 0 and nb >= 1");
  if (D == 0) return MRX_OK;
  MRX_REQUIRE(ctx, d_w && d_scale && d_a && d_y, "null pointer");
  MRX_REQUIRE(ctx, d_y != d_a, "d_y must not be d_a");
  const long long tiles = (nb + kTile - 1) / kTile;
  MRX_REQUIRE(ctx, (long long)D * tiles < (1LL << 31), "too many baselines for one launch");
  int rc = check_scales(ctx, D, d_scale);
  if (rc != MRX_OK) return rc;
  hipLaunchKernelGGL(prior_apply_kernel, dim3((unsigned)(D * tiles)), dim3(kTile), 0, ctx->stream, nb, K, (int)tiles, d_w, d_scale,
                     d_hits, d_a, d_y);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_baseline_band_factor(mrx_ctx* ctx, int D, int nb, int Kp, const double* d_w, const double* d_scale,
                             const double* d_hits, double* d_factor, uint8_t* d_ok) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  if (Kp < 0 || Kp > kMaxBand) return mrx_fail(ctx, MRX_ERR_INVALID, "Kp = %d: 0 .. %d", Kp, kMaxBand);
  MRX_REQUIRE(ctx, D >= 0 && nb >= 1, "need D >= 0 and nb >= 1");
  if (D == 0) return MRX_OK;
  MRX_REQUIRE(ctx, d_factor && d_ok && (Kp == 0 || (d_w && d_scale)), "null pointer");
  if (d_scale) {
    int rc = check_scales(ctx, D, d_scale);
    if (rc != MRX_OK) return rc;
  }
  const size_t lds = (size_t)(Kp + 1) * (Kp + 1) * kLanes * sizeof(double);
  MRX_LDS_CAP(ctx, band_factor_kernel, lds);
  hipLaunchKernelGGL(band_factor_kernel, dim3(mrx_ceil_div(D, kLanes)), dim3(kLanes), lds, ctx->stream, D, nb, Kp, d_w, d_scale,
                     d_hits, d_factor, d_ok);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_baseline_band_solve(mrx_ctx* ctx, int D, int nb, int Kp, const double* d_factor, const uint8_t* d_ok,
                            const double* d_r, double* d_z) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  if (Kp < 0 || Kp > kMaxBand) return mrx_fail(ctx, MRX_ERR_INVALID, "Kp = %d: 0 .. %d", Kp, kMaxBand);
  MRX_REQUIRE(ctx, D >= 0 && nb >= 1, "need D >= 0 and nb >= 1");
  if (D == 0) return MRX_OK;
  MRX_REQUIRE(ctx, d_factor && d_ok && d_r && d_z, "null pointer");
  switch (Kp) {
#define MRX_SOLVE_CASE(k) \
  case k:                 \
    launch_solve<k>(ctx, D, nb, d_factor, d_ok, d_r, d_z); \
    break;
    MRX_SOLVE_CASE(0) MRX_SOLVE_CASE(1) MRX_SOLVE_CASE(2) MRX_SOLVE_CASE(3) MRX_SOLVE_CASE(4) MRX_SOLVE_CASE(5)
    MRX_SOLVE_CASE(6) MRX_SOLVE_CASE(7) MRX_SOLVE_CASE(8) MRX_SOLVE_CASE(9) MRX_SOLVE_CASE(10) MRX_SOLVE_CASE(11)
    MRX_SOLVE_CASE(12) MRX_SOLVE_CASE(13) MRX_SOLVE_CASE(14) MRX_SOLVE_CASE(15) MRX_SOLVE_CASE(16)
#undef MRX_SOLVE_CASE
  }
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // extern "C"
