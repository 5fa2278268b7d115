// Band powers from the half-plane modes of two maps (maria_amd/bandpowers.py): mrx_map_band_powers.
// a1, a2 [3][ny][nx/2 + 1] complex128 hold T, Q, U in numpy.fft.rfft2's layout.  Per cell (iy, ix), fx = ix,
// fy = iy < ny/2 ? iy : iy - ny:
//   kx = 2 pi (fx / (nx res)),  ky = 2 pi (fy / (ny res)),  l2 = kx kx + ky ky
//   c = (kx kx - ky ky) / l2,   s = (2 kx ky) / l2,   E = Q c + U s,   B = -Q s + U c
//   XY = 0.5 (Re(a1_X conj a2_Y) + Re(a1_Y conj a2_X)),   w = fx == 0 ? 1 : 2
// kept when l2 > 0, fx < nx/2, |fy| < ny/2 and edges[0]^2 <= l2 < edges[n_bins]^2; bin b: edges[b]^2 <= l2 < edges[b+1]^2.
// The file is built without FMA contraction: every operation above is one float64 rounding, as in tests/bandpower_ref.py.
//
// No atomics, and an order of every sum that (ny, nx, edges) fix:
//   band_rows_kernel   one wave a row.  It walks the row in chunks of 64 cells, lane o the cell 64 c + o (one 16-byte
//                      load a plane: a wave reads 1 KiB runs).  Along a row l rises with fx, so the lanes of one bin are a
//                      run; the wave takes the chunk's bins in ascending order, each with the other lanes' values
//                      selected to 0.0, through one folded butterfly (reduce8: the eight columns halve at xor 32, 16, 8,
//                      then xor 4, 2, 1 -- 10 exchanges instead of 48; lane 8 k ends with column k), and adds the chunks
//                      of a bin in ascending order.  Lane 8 k stores column k of every (row, bin) partial exactly once,
//                      0.0 for a bin the row does not meet: the work buffer needs no clearing and its old contents
//                      (NaN included) are never read.  The bin edges' squares sit in LDS (<= 8200 bytes).
//   band_sum_kernel    one workgroup a bin.  Thread (q, k) adds column k over the rows of group q (32 groups of
//                      ceil(ny / 32) consecutive rows) in ascending order, thread k then the 32 groups in ascending order.
#include "mrx_internal.h"

#include <vector>

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kCols = 8;         // sum w, sum w l, TT, EE, BB, TE, TB, EB
constexpr int kMaxBins = 1024;
constexpr int kRowGroups = kThreads / kCols;
constexpr double kTwoPi = 6.283185307179586476925286766559;

struct BandArgs {
  const double2* a1;
  const double2* a2;
  int ny, nx, n_bins;
  double Lx, Ly;          // nx res, ny res
  const double* edges2;   // [n_bins + 1] device: the edges' squares
  double* part;           // [ny][n_bins][kCols]
};

// The 64 lanes' eight columns added: after the three halving steps a lane holds one column (lane >> 3) of its group of
// eight lanes, after the butterfly over xor 4, 2, 1 the column's sum over the wave.  The order is the same on every call.
__device__ __forceinline__ double reduce8(const double (&v)[kCols], int lane) {
  const bool h32 = (lane & 32) != 0, h16 = (lane & 16) != 0, h8 = (lane & 8) != 0;
  double a[4], b[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = (h32 ? v[j + 4] : v[j]) + __shfl_xor(h32 ? v[j] : v[j + 4], 32, kWave);
#pragma unroll
  for (int j = 0; j < 2; ++j) b[j] = (h16 ? a[j + 2] : a[j]) + __shfl_xor(h16 ? a[j] : a[j + 2], 16, kWave);
  double r = (h8 ? b[1] : b[0]) + __shfl_xor(h8 ? b[0] : b[1], 8, kWave);
  r = r + __shfl_xor(r, 4, kWave);
  r = r + __shfl_xor(r, 2, kWave);
  r = r + __shfl_xor(r, 1, kWave);
  return r;
}

// 0.5 (Re(x1 conj y2) + Re(y1 conj x2))
__device__ __forceinline__ double cross(double2 x1, double2 y1, double2 x2, double2 y2) {
  return 0.5 * ((x1.x * y2.x + x1.y * y2.y) + (y1.x * x2.x + y1.y * x2.y));
}

struct Teb {
  double2 t, e, b;
};
__device__ __forceinline__ Teb rotate(const double2* __restrict__ a, size_t plane, size_t at, double c, double s) {
  const double2 t = a[at], q = a[plane + at], u = a[2 * plane + at];
  Teb m;
  m.t = t;
  m.e = make_double2(q.x * c + u.x * s, q.y * c + u.y * s);
  m.b = make_double2(-q.x * s + u.x * c, -q.y * s + u.y * c);
  return m;
}

template <bool kCrossMaps>
__global__ __launch_bounds__(kThreads) void band_rows_kernel(BandArgs g) {
  __shared__ double s_e2[kMaxBins + 1];
  for (int i = threadIdx.x; i <= g.n_bins; i += kThreads) s_e2[i] = g.edges2[i];
  __syncthreads();  // the only barrier: a wave past the last row leaves after it
  const int lane = threadIdx.x & (kWave - 1);
  const int iy = blockIdx.x * kWaves + threadIdx.x / kWave;
  if (iy >= g.ny) return;
  const int half = g.nx / 2, nxh = half + 1, n_bins = g.n_bins;
  const int fy = iy < g.ny / 2 ? iy : iy - g.ny;
  const bool row_kept = iy != g.ny / 2;  // the Nyquist row
  const double ky = kTwoPi * ((double)fy / g.Ly);
  const double e2_lo = s_e2[0], e2_hi = s_e2[n_bins];
  const size_t plane = (size_t)g.ny * nxh;
  const size_t row_at = (size_t)iy * nxh;
  double* const part = g.part + (size_t)iy * n_bins * kCols + (lane >> 3);
  const bool writer = (lane & 7) == 0;

  int cur = -1, next = 0;  // the bin being added; the first bin of the row not stored yet (both the wave's)
  double acc = 0.0;
  auto flush = [&]() {
    if (writer) {
      for (int z = next; z < cur; ++z) part[(size_t)z * kCols] = 0.0;
      part[(size_t)cur * kCols] = acc;
    }
    next = cur + 1;
  };

  for (int x0 = 0; row_kept && x0 < half; x0 += kWave) {
    const int ix = x0 + lane;  // fx; the Nyquist column ix == half is never reached
    const double kx = kTwoPi * ((double)ix / g.Lx);
    const double l2 = kx * kx + ky * ky;
    int bin = -1;
    if (ix < half && l2 > 0.0 && l2 >= e2_lo && l2 < e2_hi) {
      int lo = 0, hi = n_bins;  // s_e2[lo] <= l2 < s_e2[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (l2 >= s_e2[mid]) lo = mid; else hi = mid;
      }
      bin = lo;
    }
    double val[kCols] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (bin >= 0) {
      const double c = (kx * kx - ky * ky) / l2, s = (2.0 * kx * ky) / l2;
      const double w = ix == 0 ? 1.0 : 2.0;
      const Teb m1 = rotate(g.a1, plane, row_at + ix, c, s);
      const Teb m2 = kCrossMaps ? rotate(g.a2, plane, row_at + ix, c, s) : m1;
      val[0] = w;
      val[1] = w * sqrt(l2);
      val[2] = w * cross(m1.t, m1.t, m2.t, m2.t);
      val[3] = w * cross(m1.e, m1.e, m2.e, m2.e);
      val[4] = w * cross(m1.b, m1.b, m2.b, m2.b);
      val[5] = w * cross(m1.t, m1.e, m2.t, m2.e);
      val[6] = w * cross(m1.t, m1.b, m2.t, m2.b);
      val[7] = w * cross(m1.e, m1.b, m2.e, m2.b);
    }
    unsigned long long todo = __ballot(bin >= 0);
    while (todo) {  // the chunk's bins, ascending: the first lane left holds the lowest
      const int b0 = __builtin_amdgcn_readfirstlane(__shfl(bin, __ffsll((long long)todo) - 1, kWave));
      const bool mine = bin == b0;
      todo &= ~__ballot(mine);
      double v[kCols];
#pragma unroll
      for (int k = 0; k < kCols; ++k) v[k] = mine ? val[k] : 0.0;
      const double r = reduce8(v, lane);
      if (b0 != cur) {
        if (cur >= 0) flush();
        cur = b0;
        acc = r;
      } else {
        acc = acc + r;
      }
    }
  }
  if (cur >= 0) flush();
  if (writer)
    for (int z = next; z < n_bins; ++z) part[(size_t)z * kCols] = 0.0;
}

__global__ __launch_bounds__(kThreads) void band_sum_kernel(const double* __restrict__ part, int ny, int n_bins, double* __restrict__ sums) {
  __shared__ double s_group[kRowGroups][kCols];
  const int b = blockIdx.x, k = threadIdx.x & (kCols - 1), q = threadIdx.x / kCols;
  const int rows = (ny + kRowGroups - 1) / kRowGroups;
  const int r0 = q * rows, r1 = min(ny, r0 + rows);
  const double* p = part + (size_t)b * kCols + k;
  double s = 0.0;
#pragma unroll 8
  for (int r = r0; r < r1; ++r) s = s + p[(size_t)r * n_bins * kCols];
  s_group[q][k] = s;
  __syncthreads();
  if (threadIdx.x < kCols) {
    double t = 0.0;
    for (int j = 0; j < kRowGroups; ++j) t = t + s_group[j][threadIdx.x];
    sums[(size_t)b * kCols + threadIdx.x] = t;
  }
}

bool sizes_ok(int ny, int nx, int n_bins) {
  return ny >= 8 && nx >= 8 && ny % 2 == 0 && nx % 2 == 0 && n_bins >= 1 && n_bins <= kMaxBins;
}

}  // namespace

extern "C" {

int mrx_band_power_work_bytes(int ny, int nx, int n_bins, size_t* bytes) {
  if (!bytes || !sizes_ok(ny, nx, n_bins)) return MRX_ERR_INVALID;
  // the edges' squares (padded to an even count: the partials stay 16-byte aligned), the [ny][n_bins][8] partials
  *bytes = sizeof(double) * ((size_t)((n_bins + 2) & ~1) + (size_t)ny * n_bins * kCols);
  return MRX_OK;
}

int mrx_map_band_powers(mrx_ctx* ctx, const double* d_a1, const double* d_a2, int ny, int nx, double res, const double* edges, int n_bins,
                        double* d_sums, void* d_work, size_t work_bytes) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_a1 && d_a2 && edges && d_sums && d_work, "null pointer");
  MRX_REQUIRE(ctx, ny >= 8 && nx >= 8 && ny % 2 == 0 && nx % 2 == 0, "ny and nx must be even and at least 8");
  MRX_REQUIRE(ctx, n_bins >= 1 && n_bins <= kMaxBins, "n_bins must be in 1 .. 1024");
  MRX_REQUIRE(ctx, res > 0, "the pixel size must be positive");  // false for a NaN too
  MRX_REQUIRE(ctx, edges[0] >= 0, "the bin edges must not be negative");
  for (int b = 0; b < n_bins; ++b) MRX_REQUIRE(ctx, edges[b + 1] > edges[b], "the bin edges must ascend");
  MRX_REQUIRE(ctx, edges[n_bins] < __builtin_inf(), "the bin edges must be finite");
  size_t need = 0;
  mrx_band_power_work_bytes(ny, nx, n_bins, &need);
  MRX_REQUIRE(ctx, work_bytes >= need, "work buffer smaller than mrx_band_power_work_bytes()");
  MRX_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(d_a1) | reinterpret_cast<uintptr_t>(d_a2) | reinterpret_cast<uintptr_t>(d_work)) & 15u) == 0,
              "d_a1, d_a2 and d_work must be 16-byte aligned");
  std::vector<double> e2((size_t)n_bins + 1);
  for (int b = 0; b <= n_bins; ++b) e2[b] = edges[b] * edges[b];
  double* const d_e2 = static_cast<double*>(d_work);
  MRX_HIP(ctx, hipMemcpyAsync(d_e2, e2.data(), sizeof(double) * e2.size(), hipMemcpyHostToDevice, ctx->stream));
  MRX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the host copy goes away with this call
  BandArgs g{};
  g.a1 = reinterpret_cast<const double2*>(d_a1);
  g.a2 = reinterpret_cast<const double2*>(d_a2);
  g.ny = ny, g.nx = nx, g.n_bins = n_bins;
  g.Lx = (double)nx * res, g.Ly = (double)ny * res;
  g.edges2 = d_e2;
  g.part = d_e2 + ((n_bins + 2) & ~1);
  const dim3 grid(mrx_ceil_div(ny, kWaves));
  if (d_a2 != d_a1)
    hipLaunchKernelGGL(band_rows_kernel<true>, grid, dim3(kThreads), 0, ctx->stream, g);
  else
    hipLaunchKernelGGL(band_rows_kernel<false>, grid, dim3(kThreads), 0, ctx->stream, g);
  MRX_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(band_sum_kernel, dim3(n_bins), dim3(kThreads), 0, ctx->stream, g.part, ny, n_bins, d_sums);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // extern "C"
