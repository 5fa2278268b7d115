// The beam fit's two device entries (maria_amd/beamfit.py): the per-sample source mask and the Gauss-Newton
// sums of a Gaussian beam model per detector.  Both need a detector sample's offsets (ox, oy) from a frame's centre exactly
// as the binning computes them: the code is the binning's own (mrx_map_pointing.h: sample_const, make_det_const,
// sample_offsets<false, false>, composed pointing only), built with mrx_map.hip's flags.
//
// mrx_tod_source_flag.  One streaming pass in the TOD tile (mrx_tile.h): a workgroup takes 16 rows x 1024 samples, a thread
// four consecutive samples whose SampleConst (float64 trigonometry) it computes once for the 16 rows.  Per row it forms
//   u = (double)ox - (double)src_x(t),  v = (double)oy - (double)src_y(t),  d2 = u u + v v
// and sets the sample's flag where d2 <= radius^2 (inside) or d2 > radius^2 (outside); a thread writes only where it has
// set a bit (one 4-byte access where pointer and pitch allow it, bytes otherwise).
//
// mrx_tod_beam_normal.  A workgroup takes 16 rows x one chunk of kChunkTiles tiles and walks the chunk tile by tile.  Per
// tile a thread first reads its four flags of every row; a wave none of whose samples is kept in any row goes on to the
// next tile (no pointing, no float64).  Otherwise, per row with a kept sample in the wave, it forms the sums of the lane's
// kept samples with the sample's rotation G (SampleConst::G, made once per call for all rows by sample_const in a kernel of
// its own: [T][6] float32 in d_work) (a flagged sample's value is never read), which the 64 lanes add in
// wave_sum_all (mrx_tod_dev.h); lane 0 then adds them to the wave's own LDS slot of the row.  At the chunk's end the four waves' slots
// are added in wave order and stored to d_work[row][chunk]; a second kernel adds a row's chunks in ascending order.  A
// skipped wave or row would have added +0.0 to every sum: the order is a function of (D, T) alone, there are no atomics,
// and the same inputs give the same bits on every call.
#include "mrx_map_pointing.h"
#include "mrx_tod_dev.h"

#include <algorithm>

namespace {

using mrx_tod::kWave;
constexpr int kWaves = kBlock / kWave;
constexpr int kChunkTiles = 16;  // 16384 samples a chunk: 15 chunks a row at T = 240 000, 44 MB of partial sums at D = 10 000, K = 7

constexpr int beam_sums(int K) { return 1 + K * (K + 1) / 2 + K; }  // chi2, the upper triangle of JtJ, Jtr

struct BeamArgs {
  const float* x;
  size_t ld_x;
  const float* model;
  size_t ld_m;
  const unsigned char* flags;
  size_t ld_f;
  int wide_f;          // flags and pitch are multiples of 4 bytes
  const float* src;    // [T][2] or null
  const float* rot;    // [T][6]: SampleConst::G of every sample (beam_rotation_kernel)
  const double* param;  // [D][K]
  double* work;        // [D][n_chunks][beam_sums(K) + 1]
  int n_chunks;
};

// The thread's four flags of one row as a word, byte q nonzero where sample sb + q is flagged or past the row's end.
// at: the row's flags + sb, or null (nothing flagged).  The pointer is the thread's own and advances by the pitch from row
// to row: a row's base as a scalar per unrolled row would be held in scalar registers across the whole kernel.
__device__ __forceinline__ uint32_t flag_word(const unsigned char* at, int wide, int sb, int T) {
  uint32_t w = 0u;
  if (at) {
    if (wide && sb + kSamplesPerThread <= T) {
      w = *reinterpret_cast<const uint32_t*>(at);
    } else {
#pragma unroll
      for (int q = 0; q < kSamplesPerThread; ++q) w |= at[min(sb + q, T - 1) - sb] != 0 ? 0xffu << (8 * q) : 0u;  // (clamped: masked below)
    }
  }
#pragma unroll
  for (int q = 0; q < kSamplesPerThread; ++q) w |= sb + q >= T ? 0xffu << (8 * q) : 0u;
  return w;
}

// the word's bytes that are zero, as a 4-bit mask
__device__ __forceinline__ unsigned kept_mask(uint32_t w) {
  unsigned k = 0u;
#pragma unroll
  for (int q = 0; q < kSamplesPerThread; ++q) k |= ((w >> (8 * q)) & 0xffu) == 0u ? 1u << q : 0u;
  return k;
}

// d c / d dx and d c / d dy of the detector's unit vector c = (-dy s, cos r, -dx s), s = sin r / r, in float64 at the
// float32 offsets the row's DetConst was made from: with h = (cos r - s) / r^2
//   dc/ddx = (-dx dy h, -dx s, -s - dx^2 h),   dc/ddy = (-s - dy^2 h, -dy s, -dx dy h)
struct DetJac {
  double cx[3], cy[3];
};

__device__ __forceinline__ DetJac make_det_jac(const DetConst& dc, float dxf, float dyf) {
  const double dx = (double)dxf, dy = (double)dyf;
  const double r2 = dx * dx + dy * dy;
  double s, h;
  if (r2 < 0.09) {  // the threshold of make_det_const: the series, exact to float64 rounding there
    s = 1.0 + r2 * (-1.0 / 6.0 + r2 * (1.0 / 120.0 + r2 * (-1.0 / 5040.0 + r2 * (1.0 / 362880.0 + r2 * (-1.0 / 39916800.0)))));
    h = -1.0 / 3.0 + r2 * (1.0 / 30.0 + r2 * (-1.0 / 840.0 + r2 * (1.0 / 45360.0 + r2 * (-1.0 / 3991680.0))));
  } else {  // beyond it from the row's own float32 constants: c_cr = cos r, (c_re, c_im) = (-dy s, -dx s)
    s = fabs(dx) > fabs(dy) ? -(double)dc.c_im / dx : -(double)dc.c_re / dy;
    h = ((double)dc.c_cr - s) / r2;
  }
  DetJac j;
  j.cx[0] = -dx * dy * h;
  j.cx[1] = -dx * s;
  j.cx[2] = -s - dx * dx * h;
  j.cy[0] = -s - dy * dy * h;
  j.cy[1] = -dy * s;
  j.cy[2] = -dx * dy * h;
  return j;
}

// the per-sample constants of the thread's four samples, with the clamped sample index as MapTile sets it
__device__ __forceinline__ void tile_samples(const MapArgs& g, int sb, SampleConst (&sc)[kSamplesPerThread]) {
#pragma unroll
  for (int q = 0; q < kSamplesPerThread; ++q) {
    sample_const(g, sb + q, false, sc[q]);
    sc[q].s = min(max(sb + q, 0), g.T - 1);
  }
}

__global__ __launch_bounds__(kBlock) void source_flag_kernel(MapArgs g, const float* __restrict__ src, double radius2, int inside, unsigned value,
                                                             unsigned char* flags, size_t ld_f, int wide) {
  __shared__ DetConst dets[kTileDet];
  const int d0 = blockIdx.y * kTileDet;
  const int nd = min(kTileDet, g.D - d0);
  const int sb = blockIdx.x * kTileSamples + threadIdx.x * kSamplesPerThread;
  if ((int)threadIdx.x < nd) dets[threadIdx.x] = make_det_const(g, d0 + threadIdx.x);
  SampleConst sc[kSamplesPerThread];
  tile_samples(g, sb, sc);
  __syncthreads();
  if (sb >= g.T) return;
  double sx[kSamplesPerThread], sy[kSamplesPerThread];
#pragma unroll
  for (int q = 0; q < kSamplesPerThread; ++q) {
    sx[q] = src ? (double)src[2 * (size_t)sc[q].s] : 0.0;
    sy[q] = src ? (double)src[2 * (size_t)sc[q].s + 1] : 0.0;
  }
  for (int dl = 0; dl < nd; ++dl) {
    const DetConst dc = dets[dl];
    unsigned char* const row = flags + (size_t)(d0 + dl) * ld_f;
    uint32_t w = 0u;
#pragma unroll
    for (int q = 0; q < kSamplesPerThread; ++q) {
      float ox, oy, el_d;
      sample_offsets<false, false>(g, dc, sc[q], ox, oy, el_d);
      const double u = (double)ox - sx[q], v = (double)oy - sy[q];
      const double d2 = u * u + v * v;
      const bool set = sb + q < g.T && (inside ? d2 <= radius2 : d2 > radius2);
      w |= set ? value << (8 * q) : 0u;
    }
    if (w == 0u) continue;
    if (wide && sb + kSamplesPerThread <= g.T) {
      uint32_t* const at = reinterpret_cast<uint32_t*>(row + sb);
      *at = *at | w;
    } else {
#pragma unroll
      for (int q = 0; q < kSamplesPerThread; ++q) {
        const unsigned b = (w >> (8 * q)) & 0xffu;
        if (b) row[sb + q] = (unsigned char)(row[sb + q] | b);  // b != 0 only where sb + q < T
      }
    }
  }
}

// SampleConst::G of every sample, once per call for all rows: the float64 trigonometry of sample_const is then no part of
// the sums' kernel (which would repeat it per group of 16 rows)
__global__ __launch_bounds__(kBlock) void beam_rotation_kernel(MapArgs g, float* __restrict__ rot) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= g.T) return;
  SampleConst sc;
  sample_const(g, s, false, sc);
#pragma unroll
  for (int j = 0; j < 6; ++j) rot[6 * (size_t)s + j] = sc.G[j];
}

// the trial offsets of every row, rounded to float32: what make_det_const reads in place of d_dx, d_dy
__global__ __launch_bounds__(kBlock) void beam_trial_kernel(const double* __restrict__ param, int K, int D, float* __restrict__ tdx,
                                                            float* __restrict__ tdy) {
  const int d = blockIdx.x * kBlock + threadIdx.x;
  if (d >= D) return;
  tdx[d] = (float)param[(size_t)d * K + 1];
  tdy[d] = (float)param[(size_t)d * K + 2];
}

template <int K, bool kModel>
__global__ __launch_bounds__(kBlock) void beam_normal_kernel(MapArgs g, BeamArgs a) {
  constexpr int kNs = beam_sums(K);  // float64 sums of a row
  constexpr int kNv = kNs + 1;       // and the hits
  static_assert(kNv <= kWave, "a lane per sum");
  __shared__ DetConst dets[kTileDet];
  __shared__ DetJac jacs[kTileDet];
  __shared__ double pars[kTileDet][K];
  __shared__ double part[kTileDet][kWaves][kNv];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int d0 = blockIdx.y * kTileDet;
  const int nd = min(kTileDet, g.D - d0);
  const int chunk = blockIdx.x;
  if ((int)threadIdx.x < nd) {
    dets[threadIdx.x] = make_det_const(g, d0 + threadIdx.x);
    jacs[threadIdx.x] = make_det_jac(dets[threadIdx.x], g.dx[d0 + threadIdx.x], g.dy[d0 + threadIdx.x]);
#pragma unroll
    for (int k = 0; k < K; ++k) pars[threadIdx.x][k] = a.param[(size_t)(d0 + threadIdx.x) * K + k];
  }
  for (int i = threadIdx.x; i < kTileDet * kWaves * kNv; i += kBlock) (&part[0][0][0])[i] = 0.0;
  __syncthreads();
  const int tile_end = min((chunk + 1) * kChunkTiles, (g.T + kTileSamples - 1) / kTileSamples);
  for (int tile = chunk * kChunkTiles; tile < tile_end; ++tile) {
    const int sb = tile * kTileSamples + (int)threadIdx.x * kSamplesPerThread;
    // one read of the flags: is anything of this wave's samples kept in any row?
    bool any = false;
    {
      const unsigned char* at = a.flags ? a.flags + (size_t)d0 * a.ld_f + sb : nullptr;
#pragma unroll 8
      for (int dl = 0; dl < kTileDet; ++dl) {
        if (dl < nd) {
          any = any || kept_mask(flag_word(at, a.wide_f, sb, g.T)) != 0u;
          if (at) at += a.ld_f;
        }
      }
    }
    if (__builtin_amdgcn_ballot_w64(any) == 0) continue;  // (wave-uniform)
    for (int dl = 0; dl < nd; ++dl) {
      const int d = d0 + dl;
      const unsigned keep = kept_mask(flag_word(a.flags ? a.flags + (size_t)d * a.ld_f + sb : nullptr, a.wide_f, sb, g.T));
      if (__builtin_amdgcn_ballot_w64(keep != 0u) == 0) continue;  // (wave-uniform)
      const DetConst dc = dets[dl];
      const DetJac dj = jacs[dl];
      const double* const p = pars[dl];  // (from LDS: uniform values in vector registers, the scalar ones are short)
      const double A = p[0], c0 = p[K - 1];
      const double qa = p[3], qb = K == 7 ? p[4] : 0.0, qc = K == 7 ? p[5] : p[3];
      const float* const xr = a.x + (size_t)d * a.ld_x;
      const float* const mr = kModel ? a.model + (size_t)d * a.ld_m : nullptr;
      double s[kNs];
#pragma unroll
      for (int j = 0; j < kNs; ++j) s[j] = 0.0;
      unsigned n = 0u;
      // one body for the four samples (not unrolled: its float64 constants and the exponential would be held four times)
#pragma unroll 1
      for (int q = 0; q < kSamplesPerThread; ++q) {
        if (keep & (1u << q)) {
          const int t = sb + q;
          SampleConst cur{};
#pragma unroll
          for (int j = 0; j < 6; ++j) cur.G[j] = a.rot[6 * (size_t)t + j];
          const double sxq = a.src ? (double)a.src[2 * (size_t)t] : 0.0, syq = a.src ? (double)a.src[2 * (size_t)t + 1] : 0.0;
          float ox, oy, el_d;
          sample_offsets<false, false>(g, dc, cur, ox, oy, el_d);
          // the factor asin(r) / r of sample_offsets, by sample_offsets' own float32 expressions (the same bits), held
          // constant in the derivative; d(ox, oy)/d(dx, dy) = -f (dc/d. @ G)
          const float zr = fmaf(dc.c_re, cur.G[0], fmaf(dc.c_cr, cur.G[2], dc.c_im * cur.G[4]));
          const float zi = fmaf(dc.c_re, cur.G[1], fmaf(dc.c_cr, cur.G[3], dc.c_im * cur.G[5]));
          const float r2 = fmaf(zr, zr, zi * zi);
          float ff = fmaf(r2, fmaf(r2, fmaf(r2, fmaf(r2, 35.0f / 1152.0f, 15.0f / 336.0f), 3.0f / 40.0f), 1.0f / 6.0f), 1.0f);
          if (r2 >= 0.01f) {
            const float r = sqrtf(r2);
            ff = asinf(fminf(r, 1.0f)) / r;
          }
          const double f = (double)ff;
          const double G0 = (double)cur.G[0], G1 = (double)cur.G[1], G2 = (double)cur.G[2], G3 = (double)cur.G[3], G4 = (double)cur.G[4],
                       G5 = (double)cur.G[5];
          const double oxx = -f * (dj.cx[0] * G0 + dj.cx[1] * G2 + dj.cx[2] * G4);
          const double oyx = -f * (dj.cx[0] * G1 + dj.cx[1] * G3 + dj.cx[2] * G5);
          const double oxy = -f * (dj.cy[0] * G0 + dj.cy[1] * G2 + dj.cy[2] * G4);
          const double oyy = -f * (dj.cy[0] * G1 + dj.cy[1] * G3 + dj.cy[2] * G5);
          const double u = (double)ox - sxq, v = (double)oy - syq;
          const double term = kModel ? (double)xr[t] - (double)mr[t] : (double)xr[t];
          const double quad = K == 7 ? qa * (u * u) + 2.0 * qb * (u * v) + qc * (v * v) : qa * (u * u + v * v);
          const double e = exp(-quad / 2.0);
          const double Ae = A * e;
          const double r = term - (Ae + c0);
          const double mu = -Ae * (K == 7 ? qa * u + qb * v : qa * u);  // dm/du
          const double mv = -Ae * (K == 7 ? qb * u + qc * v : qa * v);  // dm/dv
          double J[K];
          J[0] = e;
          J[1] = mu * oxx + mv * oyx;
          J[2] = mu * oxy + mv * oyy;
          if (K == 7) {
            J[3] = -Ae * (u * u) / 2.0;
            J[4] = -Ae * (u * v);
            J[5] = -Ae * (v * v) / 2.0;
          } else {
            J[3] = -Ae * (u * u + v * v) / 2.0;
          }
          J[K - 1] = 1.0;
          s[0] = s[0] + r * r;
          int k = 1;
#pragma unroll
          for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = i; j < K; ++j, ++k) s[k] = s[k] + J[i] * J[j];
#pragma unroll
          for (int i = 0; i < K; ++i, ++k) s[k] = s[k] + J[i] * r;
          n += 1u;
        }
      }
      mrx_tod::wave_sum_all(s, n);
      if (lane == 0) {  // (a select per lane and sum would hold 37 lane masks in scalar registers across the loops)
        double* const mine = part[dl][wave];
#pragma unroll
        for (int j = 0; j < kNs; ++j) mine[j] = mine[j] + s[j];
        mine[kNs] = mine[kNs] + (double)n;  // the hits (exact: below 2^31)
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nd * kNv; i += kBlock) {
    const int dl = i / kNv, j = i - dl * kNv;
    double v = part[dl][0][j];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v = v + part[dl][w][j];
    a.work[((size_t)(d0 + dl) * a.n_chunks + chunk) * kNv + j] = v;
  }
}

// a row's chunks in ascending order: sum j of row d to out[d][j], the hits to count[d]
__global__ __launch_bounds__(kBlock) void beam_finish_kernel(const double* __restrict__ work, int n_chunks, int nv, long long n, double* __restrict__ out,
                                                             int* __restrict__ count) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const long long d = i / nv;
  const int j = (int)(i - d * nv);
  const double* const w = work + (size_t)d * n_chunks * nv + j;
  double v = 0.0;
  for (int c = 0; c < n_chunks; ++c) v = v + w[(size_t)c * nv];
  if (j < nv - 1)
    out[(size_t)d * (nv - 1) + j] = v;
  else
    count[d] = (int)v;
}

// the frame's centre and the pointing, as mrx_map.hip's map_args fills them; no map, no Stokes weights (S = 0)
MapArgs frame_args(double center_phi, double center_theta, const float* d_az, const float* d_el, int T, const double* d_transform,
                   const float* d_dx, const float* d_dy, int D) {
  MapArgs g{};
  g.cphi = (float)center_phi;
  const float ang = (float)(1.5707963267948966 - center_theta);
  g.rot_re = (float)cos((double)ang);
  g.rot_im = (float)sin((double)ang);
  g.cos_cphi = cos(center_phi);
  g.sin_cphi = sin(center_phi);
  g.cos_ctheta = cos(center_theta);
  g.sin_ctheta = sin(center_theta);
  g.az = d_az;
  g.el = d_el;
  g.transform = d_transform;
  g.dx = d_dx;
  g.dy = d_dy;
  g.D = D;
  g.T = T;
  return g;
}

int n_chunks_of(int T) { return mrx_ceil_div(mrx_ceil_div(T, kTileSamples), kChunkTiles); }

size_t work_doubles(int D, int T, int K) { return (size_t)D * n_chunks_of(T) * (beam_sums(K) + 1); }

}  // namespace

extern "C" {

int mrx_tod_source_flag(mrx_ctx* ctx, const float* d_az, const float* d_el, int T, const double* d_transform, const float* d_dx,
                        const float* d_dy, int D, double center_phi, double center_theta, const float* d_src, double radius, int inside,
                        int value, uint8_t* d_flags, size_t ld_f) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_az && d_el && d_dx && d_dy && d_flags, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, ld_f >= (size_t)T, "ld_f smaller than T");
  MRX_REQUIRE(ctx, value >= 1 && value <= 255, "value must be in 1 .. 255");
  MRX_REQUIRE(ctx, inside == 0 || inside == 1, "inside must be 0 or 1");
  MRX_REQUIRE(ctx, radius >= 0.0 && radius < INFINITY, "radius must be finite and >= 0");
  MRX_REQUIRE(ctx, center_phi == center_phi && center_theta == center_theta && fabs(center_phi) < INFINITY && fabs(center_theta) < INFINITY,
              "the centre must be finite");
  MRX_REQUIRE(ctx, mrx_ceil_div(D, kTileDet) <= 65535, "D too large for one launch");
  MRX_REQUIRE(ctx, T <= 0x7fffffff - 2 * kTileSamples, "T too large: sample indices are 32-bit");
  if (ctx->options[MRX_OPT_POINTING_CHAIN])
    return mrx_fail(ctx, MRX_ERR_UNSUPPORTED, "%s: composed pointing only (MRX_OPT_POINTING_CHAIN is set)", __func__);
  const MapArgs g = frame_args(center_phi, center_theta, d_az, d_el, T, d_transform, d_dx, d_dy, D);
  const int wide = mrx_aligned(d_flags, ld_f, 4);
  hipLaunchKernelGGL(source_flag_kernel, dim3(mrx_ceil_div(T, kTileSamples), mrx_ceil_div(D, kTileDet)), dim3(kBlock), 0, ctx->stream, g, d_src,
                     radius * radius, inside, (unsigned)value, d_flags, ld_f, wide);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_beam_normal_work_bytes(int D, int T, int K, size_t* bytes) {
  if (!bytes || D < 1 || T < 1 || (K != 5 && K != 7)) return MRX_ERR_INVALID;
  *bytes = work_doubles(D, T, K) * sizeof(double) + (2 * (size_t)D + 6 * (size_t)T) * sizeof(float);
  return MRX_OK;
}

int mrx_tod_beam_normal(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m, const uint8_t* d_flags, size_t ld_f,
                        const float* d_az, const float* d_el, int T, const double* d_transform, const float* d_dx, const float* d_dy,
                        int D, double center_phi, double center_theta, const float* d_src, const double* d_param, int K, double* d_out, int32_t* d_count,
                        void* d_work, size_t work_bytes) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  (void)d_dx, (void)d_dy;  // the nominal offsets are not read: the trial ones of d_param stand in their place
  MRX_REQUIRE(ctx, d_x && d_az && d_el && d_param && d_out && d_count && d_work, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, K == 5 || K == 7, "K must be 5 (circular) or 7 (elliptical)");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && (!d_model || ld_m >= (size_t)T) && (!d_flags || ld_f >= (size_t)T), "ld_x, ld_m or ld_f smaller than T");
  MRX_REQUIRE(ctx, center_phi == center_phi && center_theta == center_theta && fabs(center_phi) < INFINITY && fabs(center_theta) < INFINITY,
              "the centre must be finite");
  MRX_REQUIRE(ctx, mrx_ceil_div(D, kTileDet) <= 65535, "D too large for one launch");
  MRX_REQUIRE(ctx, T <= 0x7fffffff - 2 * kTileSamples, "T too large: sample indices are 32-bit");
  MRX_REQUIRE(ctx, mrx_aligned(d_work, 0, 8), "d_work must be 8-byte aligned");
  size_t need = 0;
  (void)mrx_tod_beam_normal_work_bytes(D, T, K, &need);
  MRX_REQUIRE(ctx, work_bytes >= need, "work buffer smaller than mrx_tod_beam_normal_work_bytes");
  if (ctx->options[MRX_OPT_POINTING_CHAIN])
    return mrx_fail(ctx, MRX_ERR_UNSUPPORTED, "%s: composed pointing only (MRX_OPT_POINTING_CHAIN is set)", __func__);
  double* const work = static_cast<double*>(d_work);
  float* const tdx = reinterpret_cast<float*>(work + work_doubles(D, T, K));
  float* const tdy = tdx + D;
  float* const rot = tdy + D;
  hipLaunchKernelGGL(beam_trial_kernel, dim3(mrx_ceil_div(D, kBlock)), dim3(kBlock), 0, ctx->stream, d_param, K, D, tdx, tdy);
  MRX_CHECK_LAUNCH(ctx);
  const MapArgs g = frame_args(center_phi, center_theta, d_az, d_el, T, d_transform, tdx, tdy, D);
  hipLaunchKernelGGL(beam_rotation_kernel, dim3(mrx_ceil_div(T, kBlock)), dim3(kBlock), 0, ctx->stream, g, rot);
  MRX_CHECK_LAUNCH(ctx);
  const int n_chunks = n_chunks_of(T);
  const BeamArgs a{d_x, ld_x, d_model, ld_m, d_flags, ld_f, d_flags && mrx_aligned(d_flags, ld_f, 4),
                   d_src, rot, d_param, work, n_chunks};
  const dim3 grid(n_chunks, mrx_ceil_div(D, kTileDet));
  if (K == 5 && d_model)
    hipLaunchKernelGGL((beam_normal_kernel<5, true>), grid, dim3(kBlock), 0, ctx->stream, g, a);
  else if (K == 5)
    hipLaunchKernelGGL((beam_normal_kernel<5, false>), grid, dim3(kBlock), 0, ctx->stream, g, a);
  else if (d_model)
    hipLaunchKernelGGL((beam_normal_kernel<7, true>), grid, dim3(kBlock), 0, ctx->stream, g, a);
  else
    hipLaunchKernelGGL((beam_normal_kernel<7, false>), grid, dim3(kBlock), 0, ctx->stream, g, a);
  MRX_CHECK_LAUNCH(ctx);
  const int nv = beam_sums(K) + 1;
  const long long n = (long long)D * nv;
  hipLaunchKernelGGL(beam_finish_kernel, dim3(mrx_ceil_div(n, kBlock)), dim3(kBlock), 0, ctx->stream, work, n_chunks, nv, n, d_out, d_count);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // extern "C"
