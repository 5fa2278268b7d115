// The pointing of the map operators, steps 1-3 of mrx_map_sample.hip (detector az/el, frame rotation, offsets from the
// map centre), shared by the translation units that need a detector sample's offsets exactly as the binning computes them
// (mrx_map_sample.hip, mrx_map.hip, mrx_beamfit.hip): the map's axes and arguments (with the host's make_axis and
// map_args), the per-detector and per-sample constants and the offsets themselves.  The three files are built with the
// same flags (no FMA contraction), so that the same inputs give the same bits.
#pragma once

#include <cmath>

#include "mrx_internal.h"
#include "mrx_krj.h"  // the tile (mrx_tile.h: 16 rows x 1024 samples, 4 a thread) and the small-angle series

namespace {

static_assert(kBlock == 256 && kTileDet == 16 && kSamplesPerThread == 4 && kTileSamples == 1024, "the map kernels are written for the TOD tile");
constexpr int kMaxStokes = 4;
constexpr float kHalfPiF = 1.57079637050628662109375f;
constexpr float kTwoPiF = 6.283185482025146484375f;

// One map axis: node i sits at first + i * step (np.linspace, map/projection.py:122-123;
// step of either sign -- eta is descending after the parity flip).
struct Axis {
  int n;
  double first, inv_step;
  float lo, hi;  // float32 bounds just beyond the axis (one pixel either side): offsets are clamped into them first
  double u_last;  // the largest double below n - 1 (axis_cell, nearest pixel)
  // The sampler's bilinear cell in float32 (axis_cell): u = x inv + c with inv = inv_hi + inv_lo (float32 head and tail of
  // 1 / step) and c = -first / step = c_int + c_frac (an integer and a fraction in [0, 1), both exact float32 numbers or
  // rounded at 6e-8).  x_min / x_max: the float32 numbers just inside the axis' ends; k_lo / k_hi: the cells 0 and n - 2
  // counted from c_int.
  float inv_hi, inv_lo, c_int, c_frac, x_min, x_max, k_lo, k_hi;
};

inline Axis make_axis(int n, double first, double step) {  // (host)
  Axis a{n, first, 1.0 / step, 0.0f, 0.0f, (double)(n - 1) * (1.0 - 1.1102230246251565e-16)};
  const double x0 = first - 1.5 * step, x1 = first + ((double)n + 0.5) * step;
  a.lo = (float)(x0 < x1 ? x0 : x1);
  a.hi = (float)(x0 < x1 ? x1 : x0);
  a.inv_hi = (float)a.inv_step;
  a.inv_lo = (float)(a.inv_step - (double)a.inv_hi);
  const double c = -first * a.inv_step, ci = std::floor(c);
  a.c_int = (float)ci;  // (|c| < 2^24: a map axis has fewer than 2^24 nodes, and the host refuses centres farther off)
  a.c_frac = (float)(c - ci);
  const double last = first + (double)(n - 1) * step, e0 = first < last ? first : last, e1 = first < last ? last : first;
  a.x_min = (float)e0;
  a.x_max = (float)e1;
  if ((double)a.x_min < e0) a.x_min = std::nextafterf(a.x_min, INFINITY);
  if ((double)a.x_max > e1) a.x_max = std::nextafterf(a.x_max, -INFINITY);
  a.k_lo = -a.c_int;
  a.k_hi = (float)(n - 2) - a.c_int;
  return a;
}

struct MapArgs {
  const float* values;  // [C][S][n_eta][n_xi]
  Axis eta, xi;
  int C, S, n_eta, n_xi;
  float cphi;           // map centre longitude (float32, as jax demotes it)
  float rot_re, rot_im; // exp(i (pi/2 - ctheta)) in complex64
  double cos_cphi, sin_cphi, cos_ctheta, sin_ctheta;  // the same centre in float64 (direct mode)
  int bilinear;
  // calibration
  const float* cal;       // [C][n_pwv][n_el] or null
  const float* cal_pwv;   // [n_pwv]
  const float* cal_el;    // [n_el]
  int n_pwv, n_el;
  const double* pwv;      // [Ta][D] coarse zenith-scaled pwv
  int Ta;
  double ta0, dta, inv_dta;
  const double* t;        // [T]
  const double* scalar;   // [C] (no atmosphere)
  // pointing
  const float* az;        // [T]
  const float* el;        // [T]
  const double* transform;  // [T][9] or null
  const float* dx;
  const float* dy;
  const double* stokes_w;  // [D][S]
  int D, T;
  float* out;
  size_t ld;
  int vec_ok;
  uint32_t map_bytes;  // of all planes (below 4 GiB): the sampler's raw buffer
  // The map's row pairs interleaved (round 6): pairs[plane][e][x] = (m[e][x], m[e + 1][x]), e = 0 .. n_eta - 2 -- the four
  // corners of a cell are then 16 contiguous bytes, ONE gather a sample and plane instead of two of 8 bytes.  The
  // sampler waits on the number of gather instructions (a what-if build without them: 7.1 -> 3.9 ms; the texture
  // addresser takes a wave's 64 addresses at the same rate whether they fetch 8 or 16 bytes), not on bytes or arithmetic.
  const float* pairs;
  uint32_t pairs_bytes;
  int coef_offset;     // of the calibration's interval table in the dynamic LDS, in floats; < 0: none (more than kCalFastChannels channels)
  int coef_cap;        // coarse steps per row the table holds
};

// the map's grid and centre and the detectors' pointing, as every map kernel takes them (the callers check the sizes)
inline MapArgs map_args(const mrx_sky_map* map, const float* d_az, const float* d_el, int T, const double* d_transform,
                        const float* d_dx, const float* d_dy, const double* d_stokes_w, int D) {  // (host)
  MapArgs g{};
  g.eta = make_axis(map->n_eta, map->eta0, map->deta);
  g.xi = make_axis(map->n_xi, map->xi0, map->dxi);
  g.C = map->n_channels;
  g.S = map->n_stokes;
  g.n_eta = map->n_eta;
  g.n_xi = map->n_xi;
  g.cphi = (float)map->center_phi;
  // exp(1j * (pi/2 - ctheta)) as jax evaluates it: the python float demoted to float32,
  // then a complex64 exponential
  const float ang = (float)(1.5707963267948966 - map->center_theta);
  g.rot_re = (float)cos((double)ang);
  g.rot_im = (float)sin((double)ang);
  g.cos_cphi = cos(map->center_phi);
  g.sin_cphi = sin(map->center_phi);
  g.cos_ctheta = cos(map->center_theta);
  g.sin_ctheta = sin(map->center_theta);
  g.bilinear = map->bilinear;
  g.az = d_az;
  g.el = d_el;
  g.transform = d_transform;
  g.dx = d_dx;
  g.dy = d_dy;
  g.stokes_w = d_stokes_w;
  g.D = D;
  g.T = T;
  return g;
}

// TOD.to("K_RJ") on the sampler's store (mrx_map_sample_krj): the arguments of mrx_tod_to_krj for the rows of this call
struct MapKrj {
  const float* bore_el;     // [T]
  const float* dx;          // [D]
  const float* dy;          // [D]
  const int32_t* band;      // [D]
  const float* scale;       // [D] or null
  const float* cal_axis;    // [n_el]
  const float* cal_values;  // [n_bands][n_el]
  int n_el, n_bands;
  int cells_offset;         // of the cell table in the dynamic LDS, in float4
};

struct DetConst {
  float c_re, c_cr, c_im;  // sin(r)cos(p), cos(r), sin(r)sin(p)
  double w[kMaxStokes];    // Mueller[d, 0, stokes]: float64 for the binning's float64 sums; map sampling rounds them to float32
};

struct SampleConst;
__device__ __forceinline__ int sc_index(const struct MapArgs& g, const SampleConst& sc);

// What a sample contributes to every detector of the tile.
struct SampleConst {
  float ca, sa;   // cos / sin of (el_bore - pi/2), float32 as the chain computes them
  float az;       // boresight azimuth
  float G[6];     // direct mode: (dz_re, dz_im) = c @ G, c = (sin r cos p, cos r, sin r sin p); composed in float64
  int jj;         // coarse interval of the sample time and the weight within it
  double u;
  int s;          // the (clamped) sample index
};

__device__ __forceinline__ int sc_index(const MapArgs&, const SampleConst& sc) { return sc.s; }

// The coarse step of the pwv series that time t falls in, 0 .. Ta - 2, and t's place u in it in float64 (below 0 or past
// 1 where the series is extrapolated): linear interpolation of the coarse series (sim/atmosphere.py:30-37).  The one
// statement of this arithmetic: the per-sample calibration (sample_const, the sampler's slot_record) and the interval form
// (IntervalCal, mrx_map_sample.hip) must name the same step for the same time, and tests/test_gpu_map_cal.py restates it.
__device__ __forceinline__ int coarse_step(const MapArgs& g, double t, double& u) {
  int jj = (int)floor(fmin(fmax((t - g.ta0) * g.inv_dta, -1.0), 2.0e9));
  jj = min(max(jj, 0), g.Ta - 2);
  u = (t - (g.ta0 + (double)jj * g.dta)) * g.inv_dta;
  return jj;
}

__device__ __forceinline__ void sample_const(const MapArgs& g, int s, bool chain, SampleConst& sc) {
  s = min(max(s, 0), g.T - 1);
  const float a = __fsub_rn(g.el[s], kHalfPiF);
  sc.ca = cosf(a);
  sc.sa = sinf(a);
  sc.az = g.az[s];
  if (g.cal) sc.jj = coarse_step(g, g.t[s], sc.u);  // zenith-scaled pwv of the sample
  if (!chain) {
    // Steps 1-3 are rotations of the unit vector c: xyz = c @ R(az, el), v = xyz @ M(t),
    // and phi_theta_to_offsets only needs two components of v in the frame of the map
    // centre, dz = (sin dphi cos theta, cos dphi cos theta sin ctheta - sin theta cos ctheta).
    // Composed once per sample in float64.
    const double ca = (double)sc.ca, sa = (double)sc.sa;
    const double cb = cos((double)sc.az), sb = sin((double)sc.az);
    // rows of R: xyz = c_re R[0] + c_cr R[1] + c_im R[2]
    const double R[3][3] = {{ca * cb, ca * sb, sa}, {-sa * cb, -sa * sb, ca}, {-sb, cb, 0.0}};
    double P[3][2];  // v -> dz: P = M @ Cmat^T
    double M[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (g.transform) {
      const double* m = g.transform + (size_t)s * 9;
#pragma unroll
      for (int k = 0; k < 9; ++k) M[k] = m[k];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double vx = M[j * 3 + 0], vy = M[j * 3 + 1], vz = M[j * 3 + 2];
      P[j][0] = -vx * g.sin_cphi + vy * g.cos_cphi;
      P[j][1] = (vx * g.cos_cphi + vy * g.sin_cphi) * g.sin_ctheta - vz * g.cos_ctheta;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 2; ++k) sc.G[i * 2 + k] = (float)(R[i][0] * P[0][k] + R[i][1] * P[1][k] + R[i][2] * P[2][k]);
  }
}

// asin on [-1, 1] by Abramowitz & Stegun 4.4.46 (|error| <= 2e-8, below the float32 spacing of
// an elevation): pi/2 - sqrt(1 - |x|) P7(|x|).  Only the composed path's table lookup uses it.
__device__ __forceinline__ float asin_poly(float x) {
  const float a = fabsf(x);
  float p = -0.0012624911f;
  p = fmaf(p, a, 0.0066700901f);
  p = fmaf(p, a, -0.0170881256f);
  p = fmaf(p, a, 0.0308918810f);
  p = fmaf(p, a, -0.0501743046f);
  p = fmaf(p, a, 0.0889789874f);
  p = fmaf(p, a, -0.2145988016f);
  p = fmaf(p, a, 1.5707963050f);
  const float r = 1.57079632679f - sqrtf(fmaxf(1.0f - a, 0.0f)) * p;
  return copysignf(r, x);
}

// Steps 1-3: offsets (ox, oy) of one detector sample from the map centre, and the
// detector's elevation when the calibration needs it.
template <bool kChain, bool kNeedEl>
__device__ __forceinline__ void sample_offsets(const MapArgs& g, const DetConst& dc, const SampleConst& sc,
                                               float& ox, float& oy, float& el_d) {
  const float im = __fadd_rn(__fmul_rn(dc.c_re, sc.sa), __fmul_rn(dc.c_cr, sc.ca));
  el_d = 0.0f;
  if (kChain) {
    // 1. detector az/el (transforms.py:10-29)
    const float re = __fsub_rn(__fmul_rn(dc.c_re, sc.ca), __fmul_rn(dc.c_cr, sc.sa));
    const float az_d = __fadd_rn(atan2f(dc.c_im, re), sc.az);
    el_d = asinf(im);
    // 2. frame rotation (coordinates.py:220-230)
    float phi = az_d, theta = el_d;
    if (g.transform) {
      const float ce = cosf(el_d);
      const double x = (double)__fmul_rn(cosf(az_d), ce), y = (double)__fmul_rn(sinf(az_d), ce), z = (double)sinf(el_d);
      const double* M = g.transform + (size_t)sc_index(g, sc) * 9;
      const float vx = (float)(x * M[0] + y * M[3] + z * M[6]);
      const float vy = (float)(x * M[1] + y * M[4] + z * M[7]);
      const float vz = (float)(x * M[2] + y * M[5] + z * M[8]);
      float ph = fmodf(atan2f(vy, vx), kTwoPiF);
      if (ph < 0.0f) ph = __fadd_rn(ph, kTwoPiF);
      phi = ph;
      const float nrm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(vx, vx), __fmul_rn(vy, vy)), __fmul_rn(vz, vz)));
      theta = asinf(__fdiv_rn(vz, nrm));
    }
    // 3. offsets from the map centre (transforms.py:36-53)
    const float dphi = __fsub_rn(phi, g.cphi);
    const float ct = cosf(theta), st = sinf(theta);
    const float pr = __fmul_rn(cosf(dphi), ct);
    const float proj_re = __fsub_rn(__fmul_rn(pr, g.rot_re), __fmul_rn(st, g.rot_im));
    const float dz_re = __fmul_rn(sinf(dphi), ct), dz_im = proj_re;
    const float r = sqrtf(__fadd_rn(__fmul_rn(dz_re, dz_re), __fmul_rn(dz_im, dz_im)));
    const float f = __fdiv_rn(asinf(r), r > 0.0f ? r : 1.0f);
    ox = -__fmul_rn(dz_re, f);
    oy = -__fmul_rn(dz_im, f);
  } else {
    // float32 (round 3): the offsets are float32 numbers in the reference (transforms.py:36-53); with the
    // composed rotation rounded to float32 every term below is good to 6e-8 of ~1e-2 rad, i.e. to the
    // spacing of the float32 result itself
    const float dz_re = fmaf(dc.c_re, sc.G[0], fmaf(dc.c_cr, sc.G[2], dc.c_im * sc.G[4]));
    const float dz_im = fmaf(dc.c_re, sc.G[1], fmaf(dc.c_cr, sc.G[3], dc.c_im * sc.G[5]));
    const float r2 = fmaf(dz_re, dz_re, dz_im * dz_im);
    // asin(r)/r: the series to r^8 below 0.1 rad (error < 3e-10), the function beyond
    float f = fmaf(r2, fmaf(r2, fmaf(r2, fmaf(r2, 35.0f / 1152.0f, 15.0f / 336.0f), 3.0f / 40.0f), 1.0f / 6.0f), 1.0f);
    if (__builtin_amdgcn_ballot_w64(r2 >= 0.01f) != 0) {
      if (r2 >= 0.01f) {
        const float r = sqrtf(r2);
        f = asinf(fminf(r, 1.0f)) / r;
      }
    }
    ox = -dz_re * f;
    oy = -dz_im * f;
    if (kNeedEl) el_d = asin_poly(im);
  }
}

__device__ __forceinline__ DetConst make_det_const(const MapArgs& g, int d) {
  // transforms.py:14-23: r = |offset|, p = atan2(-dx, -dy); c = (sin r cos p, cos r, sin r sin p) = (-dy s, cos r, -dx s) with
  // s = sin(r) / r.  Round 6: the series of mrx_krj.h for a focal-plane offset (exact to a float32 rounding below 0.3 rad)
  // instead of a square root, an arctangent and four sines and cosines -- once per row and tile, but on sixteen lanes of
  // one wave while the workgroup waits at the barrier behind it.
  const float dx = g.dx[d], dy = g.dy[d];
  const float r2 = fmaf(dx, dx, dy * dy);
  DetConst dc;
  if (r2 < 0.09f) {
    const float sc = sinc_small(r2);
    dc.c_re = -dy * sc;
    dc.c_cr = cos_small(r2);
    dc.c_im = -dx * sc;
  } else {
    const float r = sqrtf(r2);
    const float p = atan2f(-dx, -dy);
    const float sr = sinf(r);
    dc.c_re = __fmul_rn(sr, cosf(p));
    dc.c_cr = cosf(r);
    dc.c_im = __fmul_rn(sr, sinf(p));
  }
  for (int k = 0; k < kMaxStokes; ++k) dc.w[k] = k < g.S ? g.stokes_w[(size_t)d * g.S + k] : 0.0;
  return dc;
}
}  // namespace
