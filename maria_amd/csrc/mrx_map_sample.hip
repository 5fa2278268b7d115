// Map sampling for gfx950: the celestial map's contribution to
// the TOD, sim/map.py:76-172.  For every detector sample the reference
//   1. takes the detector's az/el (coords/transforms.py:10-29, float32),
//   2. rotates it into the map's frame: float32 unit vector times the float64 3x3
//      of that sample, back to float32 angles (coords/coordinates.py:220-230),
//   3. turns the angles into offsets from the map centre (transforms.py:36-53, float32),
//   4. builds a sparse pointing matrix from np.digitize on the eta / xi axes with
//      bilinear (or nearest) weights in float64, times the Stokes row of the
//      detector's Mueller matrix (utils/linalg.py:9-58, map/projection.py:134-179),
//   5. multiplies P @ map by the channel's K_RJ -> pW factor 1e12 k_B Int tau exp(-opacity)
//      looked up at the sample's (zenith pwv, elevation) (band/band.py:235-255),
//      accumulates the channels in float32,
//   6. convolves the result with [0.25, 0.5, 0.25] along time (scipy reflect mode).
// Here all of it is one kernel: no [D, T] pointing, no sparse matrix, one store per
// sample.  Tile = 16 detectors x 1024 samples like the TOD writer; a thread computes 4
// consecutive raw samples per detector and trades edge values with its neighbours
// through LDS for the 3-tap kernel (tile edges: one extra evaluation by the first and
// last thread).  Steps 1-3 are three rotations of a unit vector: by default they are
// composed once per sample in float64 and applied to the detector's vector with six
// multiply-adds (the literal float32 chain, ~15 transcendental calls per sample, stays
// available through MRX_OPT_POINTING_CHAIN and agrees to float32 rounding of the angles).
// Bound by arithmetic (float64 weights and sums, as the reference's sparse product), not
// by memory.
// The operators on the same pointing -- the binning, the maximum-likelihood map-maker's and the destriper's -- are
// mrx_map.hip; the two files share steps 1-3 and the host's map_args (mrx_map_pointing.h) and the build's flags.
#include <cmath>
#include <type_traits>

#include "mrx_internal.h"
#include "mrx_krj.h"  // the tile (mrx_tile.h: 16 rows x 1024 samples, 4 a thread) and TOD.to("K_RJ") on the sampler's store
#include "mrx_map_pointing.h"  // steps 1-3: MapArgs, map_args, DetConst, SampleConst, sample_const, sample_offsets, make_det_const

namespace {

// One axis of utils/linalg.py:25-41 for the map SAMPLER (the binning's form is axis_weights, mrx_map.hip), as one cell:
// i0 in [0, n - 2] and the weight p in [0, 1] of node i0 + 1 -- the value
// (1 - p) v[i0] + p v[i0 + 1] is axis_weights' everywhere: inside the axis the same floor and the same fraction of the
// same float64 u; at a node p = 0; before the first node (0, p = 0) = v[0]; from the last node on (n - 2, p = 1) =
// v[n - 1], where axis_weights says (n - 1, n - 1, 0).  What it saves the kernel -- which is bound by its instruction
// count (173 vector instructions a sample, the SIMDs 85 % busy issuing them) -- is the integer clamps and selects of two
// indices (u is clamped instead, NaN to the low end by fmax's rule; just below n - 1, so that the floor stays <= n - 2)
// and, in sample_value, the special case of the last column for its corner pairs: 26 -> 16 issue slots an axis.
template <bool kBil>
__device__ __forceinline__ void axis_cell_t(const Axis& a, float x, int& i0, float& p) {
  if (kBil) {
    // Round 6: float32, no float64 (nine of the axis' eleven instructions were float64, at half rate or less).  With
    // u = x inv + c split as in Axis: p0 = x inv_hi + c_frac is u - c_int to float32 rounding (3e-5 pixel at pixel 500: good
    // enough to name the cell, not the weight); k = floor(p0) kept inside the axis; then the weight as
    // (x inv_hi - k) + (x inv_lo + c_frac): the first bracket is ONE fused multiply-add whose exact value is below one
    // pixel, so it rounds at 6e-8 of a pixel -- the float64 form's fraction to float32 rounding.  A p0 within rounding of
    // an integer may name the neighbouring cell: the weight then comes out just below 0 or just above 1, which is the same
    // interpolated value to 1e-7 of the corner difference.  The offset is first clamped INTO the axis (a NaN goes to the
    // low end by med3's rule): before the first node (cell 0, p = 0), from the last node on (cell n - 2, p = 1).
    const float xc = __builtin_amdgcn_fmed3f(x, a.x_min, a.x_max);
    const float k = __builtin_amdgcn_fmed3f(floorf(fmaf(xc, a.inv_hi, a.c_frac)), a.k_lo, a.k_hi);
    p = fmaf(xc, a.inv_hi, -k) + fmaf(xc, a.inv_lo, a.c_frac);
    i0 = (int)(k + a.c_int);
  } else {
    // np.digitize on the midpoints: the nearest node, as the cell that holds it with weight 0 or 1
    const double u = ((double)x - a.first) * a.inv_step;
    const int i = (int)fmin(fmax(floor(u + 0.5), 0.0), (double)(a.n - 1));
    i0 = min(i, a.n - 2);
    p = i > a.n - 2 ? 1.0f : 0.0f;
  }
}

__device__ __forceinline__ void axis_cell(const Axis& a, float x, bool bilinear, int& i0, float& p) {
  if (bilinear) {  // workgroup-uniform
    asm volatile("" ::: "memory");  // keep this a branch (see axis_weights)
    axis_cell_t<true>(a, x, i0, p);
  } else {
    asm volatile("" ::: "memory");
    axis_cell_t<false>(a, x, i0, p);
  }
}

// jax RegularGridInterpolator index and weight on a float32 axis (searchsorted left)
struct RgiAxis {
  const float* g;  // nodes (LDS)
  int n;
  float first, last, inv;  // inv: (n - 1) / (last - first), the arithmetic first guess
};

__device__ __forceinline__ RgiAxis make_rgi_axis(const float* g, int n) {
  RgiAxis a{g, n, g[0], g[n - 1], 0.0f};
  a.inv = (float)(n - 1) / (a.last - a.first);
  return a;
}

__device__ __forceinline__ void rgi_axis(const RgiAxis& a, float x, int& i, float& w, bool& oob) {
  const float* g = a.g;
  int k = min(max((int)fminf(fmaxf((x - a.first) * a.inv, -1.0f), 2.0e9f), 0), a.n - 2);
  float lo = g[k], hi = g[k + 1];
  while (k < a.n - 2 && hi < x) {
    ++k;
    lo = hi;
    hi = g[k + 1];
  }
  while (k > 0 && lo >= x) {
    --k;
    hi = lo;
    lo = g[k];
  }
  i = k;
  w = (x - lo) * __builtin_amdgcn_rcpf(hi - lo);  // 1 ulp from the reference's division
  oob = !(x >= a.first && x <= a.last);
}

// Steps 4-5 for a sample at offsets (ox, oy) from the map centre, detector elevation el_d.
struct CalLds {
  RgiAxis pwv, el;   // axes (nodes in LDS)
  const float* tab;  // [C][n_pwv][n_el] (LDS)
  const float* chan; // without the tables: [C] pW per K_RJ of a channel, 1e12 k_B x the caller's scalar, float32 (LDS)
};

// the cell of the calibration tables a (zenith pwv, elevation) pair falls in, with jax's index rule and weights
struct CalCell {
  int ip, ie;
  float wp, we;
  bool oob;
};

__device__ __forceinline__ CalCell cal_cell(const CalLds& cl, float pw, float el_d) {
  CalCell k;
  bool o1, o2;
  rgi_axis(cl.pwv, pw, k.ip, k.wp, o1);
  rgi_axis(cl.el, el_d, k.ie, k.we, o2);
  k.oob = o1 || o2;
  return k;
}

// pW per K_RJ of channel c there (band/band.py:250-255): float32 corner sum in product order, weights built as
// (1 * w_pwv) * w_el; 1e12 k_B as a weak scalar on a float32 array
__device__ __forceinline__ float cal_factor(const MapArgs& g, const CalLds& cl, const CalCell& k, int c) {
  const float* tab = cl.tab + c * g.n_pwv * g.n_el + k.ip * g.n_el + k.ie;
  const float wp0 = __fsub_rn(1.0f, k.wp), we0 = __fsub_rn(1.0f, k.we);
  float v = __fmul_rn(tab[0], __fmul_rn(wp0, we0));
  v = __fadd_rn(v, __fmul_rn(tab[1], __fmul_rn(wp0, k.we)));
  v = __fadd_rn(v, __fmul_rn(tab[g.n_el], __fmul_rn(k.wp, we0)));
  v = __fadd_rn(v, __fmul_rn(tab[g.n_el + 1], __fmul_rn(k.wp, k.we)));
  if (k.oob) v = __builtin_nanf("");
  return __fmul_rn(1.380649e-11f, v);
}

constexpr int kCalFastChannels = 4;  // channels whose factors the interval form below tabulates
// The interval form of the per-sample calibration (round 6): per row and coarse step of the pwv series that the tile
// meets, the factor along the step as a parabola in the step's own coordinate (three floats), in LDS as
// [channel][row][steps][3] (row pitch 3 * cap + 1 floats).  kMaxSteps: the most steps a tile may meet for the form to
// apply (the knots' boresight table is sized for it); the launcher sizes the coefficients by mrx_map_cal.steps_per_tile.
constexpr int kMaxSteps = 64, kDefaultSteps = 33;

// Steps 4-5 of one sample with the calibration looked up AT the sample (kCal: the tables at its pwv and the detector's
// elevation; else the caller's scalars): the per-sample form's value
template <bool kCal, int kS>
__device__ __forceinline__ float sample_value(const MapArgs& g, const CalLds& cl, const Axis& ax_eta, const Axis& ax_xi,
                                              const DetConst& dc, const SampleConst& sc, float ox, float oy, float el_d,
                                              double y0, double y1) {
  int e0, x0;
  float pe, px;
  axis_cell(ax_eta, oy, g.bilinear, e0, pe);
  axis_cell(ax_xi, ox, g.bilinear, x0, px);
  // float32 weights and sums (round 3): the reference's float64 sparse product P @ map is rounded to
  // float32 per channel anyway (map.py:155); a float32 evaluation is within 2e-7 of it
  const float qe = 1.0f - pe;
  CalCell cell{};
  if (kCal) cell = cal_cell(cl, (float)fma(sc.u, y1 - y0, y0), el_d);  // (pwv demoted to float32 by the jax interpolator)
  const int plane = g.n_eta * g.n_xi;  // < 2^29: checked by the host (byte offsets in 32 bits)
  // The two corners of a row as ONE 8-byte load (x0, x0 + 1), rows e0 and e0 + 1 (axis_cell: a sample in the last
  // column or row, or beyond, sits in the last cell with upper weight 1).  Round 6: BUFFER loads -- a plane is a raw
  // buffer whose descriptor lives in scalar registers, the cell's byte offset (one 24-bit multiply-add and a shift)
  // is the only vector operand and the second row is the same offset with the row pitch as the scalar offset: the
  // plain loads added the plane's base to a 64-bit vector address twice per plane and sample.
  const float w0a = qe * (1.0f - px), w0b = qe * px, w1a = pe * (1.0f - px), w1b = pe * px;
  const int o0 = (int)(__umul24((unsigned)e0, (unsigned)g.n_xi) + (unsigned)x0) << 2;  // (e0 < n_eta, n_xi < 2^24)
  const int pitch4 = g.n_xi << 2;
  typedef float pair4 __attribute__((ext_vector_type(2)));
  // ONE descriptor for the whole map (four scalar registers for the kernel's life; a descriptor per plane had the
  // compiler keep them all and spill scalars by the hundred), the plane as the load's scalar offset: the host refuses
  // maps of 4 GiB or more.
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)g.values, 0, (int)g.map_bytes, 0x00020000);
  float acc = 0.0f;
  for (int c = 0; c < g.C; ++c) {
    const float pw_per_k = kCal ? cal_factor(g, cl, cell, c) : cl.chan[c];
    float val = 0.0f;
#pragma unroll
    for (int k = 0; k < kS; ++k) {
      const int soff = (c * kS + k) * (plane << 2);
      const pair4 r0 = __builtin_bit_cast(pair4, __builtin_amdgcn_raw_buffer_load_b64(rs, o0, soff, 0));
      const pair4 r1 = __builtin_bit_cast(pair4, __builtin_amdgcn_raw_buffer_load_b64(rs, o0, soff + pitch4, 0));
      const float v = fmaf(w0a, r0.x, fmaf(w0b, r0.y, fmaf(w1a, r1.x, w1b * r1.y)));
      val = k == 0 ? (float)dc.w[k] * v : fmaf((float)dc.w[k], v, val);  // (0 + x: the sum's first term as it is)
    }
    acc = fmaf(pw_per_k, val, acc);  // float32 accumulator (map.py:155)
  }
  return acc;
}

// raw (unconvolved) map loading of one detector at one sample, float32.
// kChain: steps 1-3 literally as the reference's float32 chain; otherwise the composed
// rotation of sample_const (same angles to float32 rounding, ~10x less arithmetic).
// (jj0, y0, y1): the coarse pwv pair the caller already holds for this detector (the samples
// of a thread nearly always share their coarse interval); reloaded when the sample's differs.
template <bool kChain, bool kCal, int kS>
__device__ __forceinline__ float raw_sample(const MapArgs& g, const CalLds& cl, const Axis& ax_eta, const Axis& ax_xi,
                                            const DetConst& dc, int d, const SampleConst& sc, int jj0, double y0,
                                            double y1) {
  float ox, oy, el_d;
  sample_offsets<kChain, kCal>(g, dc, sc, ox, oy, el_d);
  if (kCal && sc.jj != jj0) {
    y0 = g.pwv[(size_t)sc.jj * g.D + d];
    y1 = g.pwv[(size_t)(sc.jj + 1) * g.D + d];
  }
  return sample_value<kCal, kS>(g, cl, ax_eta, ax_xi, dc, sc, ox, oy, el_d, y0, y1);
}

// The tile's sample records in LDS (the composed pointing): six float32 entries of the composed rotation a sample, slot 0
// and kTileSamples + 1 the halo samples of the 3-tap kernel.  As six planes (round 6; an array of 24-byte records before):
// entry k of slot i at p[k * kRecPitch + i + 3], so that a thread's four samples' entries -- slots 1 + 4 tid .. 4 + 4 tid --
// are ONE aligned 16-byte read per plane, consecutive lanes at consecutive addresses.  As records, a thread's slots lay 96
// bytes apart: its three 8-byte reads a sample met the banks four lanes at a time.
constexpr int kRec = 6, kRecPitch = (kTileSamples + 2 + 3 + 3) & ~3;
struct RecordLds {
  float* p;
  __device__ __forceinline__ SampleConst record(int slot) const {  // one sample's
    SampleConst one{};
#pragma unroll
    for (int k = 0; k < kRec; ++k) one.G[k] = p[k * kRecPitch + slot + 3];
    return one;
  }
  // the four samples of a thread at once: G[k][q], slot0 = 1 + 4 tid
  __device__ __forceinline__ void record4(int slot0, float (&G)[kRec][4]) const {
#pragma unroll
    for (int k = 0; k < kRec; ++k) {
      const float4 v = *reinterpret_cast<const float4*>(p + k * kRecPitch + slot0 + 3);
      G[k][0] = v.x; G[k][1] = v.y; G[k][2] = v.z; G[k][3] = v.w;
    }
  }
};

// Round 6: the kN samples of one thread and one detector row TOGETHER (kN = 4, or 5 with the thread's halo sample), for the
// composed rotation with per-channel factors that need no lookup per sample (the caller's scalars, or the stretch form's
// chord).  One sample at a time the kernel was a chain of latencies -- three LDS reads, arithmetic, two gathers from L2,
// arithmetic, per sample and plane, every wave waiting 59 % of its cycles at 38 % of the vector issue rate
// (gpurun_out/r6a_pmc_*: 5.6e9 wave-instructions in 2.8e7 cycles of 1024 SIMDs at two cycles each) -- because the sample's
// code sat behind branches (bilinear or nearest, the far-offset form of asin(r)/r, a guard per channel) that end a basic
// block, and the compiler schedules inside a block.  Here the branches are out of the samples' way: kBil is a template
// parameter, the far-offset form is one vote per row, the channel loop is outside the samples -- so a thread's 2 kN kS
// gathers of a channel are in flight together, behind 3 kN LDS reads issued together.
//   rec: the tile's sample records (LDS); slot[q]: the samples' slots; pw(c, f): fills f[q] with pW per K_RJ of channel c
//   at sample q; kUnrollC: at most kCalFastChannels channels, unrolled under a guard; else a loop.
template <bool kBil, int kS, int kN, bool kUnrollC, typename PwFn>
__device__ __forceinline__ void row_samples(const MapArgs& g, const Axis& ax_eta, const Axis& ax_xi, const DetConst& dc,
                                            const int (&slot)[kN], const RecordLds& rec, PwFn pw, float (&out)[kN]) {
  float ox[kN], oy[kN], r2[kN];
  bool far = false;
  float G[6][kN];  // slots slot[0] .. slot[0] + 3 are the thread's own four samples: one 16-byte read per entry
  {
    float G4[6][4];
    rec.record4(slot[0], G4);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
      for (int q = 0; q < 4; ++q) G[k][q] = G4[k][q];
    }
    if (kN > 4) {
      const SampleConst h = rec.record(slot[kN - 1]);
#pragma unroll
      for (int k = 0; k < 6; ++k) G[k][kN - 1] = h.G[k];
    }
  }
#pragma unroll
  for (int q = 0; q < kN; ++q) {
    // (sample_offsets' composed form: float32, see there)
    const float dz_re = fmaf(dc.c_re, G[0][q], fmaf(dc.c_cr, G[2][q], dc.c_im * G[4][q]));
    const float dz_im = fmaf(dc.c_re, G[1][q], fmaf(dc.c_cr, G[3][q], dc.c_im * G[5][q]));
    r2[q] = fmaf(dz_re, dz_re, dz_im * dz_im);
    const float f = fmaf(r2[q], fmaf(r2[q], fmaf(r2[q], fmaf(r2[q], 35.0f / 1152.0f, 15.0f / 336.0f), 3.0f / 40.0f), 1.0f / 6.0f), 1.0f);
    far |= r2[q] >= 0.01f;
    ox[q] = -dz_re * f;
    oy[q] = -dz_im * f;
  }
  if (__builtin_amdgcn_ballot_w64(far) != 0) {  // beyond 0.1 rad of the map's centre: asin(r)/r itself instead of its series
#pragma unroll 1
    for (int q = 0; q < kN; ++q) {
      const float x = r2[q];
      if (x >= 0.01f) {
        const float series = fmaf(x, fmaf(x, fmaf(x, fmaf(x, 35.0f / 1152.0f, 15.0f / 336.0f), 3.0f / 40.0f), 1.0f / 6.0f), 1.0f);
        const float r = sqrtf(x);
        const float ratio = (asinf(fminf(r, 1.0f)) / r) / series;
#pragma unroll
        for (int k = 0; k < kN; ++k) {  // (registers, not an indexed array)
          ox[k] = k == q ? ox[k] * ratio : ox[k];
          oy[k] = k == q ? oy[k] * ratio : oy[k];
        }
      }
    }
  }
  int o0[kN];
  float w0a[kN], w0b[kN], w1a[kN], w1b[kN];
#pragma unroll
  for (int q = 0; q < kN; ++q) {
    int e0, x0;
    float pe, px;
    axis_cell_t<kBil>(ax_eta, oy[q], e0, pe);
    axis_cell_t<kBil>(ax_xi, ox[q], x0, px);
    const float qe = 1.0f - pe, qx = 1.0f - px;
    w0a[q] = qe * qx; w0b[q] = qe * px; w1a[q] = pe * qx; w1b[q] = pe * px;
    o0[q] = (int)(__umul24((unsigned)e0, (unsigned)g.n_xi) + (unsigned)x0) << 3;  // (e0 < n_eta, n_xi < 2^24): the cell's 16 bytes in its plane of pairs
  }
  typedef float quad4 __attribute__((ext_vector_type(4)));
  const int plane8 = ((g.n_eta - 1) * g.n_xi) << 3;  // a plane of row pairs, bytes
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)g.pairs, 0, (int)g.pairs_bytes, 0x00020000);
#pragma unroll
  for (int q = 0; q < kN; ++q) out[q] = 0.0f;
  float wf[kS];  // the Stokes weights as the float32 numbers the sums take
#pragma unroll
  for (int k = 0; k < kS; ++k) wf[k] = (float)dc.w[k];
  auto channel = [&](int c, bool first_channel) {
    float val[kN];
#pragma unroll
    for (int k = 0; k < kS; ++k) {  // (a plane's kN gathers in flight together; all kS planes' at once would not fit the registers)
      const int soff = (c * kS + k) * plane8;
      quad4 cn[kN];  // (m[e0][x0], m[e0 + 1][x0], m[e0][x0 + 1], m[e0 + 1][x0 + 1])
#pragma unroll
      for (int q = 0; q < kN; ++q) cn[q] = __builtin_bit_cast(quad4, __builtin_amdgcn_raw_buffer_load_b128(rs, o0[q], soff, 0));
#pragma unroll
      for (int q = 0; q < kN; ++q) {
        const float v = fmaf(w0a[q], cn[q].x, fmaf(w0b[q], cn[q].z, fmaf(w1a[q], cn[q].y, w1b[q] * cn[q].w)));
        val[q] = k == 0 ? wf[k] * v : fmaf(wf[k], v, val[q]);
      }
    }
    float f[kN];
    pw(c, f);
#pragma unroll
    for (int q = 0; q < kN; ++q)
      out[q] = first_channel ? f[q] * val[q] : fmaf(f[q], val[q], out[q]);  // float32 accumulator (map.py:155)
  };
  if (kUnrollC) {
#pragma unroll
    for (int c = 0; c < kCalFastChannels; ++c)
      if (c < g.C) channel(c, c == 0);  // (uniform)
  } else {
    for (int c = 0; c < g.C; ++c) channel(c, false);
  }
}

// pairs[plane][e][x] = (m[e][x], m[e + 1][x]) (MapArgs::pairs), one thread per pair
__global__ __launch_bounds__(kBlock) void map_pairs_kernel(const float* __restrict__ m, float2* __restrict__ pairs, int planes, int n_eta, int n_xi) {
  const size_t per = (size_t)(n_eta - 1) * n_xi, n = per * planes;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    const size_t p = i / per, r = i - p * per;
    const float* src = m + p * (size_t)n_eta * n_xi + r;
    pairs[i] = make_float2(src[0], src[n_xi]);
  }
}

// ---- the stages of map_sample_kernel, in the order in which it runs them (stages 2 and 4 stand in its body) ----

// the thread's place in its tile of 1024 samples
struct TilePos {
  int s_tile, sb;    // the tile's first sample and the thread's first of four
  bool first, last;  // the tile's first and last thread: they evaluate the halo samples of the 3-tap kernel
};

// Stage 1, the calibration.  Reads the tables and their axes (kCal) or the caller's scalars from global memory; leaves
// them at the start of the dynamic LDS (axes, then [C][n_pwv][n_el]; or [C] factors in pW per K_RJ).  No barrier: the
// kernel's barrier behind stage 2 covers it, and cal_view (which reads the axes' ends) comes after that.
template <bool kCal>
__device__ __forceinline__ void stage_cal_tables(const MapArgs& g, float* cal_lds) {
  if (kCal) {
    for (int i = threadIdx.x; i < g.n_pwv; i += kBlock) cal_lds[i] = g.cal_pwv[i];
    for (int i = threadIdx.x; i < g.n_el; i += kBlock) cal_lds[g.n_pwv + i] = g.cal_el[i];
    for (int i = threadIdx.x; i < g.C * g.n_pwv * g.n_el; i += kBlock) cal_lds[g.n_pwv + g.n_el + i] = g.cal[i];
  } else {
    // (once per workgroup: per sample and channel this was a float64 product and a conversion)
    for (int i = threadIdx.x; i < g.C; i += kBlock) cal_lds[i] = (float)(1.380649e-11 * g.scalar[i]);
  }
}

template <bool kCal>
__device__ __forceinline__ CalLds cal_view(const MapArgs& g, const float* cal_lds) {
  CalLds cl{};
  if (kCal) {
    cl.pwv = make_rgi_axis(cal_lds, g.n_pwv);
    cl.el = make_rgi_axis(cal_lds + g.n_pwv, g.n_el);
    cl.tab = cal_lds + g.n_pwv + g.n_el;
  } else {
    cl.chan = cal_lds;
  }
  return cl;
}

// the record of a slot for the per-sample form under the composed pointing: with the tables (kCal) the calibration's part
// is recomputed (sample_const's arithmetic; the pwv's place in its step demoted to float32)
template <bool kCal>
__device__ __forceinline__ SampleConst slot_record(const MapArgs& g, int s_tile, const RecordLds& rec, int slot) {
  SampleConst one = rec.record(slot);
  if (kCal) {
    const int sidx = min(max(s_tile - 1 + slot, 0), g.T - 1);
    const float a = __fsub_rn(g.el[sidx], kHalfPiF);
    one.ca = cosf(a);
    one.sa = sinf(a);
    double u;
    one.jj = coarse_step(g, g.t[sidx], u);
    one.u = (double)(float)u;
  }
  return one;
}

// Stage 3, the interval form of the per-sample calibration (round 6).  The factor -- pW per K_RJ at the sample's zenith
// pwv and the detector's elevation, per channel -- along a row: the pwv is piecewise LINEAR between the coarse samples
// (0.1 s; sim/atmosphere.py:30-37), the elevation a smooth scan.  Inside one coarse step the factor is therefore smooth,
// and its kinks sit at the steps' ends.  So it is looked up ONCE per row at the start, the middle and the end of every
// coarse step the tile meets (16 rows x ~26 steps x 3 lookups a group, five a thread, all of a thread's in flight
// together), kept in LDS as the parabola through the three in the step's own coordinate, and a sample evaluates its
// step's parabola at its place in the step: the kinks are where the reference has them, the elevation's curvature inside
// a step is the parabola's (what is left is the third difference over 0.1 s: below 1e-8 of the factor), and a kink of the
// TABLES inside a step is missed by less than 1e-7 of the factor.  Rounds 3-5 looked the factor up per thread and row (at
// its first sample; a lane shuffle for the chord to the next thread's): a chain of LDS reads, two global loads and a
// barrier per ROW -- a third of the kernel's instructions and most of its waiting.  The form applies to whole tiles
// that meet at most coef_cap steps (the launcher's table; mrx_map_cal.steps_per_tile) of at least eight samples; a row
// with a knot off the tables (NaN: jax's fill) takes the per-sample form, which marks exactly the samples that are off.
struct IntervalCal {
  bool ok = false;          // the form applies to this tile (workgroup-uniform)
  int j_lo = 0, n_int = 0;  // the first coarse step the tile meets, and how many
  int rb = 0;               // the step of the thread's earliest sample, counted from j_lo
  float v0 = 0.0f, dvt = 0.0f, lim = 1.0f;  // the thread's samples in units of a step (tile), and where the next step begins
  float* coef;      // the parabola records, [channel][row][step][3] with row pitch `pitch` floats (dynamic LDS)
  int pitch;
  float2* knot_cs;  // (cos, sin) of (boresight elevation - pi/2) at the start, the middle and the end of every step (LDS)
  int* bad_row;     // per row of the group: a knot off the tables (LDS)

  static __device__ __forceinline__ int step_of(const MapArgs& g, int sidx, double& u) {
    return coarse_step(g, g.t[min(max(sidx, 0), g.T - 1)], u);
  }

  // The tile's part.  Reads the sample times and the boresight elevation around the tile (global); leaves ok, the
  // thread's place in the steps (registers) and, where ok, knot_cs.  No barrier: the group loop's two come before
  // knot_cs is read.
  __device__ __forceinline__ void tile(const MapArgs& g, const TilePos& t) {
    double u_lo, u_hi;
    j_lo = step_of(g, t.s_tile - 1, u_lo);
    n_int = step_of(g, t.s_tile + kTileSamples, u_hi) - j_lo + 1;
    ok = g.coef_offset >= 0 && t.s_tile + kTileSamples <= g.T && n_int <= min(g.coef_cap, kMaxSteps) && n_int * 8 <= kTileSamples;  // (uniform)
    if (!ok) return;
    // the thread's samples in units of a step, counted from the start of the step of its earliest sample (the first
    // thread's halo): v0 at its first sample, dvt a sample (the samples are evenly spaced over a thread's 10 ms)
    double u_b, u_0, u_3;
    const int jb = step_of(g, t.first ? t.s_tile - 1 : t.sb, u_b), j0 = step_of(g, t.sb, u_0), j3 = step_of(g, t.sb + kSamplesPerThread - 1, u_3);
    v0 = (float)((double)(j0 - jb) + u_0);
    dvt = (float)(((double)(j3 - jb) + u_3 - ((double)(j0 - jb) + u_0)) * (1.0 / (kSamplesPerThread - 1)));
    lim = jb >= g.Ta - 2 ? 3.0e38f : 1.0f;  // (past the last coarse sample the series is extrapolated: still the last step)
    rb = jb - j_lo;
    // the boresight at the steps' starts, middles and ends: linear between the two samples around the knot's time
    const int s_a = max(t.s_tile - 1, 0), s_b = min(t.s_tile + kTileSamples, g.T - 1);
    const double t_a = g.t[s_a], inv_dt = (double)(s_b - s_a) / (g.t[s_b] - t_a);
    for (int m = threadIdx.x; m < 2 * n_int + 1; m += kBlock) {
      const double tau = g.ta0 + ((double)j_lo + 0.5 * (double)m) * g.dta;
      int sidx = min(max(s_a + (int)floor(fmin(fmax((tau - t_a) * inv_dt, -2.0e9), 2.0e9)), 0), g.T - 2);
      for (int it = 0; it < 8 && sidx < g.T - 2 && g.t[sidx + 1] < tau; ++it) ++sidx;  // (unevenly spaced samples)
      for (int it = 0; it < 8 && sidx > 0 && g.t[sidx] > tau; ++it) --sidx;
      const double wt = (tau - g.t[sidx]) / (g.t[sidx + 1] - g.t[sidx]);
      const float e0 = g.el[sidx], e1 = g.el[sidx + 1];
      const float a = __fsub_rn((float)((double)e0 + wt * ((double)e1 - (double)e0)), kHalfPiF);
      knot_cs[m] = make_float2(cosf(a), sinf(a));
    }
  }

  // (between the group's two barriers)
  __device__ __forceinline__ void clear_rows() const {
    if ((int)threadIdx.x < kTileDet) bad_row[threadIdx.x] = 0;
  }

  // The group's part.  Reads the rows' constants (dets, LDS), knot_cs, the tables (cl, LDS) and the rows' coarse pwv
  // (global); leaves the rows' parabola records in coef and bad_row.  Ends with a barrier where the form applies.
  __device__ __forceinline__ void group(const MapArgs& g, const CalLds& cl, const DetConst* dets, int d0, int nd) const {
    if (!ok) return;
    for (int i = threadIdx.x; i < kTileDet * n_int; i += kBlock) {
      const int dl = i & (kTileDet - 1), r = i / kTileDet;
      if (dl >= nd) continue;
      const int j = j_lo + r, d = d0 + dl;
      const double y0 = g.pwv[(size_t)j * g.D + d], y1 = g.pwv[(size_t)(j + 1) * g.D + d];
      float F[3][kCalFastChannels];
      bool bad = false;
#pragma unroll
      for (int k = 0; k < 3; ++k) {  // the step's start, middle and end
        const float2 cs = knot_cs[2 * r + k];
        const float im = __fadd_rn(__fmul_rn(dets[dl].c_re, cs.y), __fmul_rn(dets[dl].c_cr, cs.x));
        const CalCell cell = cal_cell(cl, (float)fma(0.5 * (double)k, y1 - y0, y0), asin_poly(im));  // (pwv demoted to float32 by the jax interpolator)
#pragma unroll
        for (int c = 0; c < kCalFastChannels; ++c) {
          F[k][c] = 0.0f;
          if (c < g.C) {  // (uniform)
            F[k][c] = cal_factor(g, cl, cell, c);
            bad |= !(F[k][c] == F[k][c]);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < kCalFastChannels; ++c)
        if (c < g.C) {  // the parabola through (0, F0), (1/2, F1), (1, F2): F0 + w (4 F1 - 3 F0 - F2) + w^2 (2 F0 + 2 F2 - 4 F1)
          float* rec = coef + (c * kTileDet + dl) * pitch + 3 * r;
          rec[0] = F[0][c];
          rec[1] = fmaf(4.0f, F[1][c], fmaf(-3.0f, F[0][c], -F[2][c]));
          rec[2] = fmaf(-4.0f, F[1][c], 2.0f * (F[0][c] + F[2][c]));
        }
      if (bad) bad_row[dl] = 1;
    }
    __syncthreads();
  }

  // the form applies to row dl of the group (uniform)
  __device__ __forceinline__ bool row_ok(int dl) const { return ok && __builtin_amdgcn_readfirstlane(bad_row[dl]) == 0; }

  // The evaluation: f[q] = channel c's factor at the thread's sample q of row dl (q = 4: the halo sample, at place q_halo
  // among the thread's).  The sample's place in its coarse step: v counts from the start of the thread's first step; past
  // 1 it is the next step's (one record on).  The tile has n_int records: a v that float32 rounds up to 1 in the last
  // step (a float64 u of 1 - 1e-14) keeps that step's record, whose parabola at w = 1 is the next step's start.
  template <int n>
  __device__ __forceinline__ void factor(int c, int dl, float q_halo, float (&f)[n]) const {
    const float* cf = coef + (c * kTileDet + dl) * pitch + 3 * rb;
#pragma unroll
    for (int q = 0; q < n; ++q) {
      const float v = fmaf(q == 4 ? q_halo : (float)q, dvt, v0);
      const bool next = v >= lim && rb + 1 < n_int;
      const float w = next ? v - 1.0f : v;
      const float* rec = next ? cf + 3 : cf;
      f[q] = fmaf(w, fmaf(w, rec[2], rec[1]), rec[0]);
    }
  }
};

// Stage 5, the 3-tap filter along time.  Reads r and halo; trades the thread's first and last value with its neighbours
// through edge (LDS; ONE barrier, between the write and the reads -- the caller alternates two buffers from row to row, so
// none is needed behind the reads); leaves o.
__device__ __forceinline__ void filter3(float2* edge, const TilePos& t, const float (&r)[kSamplesPerThread], float halo,
                                        float (&o)[kSamplesPerThread]) {
  edge[threadIdx.x] = make_float2(r[0], r[kSamplesPerThread - 1]);
  __syncthreads();
  const float left = t.first ? halo : edge[threadIdx.x - 1].y;
  const float right = t.last ? halo : edge[threadIdx.x + 1].x;
  // scipy.ndimage.convolve1d, symmetric 3-tap kernel (map.py:170): 0.5 r + 0.25 (prev + next); the
  // float32 form differs from scipy's float64 accumulation by one rounding of the float32 result
#pragma unroll
  for (int q = 0; q < kSamplesPerThread; ++q) {
    const float prev = q == 0 ? left : r[q - 1];
    const float next = q == kSamplesPerThread - 1 ? right : r[q + 1];
    o[q] = fmaf(r[q], 0.5f, (prev + next) * 0.25f);
  }
}

// Stage 6, the store: the thread's four values of row d, as 16 bytes where the row is aligned and whole
__device__ __forceinline__ void store_row(const MapArgs& g, int d, int sb, bool full, const float (&o)[kSamplesPerThread]) {
  float* dst = g.out + (size_t)d * g.ld + sb;
  if (full) {
    const vfloat4 v = {o[0], o[1], o[2], o[3]};
    __builtin_nontemporal_store(v, reinterpret_cast<vfloat4*>(dst));
  } else {
#pragma unroll
    for (int q = 0; q < kSamplesPerThread; ++q)
      if (sb + q < g.T) dst[q] = o[q];
  }
}

#ifndef MRX_MAP_CAL_WAVES
#define MRX_MAP_CAL_WAVES 4
#endif
// kKrj: the field leaves in K_RJ -- every row's four values times the row's scale, divided by den_band(el_det) exactly as
// tod_krj_kernel divides a finished field (mrx_krj.h: the same per-tile elevation model from the same 1024 samples, the same
// lookup), instead of a second pass that reads and writes the field again (3.9 of 18.3 ms at 10 000 x 240 000).
// Without the per-sample atmospheric calibration the kernel fits 168 registers (three waves per
// SIMD: 16.8 -> 14.8 ms at 10 000 x 240 000); with it the cap costs spills (26.8 -> 34.4 ms).
// Stages 2 (the sample records) and 4 (a row's raw values) stand in the body, the second with its two lambdas: as
// functions they compile to other code, with more registers and spills (DESIGN 3.39 has the numbers).
template <bool kChain, bool kCal, int kS, bool kKrj = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kChain ? (kCal ? 2 : 3) : (kCal ? MRX_MAP_CAL_WAVES : kS == 1 ? 5 : 4), kChain ? (kCal ? 2 : 3) : 8))) void map_sample_kernel(MapArgs g, int groups, MapKrj kj) {
  __shared__ DetConst dets[kTileDet];
  __shared__ float2 edge[2][kBlock];  // (first, last) raw value of every thread, double-buffered
  extern __shared__ __align__(16) float cal_lds[];   // calibration axes and tables (a few KB), the interval table; K_RJ: the cell table behind them
  __shared__ CalDet cdet[kKrj ? kTileDet : 1];
  __shared__ float red[12];
  stage_cal_tables<kCal>(g, cal_lds);
  const int s_tile = blockIdx.x * kTileSamples;
  const int sb = s_tile + threadIdx.x * kSamplesPerThread;
  const Axis ax_eta = g.eta, ax_xi = g.xi;
  // Stage 2, the sample records.  The per-sample part (float64 composition of the three rotations, ~500 instruction
  // slots a sample) is shared by the `groups` x 16 detector rows this workgroup walks.  Composed pointing: reads az, el and
  // the transform of the tile's 1026 samples, leaves their records in LDS (RecordLds), where the row loop fetches them --
  // instead of five records held in 65 registers per thread (168 -> 63 registers).  The literal chain: the thread's four
  // records and, in the tile's first and last thread, the halo sample's stay in registers.  Ends with the barrier below.
  constexpr bool kLdsSc = !kChain;
  __shared__ __align__(16) float sc_lds[kLdsSc ? kRec * kRecPitch : 8];
  __shared__ float2 knot_cs[kLdsSc && kCal ? 2 * kMaxSteps + 1 : 1];  // IntervalCal's
  __shared__ int bad_row[kLdsSc && kCal ? kTileDet : 1];
  SampleConst sc[kSamplesPerThread], sc_halo;
  const bool first = threadIdx.x == 0, last = threadIdx.x == kBlock - 1;
  if (kLdsSc) {
    for (int i = threadIdx.x; i < kTileSamples + 2; i += kBlock) {
      SampleConst one;
      sample_const(g, s_tile - 1 + i, false, one);
#pragma unroll
      for (int k = 0; k < kRec; ++k) sc_lds[k * kRecPitch + i + 3] = one.G[k];
    }
  } else {
#pragma unroll
    for (int q = 0; q < kSamplesPerThread; ++q) {
      sample_const(g, sb + q, kChain, sc[q]);
      sc[q].s = min(max(sb + q, 0), g.T - 1);
    }
    if (first || last) {
      const int sh = first ? s_tile - 1 : s_tile + kTileSamples;
      sample_const(g, sh, kChain, sc_halo);
      sc_halo.s = min(max(sh, 0), g.T - 1);
    }
  }
  float4* const cal_cells = reinterpret_cast<float4*>(cal_lds) + kj.cells_offset;
  KrjSamples ks{};
  if constexpr (kKrj) ks = krj_prologue(cal_cells, red, kj.bore_el, g.T, sb, kj.cal_axis, kj.cal_values, kj.n_el, kj.n_bands);  // (ends with a barrier)
  __syncthreads();
  const CalLds cl = cal_view<kCal>(g, cal_lds);
  const RecordLds rec{sc_lds};
  const bool full = (sb + kSamplesPerThread <= g.T) && g.vec_ok;
  const TilePos t = {s_tile, sb, first, last};
  IntervalCal ic;
  ic.coef = cal_lds + (g.coef_offset >= 0 ? g.coef_offset : 0);
  ic.pitch = 3 * g.coef_cap + 1;
  ic.knot_cs = knot_cs;
  ic.bad_row = bad_row;
  if constexpr (kCal && kLdsSc) ic.tile(g, t);
  for (int grp = 0; grp < groups; ++grp) {
    const int d0 = (blockIdx.y * groups + grp) * kTileDet;
    if (d0 >= g.D) break;
    const int nd = min(kTileDet, g.D - d0);
    __syncthreads();  // the previous group is done with dets[], cdet[] and edge[]
    if ((int)threadIdx.x < nd) dets[threadIdx.x] = make_det_const(g, d0 + threadIdx.x);
    if constexpr (kCal && kLdsSc) ic.clear_rows();
    if constexpr (kKrj) krj_stage_rows(cdet, red, kj.dx, kj.dy, kj.band, kj.scale, kj.n_bands, d0, nd, cal_cells, kj.n_el);
    __syncthreads();
    if constexpr (kCal && kLdsSc) ic.group(g, cl, dets, d0, nd);
    for (int dl = 0; dl < nd; ++dl) {
      const DetConst dc = dets[dl];
      const int d = d0 + dl;
      // Stage 4, the row's raw (unconvolved) values: r, and halo in the tile's first and last thread.  No barrier.
      float r[kSamplesPerThread];
      float halo = 0.0f;
      // The batched form (round 6): the thread's four samples TOGETHER (row_samples: their LDS reads, then their gathers,
      // in flight at once); the tile's halo samples ride along as a fifth sample of waves 0 and 3 (in a branch of their
      // own the first and the last thread's waves ran a whole sample's chain of latencies alone, once per row)
      auto batched = [&](auto unroll_c, auto pw) {
        const int s0 = 1 + threadIdx.x * kSamplesPerThread;
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        auto run = [&](auto bil) {
          if (wave == 0 || wave == kBlock / 64 - 1) {
            const int slot[5] = {s0, s0 + 1, s0 + 2, s0 + 3, first ? 0 : last ? kTileSamples + 1 : s0 + 3};
            float v[5];
            row_samples<decltype(bil)::value, kS, 5, decltype(unroll_c)::value>(g, ax_eta, ax_xi, dc, slot, rec, pw, v);
            r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[3];
            halo = v[4];
          } else {
            const int slot[4] = {s0, s0 + 1, s0 + 2, s0 + 3};
            row_samples<decltype(bil)::value, kS, 4, decltype(unroll_c)::value>(g, ax_eta, ax_xi, dc, slot, rec, pw, r);
          }
        };
        if (g.bilinear) run(std::true_type{}); else run(std::false_type{});  // (uniform)
      };
      if constexpr (kLdsSc && !kCal) {
        // composed pointing, the caller's scalar factors (LDS): batched, the same factor at every sample
        batched(std::false_type{}, [&](int c, auto& f) {
          const float v = cl.chan[c];
          constexpr int n = sizeof(f) / sizeof(f[0]);
#pragma unroll
          for (int q = 0; q < n; ++q) f[q] = v;
        });
      } else if (kLdsSc && ic.row_ok(dl)) {  // (uniform)
        // composed pointing, the tables: batched on the interval form, where it applies to the tile and the row.
        // The halo's place in the thread's samples: one before the first, one after the last -- or, where that index is
        // clamped to the run's ends (the per-sample form's rule, scipy's 'reflect'), the end sample itself
        const float q_halo = first ? (s_tile > 0 ? -1.0f : 0.0f) : (s_tile + kTileSamples < g.T ? 4.0f : 3.0f);
        batched(std::true_type{}, [&](int c, auto& f) { ic.factor(c, dl, q_halo, f); });
      } else {
        // per sample: the literal chain, more than kCalFastChannels channels, a ragged last tile, a tile that meets too
        // many or too short coarse steps, a row with a knot off the tables
        int jj0 = -1;  // (the coarse pwv pair the caller holds: none -- raw_sample loads the sample's own)
        double y0 = 0.0, y1 = 0.0;
        if (kCal && !kLdsSc) {
          jj0 = sc[0].jj;
          y0 = g.pwv[(size_t)jj0 * g.D + d];
          y1 = g.pwv[(size_t)(jj0 + 1) * g.D + d];
        }
        auto rec_of = [&](int slot) { return slot_record<kCal && kLdsSc>(g, s_tile, rec, slot); };
        if constexpr (kLdsSc) {
          // (one sample at a time, not unrolled: this form is the exception, and four samples of it side by side set the
          // whole kernel's register count -- 138 against the batched form's own need)
#pragma unroll 1
          for (int q = 0; q < kSamplesPerThread; ++q) {
            const float v = raw_sample<kChain, kCal, kS>(g, cl, ax_eta, ax_xi, dc, d, rec_of(1 + threadIdx.x * kSamplesPerThread + q), jj0, y0, y1);
            r[0] = q == 0 ? v : r[0]; r[1] = q == 1 ? v : r[1]; r[2] = q == 2 ? v : r[2]; r[3] = q == 3 ? v : r[3];
          }
        } else {
#pragma unroll
          for (int q = 0; q < kSamplesPerThread; ++q)
            r[q] = raw_sample<kChain, kCal, kS>(g, cl, ax_eta, ax_xi, dc, d, sc[q], jj0, y0, y1);
        }
        if (first || last)
          halo = raw_sample<kChain, kCal, kS>(g, cl, ax_eta, ax_xi, dc, d, kLdsSc ? rec_of(first ? 0 : kTileSamples + 1) : sc_halo, jj0, y0, y1);
      }
      float o[kSamplesPerThread];
      filter3(edge[dl & 1], t, r, halo, o);
      if constexpr (kKrj) {
        const CalDet c = cdet[dl];
        float sv[kSamplesPerThread];
#pragma unroll
        for (int q = 0; q < kSamplesPerThread; ++q) sv[q] = c.scale * o[q];
        const float4* C = cal_cells + c.band * (kj.n_el - 1);
        krj_row<false>(c, C, kj.n_el, ks, sv, o, kj.bore_el, sb, g.T, cal_cells, kj.cal_axis);
      }
      store_row(g, d, sb, full, o);
    }
  }
}

}  // namespace

// The sampler's dynamic LDS: the calibration tables (or the channels' scalar factors), behind them the interval table of
// the per-sample calibration, behind that -- on a 16-byte boundary -- the cell table of TOD.to("K_RJ")
struct SampleLds {
  size_t table_bytes;  // the tables with their axes, or the scalar factors
  int coef_offset;     // MapArgs::coef_offset, in floats; -1: no interval table
  int coef_cap;        // MapArgs::coef_cap
  int cells_offset;    // MapKrj::cells_offset, in float4
  size_t bytes;        // all of it
};

static SampleLds sample_lds(const mrx_sky_map* map, const mrx_map_cal* cal, const MapKrj* krj, int T) {
  SampleLds l{0, -1, 0, 0, 0};
  const size_t krj_bytes = krj ? sizeof(float4) * (size_t)(krj->n_el - 1) * krj->n_bands : 0;
  if (cal->d_table) {
    l.table_bytes = sizeof(float) * ((size_t)cal->n_pwv + cal->n_el + (size_t)map->n_channels * cal->n_pwv * cal->n_el);
    l.bytes = l.table_bytes;
    // the interval table -- not where no tile can use it (a tile that meets more than kMaxSteps steps takes the per-sample
    // form), nor where it would push the K_RJ form's tables past their 60 KiB
    const int cap = cal->steps_per_tile > 0 ? std::min(cal->steps_per_tile, kMaxSteps) : kDefaultSteps;
    const size_t coef_bytes = sizeof(float) * (size_t)map->n_channels * kTileDet * (3 * cap + 1);
    if (map->n_channels <= kCalFastChannels && T >= 2 && cal->steps_per_tile <= kMaxSteps &&
        (!krj || (l.bytes + coef_bytes + 15) / 16 * 16 + krj_bytes <= 60 * 1024)) {
      l.coef_cap = cap;
      l.coef_offset = (int)(l.bytes / sizeof(float));
      l.bytes += coef_bytes;
    }
  } else {
    l.table_bytes = l.bytes = sizeof(float) * (size_t)map->n_channels;
  }
  if (krj) {
    l.bytes = (l.bytes + 15) / 16 * 16;
    l.cells_offset = (int)(l.bytes / 16);
    l.bytes += krj_bytes;
  }
  return l;
}

// The map's row pairs (MapArgs::pairs) for the composed pointing: the context's copy, grown on demand, filled on the
// stream behind the sampler that last read it.  The caller records map_pairs_read behind its own launch.
static int map_pairs(mrx_ctx* ctx, const mrx_sky_map* map, MapArgs& g) {
  const int planes = map->n_channels * map->n_stokes;
  const unsigned long long bytes = 8ull * (unsigned long long)planes * (map->n_eta - 1) * map->n_xi;  // (below 4 GiB: checked)
  if (!ctx->map_pairs_read) MRX_HIP(ctx, hipEventCreateWithFlags(&ctx->map_pairs_read, hipEventDisableTiming));
  else MRX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->map_pairs_read, 0));  // (the sampler that last read the copy)
  if (ctx->map_pairs_cap < bytes) {  // (grown on demand: rare)
    if (ctx->d_map_pairs) {
      MRX_HIP(ctx, hipDeviceSynchronize());
      (void)hipFree(ctx->d_map_pairs);
      ctx->d_map_pairs = nullptr;
      ctx->map_pairs_cap = 0;
    }
    MRX_HIP(ctx, hipMalloc(&ctx->d_map_pairs, (size_t)bytes));
    ctx->map_pairs_cap = (size_t)bytes;
  }
  const unsigned long long n_pairs = bytes / 8;
  const unsigned blocks = (unsigned)std::min<unsigned long long>((n_pairs + kBlock - 1) / kBlock, 65536ull);
  hipLaunchKernelGGL(map_pairs_kernel, dim3(blocks), dim3(kBlock), 0, ctx->stream, map->d_values, reinterpret_cast<float2*>(ctx->d_map_pairs),
                     planes, map->n_eta, map->n_xi);
  g.pairs = ctx->d_map_pairs;
  g.pairs_bytes = (uint32_t)bytes;
  return MRX_OK;
}

// the kernel's instance for the map's Stokes planes, launched
template <bool kChain, bool kCal, bool kKrj>
static int launch_sample(mrx_ctx* ctx, dim3 grid, size_t lds, const MapArgs& g, int groups, const MapKrj& kj) {
  void (*const kernel)(MapArgs, int, MapKrj) = g.S == 1   ? map_sample_kernel<kChain, kCal, 1, kKrj>
                                               : g.S == 2 ? map_sample_kernel<kChain, kCal, 2, kKrj>
                                               : g.S == 3 ? map_sample_kernel<kChain, kCal, 3, kKrj>
                                                          : map_sample_kernel<kChain, kCal, 4, kKrj>;
  // (the kernel's static LDS -- sample records, edge exchange -- is up to 46 KiB: with large calibration
  // tables the sum passes the 64 KiB a launch gets by default)
  if (lds + 48 * 1024 > 64 * 1024)
    MRX_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, dim3(kBlock), lds, ctx->stream, g, groups, kj);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

// mrx_map_sample (krj == nullptr) and mrx_map_sample_krj: the checks, the LDS layout, the row pairs, the launch.
// (The checks stand here and not in a function of their own: a message names the function that raises it.)
static int map_sample(mrx_ctx* ctx, const mrx_sky_map* map, const mrx_map_cal* cal,
                      const float* d_az, const float* d_el, int T, const double* d_transform,
                      const float* d_dx, const float* d_dy, const double* d_stokes_w, int D,
                      float* d_out, size_t ld_out, const MapKrj* krj) {
  MRX_REQUIRE(ctx, D >= 0 && T >= 0, "negative size");
  if (D == 0 || T == 0) return MRX_OK;
  MRX_REQUIRE(ctx, map && cal && d_az && d_el && d_dx && d_dy && d_stokes_w && d_out, "null pointer");
  MRX_REQUIRE(ctx, map->d_values, "null map pointer");
  MRX_REQUIRE(ctx, map->deta != 0.0 && map->dxi != 0.0, "map axes need a non-zero step");
  MRX_REQUIRE(ctx, map->n_channels >= 1 && map->n_stokes >= 1 && map->n_stokes <= kMaxStokes &&
                       map->n_eta >= 2 && map->n_xi >= 2,
              "need n_channels >= 1, 1 <= n_stokes <= 4, n_eta >= 2, n_xi >= 2");
  MRX_REQUIRE(ctx, ld_out >= (size_t)T, "ld_out smaller than T");
  const bool chain = ctx->options[MRX_OPT_POINTING_CHAIN] != 0, has_cal = cal->d_table != nullptr;
  if (has_cal) {
    MRX_REQUIRE(ctx, cal->d_axis_pwv && cal->d_axis_el && cal->d_pwv && cal->d_t, "null calibration pointer");
    MRX_REQUIRE(ctx, cal->n_pwv >= 2 && cal->n_el >= 2 && cal->Ta >= 2 && cal->dta > 0.0,
                "calibration needs n_pwv >= 2, n_el >= 2, Ta >= 2, dta > 0");
  } else {
    MRX_REQUIRE(ctx, cal->d_scalar, "need a per-channel scalar calibration without a table");
  }
  // (the sampler reads the map as ONE raw buffer: 32-bit offsets)
  const unsigned long long map_bytes = 4ull * (unsigned long long)map->n_channels * map->n_stokes * map->n_eta * map->n_xi;
  MRX_REQUIRE(ctx, map_bytes < (1ull << 32), "the map (all channels and Stokes planes) must be smaller than 4 GiB");
  // detector tiles per workgroup (they share the per-sample constants): MRX_MAP_GROUPS while that leaves >= 16
  // workgroups per CU in the grid
#ifndef MRX_MAP_GROUPS
#define MRX_MAP_GROUPS 4
#endif
  int groups = MRX_MAP_GROUPS;
  while (groups > 1 && (long long)mrx_ceil_div(T, kTileSamples) * mrx_ceil_div(D, kTileDet * groups) < 16LL * 256) groups /= 2;
  const dim3 grid(mrx_ceil_div(T, kTileSamples), mrx_ceil_div(D, kTileDet * groups));
  MRX_REQUIRE(ctx, grid.y <= 65535u, "D too large for one launch");
  const SampleLds lds = sample_lds(map, cal, krj, T);
  MRX_REQUIRE(ctx, lds.table_bytes <= 48 * 1024, has_cal ? "calibration tables of all channels must fit in 48 KiB" : "too many channels");
  MRX_REQUIRE(ctx, !krj || lds.bytes <= 60 * 1024, "the calibration tables (sampling and K_RJ) must fit in 60 KiB");
  MRX_REQUIRE(ctx, (long long)map->n_eta * map->n_xi < (1LL << 29), "a map plane must hold fewer than 2^29 pixels");
  MRX_REQUIRE(ctx, map->n_eta < (1 << 23) && map->n_xi < (1 << 23) && std::fabs(map->eta0 / map->deta) < 8388608.0 &&
                       std::fabs(map->xi0 / map->dxi) < 8388608.0,
              "a map axis must have fewer than 2^23 nodes and start within 2^23 pixels of the map's centre");
  MRX_REQUIRE(ctx, chain || 8ull * map->n_channels * map->n_stokes * (map->n_eta - 1) * map->n_xi < (1ull << 32),
              "the map (all channels and Stokes planes) must be smaller than 2 GiB (its row pairs than 4 GiB)");
  if (krj && chain)
    return mrx_fail(ctx, MRX_ERR_UNSUPPORTED, "mrx_map_sample_krj: not with MRX_OPT_POINTING_CHAIN (sample in pW, then mrx_tod_to_krj)");

  MapArgs g = map_args(map, d_az, d_el, T, d_transform, d_dx, d_dy, d_stokes_w, D);
  g.values = map->d_values;
  g.map_bytes = (uint32_t)map_bytes;
  g.cal = cal->d_table;
  g.cal_pwv = cal->d_axis_pwv;
  g.cal_el = cal->d_axis_el;
  g.n_pwv = cal->n_pwv;
  g.n_el = cal->n_el;
  g.pwv = cal->d_pwv;
  g.Ta = cal->Ta;
  g.ta0 = cal->ta0;
  g.dta = cal->dta;
  g.inv_dta = cal->dta > 0.0 ? 1.0 / cal->dta : 0.0;
  g.t = cal->d_t;
  g.scalar = cal->d_scalar;
  g.out = d_out;
  g.ld = ld_out;
  g.vec_ok = (ld_out % 4 == 0) && ((reinterpret_cast<uintptr_t>(d_out) & 15u) == 0);
  g.coef_offset = lds.coef_offset;
  g.coef_cap = lds.coef_cap;
  MapKrj kj{};
  if (krj) kj = *krj;
  kj.cells_offset = lds.cells_offset;
  if (!chain) {
    const int rc = map_pairs(ctx, map, g);
    if (rc != MRX_OK) return rc;
  }
  const int rc = chain     ? (has_cal ? launch_sample<true, true, false>(ctx, grid, lds.bytes, g, groups, kj)
                                      : launch_sample<true, false, false>(ctx, grid, lds.bytes, g, groups, kj))
                 : krj     ? (has_cal ? launch_sample<false, true, true>(ctx, grid, lds.bytes, g, groups, kj)
                                      : launch_sample<false, false, true>(ctx, grid, lds.bytes, g, groups, kj))
                 : has_cal ? launch_sample<false, true, false>(ctx, grid, lds.bytes, g, groups, kj)
                           : launch_sample<false, false, false>(ctx, grid, lds.bytes, g, groups, kj);
  if (rc != MRX_OK) return rc;
  if (g.pairs) MRX_HIP(ctx, hipEventRecord(ctx->map_pairs_read, ctx->stream));
  return MRX_OK;
}

extern "C" {

int mrx_map_sample(mrx_ctx* ctx, const mrx_sky_map* map, const mrx_map_cal* cal,
                   const float* d_az, const float* d_el, int T, const double* d_transform,
                   const float* d_dx, const float* d_dy, const double* d_stokes_w, int D,
                   float* d_out, size_t ld_out) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  return map_sample(ctx, map, cal, d_az, d_el, T, d_transform, d_dx, d_dy, d_stokes_w, D, d_out, ld_out, nullptr);
}

int mrx_map_sample_krj(mrx_ctx* ctx, const mrx_sky_map* map, const mrx_map_cal* cal,
                       const float* d_az, const float* d_el, int T, const double* d_transform,
                       const float* d_dx, const float* d_dy, const double* d_stokes_w, int D,
                       const float* d_scale, const float* d_bore_el, const float* d_krj_dx, const float* d_krj_dy,
                       const int32_t* d_band, const float* d_cal_axis_el, const float* d_cal_values, int n_el, int n_bands,
                       float* d_out, size_t ld_out) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_bore_el && d_krj_dx && d_krj_dy && d_band && d_cal_axis_el && d_cal_values, "null K_RJ pointer");
  MRX_REQUIRE(ctx, n_el >= 2 && n_bands >= 1, "need n_el >= 2 and n_bands >= 1");
  MapKrj kj{};
  kj.bore_el = d_bore_el;
  kj.dx = d_krj_dx;
  kj.dy = d_krj_dy;
  kj.band = d_band;
  kj.scale = d_scale;
  kj.cal_axis = d_cal_axis_el;
  kj.cal_values = d_cal_values;
  kj.n_el = n_el;
  kj.n_bands = n_bands;
  return map_sample(ctx, map, cal, d_az, d_el, T, d_transform, d_dx, d_dy, d_stokes_w, D, d_out, ld_out, &kj);
}

}  // extern "C"
