// The statistics of a [D, T] TOD per (row, segment) and the flagging of whole segments (maria_amd/cuts.py).
// Segment s of d_bound [S + 1] is [lo, hi), both clamped to 0 .. T, L = hi - lo, as in mrx_subscan.hip:
//   term(d, t) = (double)x[d][t] - (double)model[d][t]                       (plain (double)x without a model)
//   kept       = the segment's t with flags[d][t] == 0, n of them;  p pairs (t, t + 1) both in the segment and kept
//   mu = (sum over kept of term) / (double)n;   e = term - mu;   M2, M3, M4 = sums over kept of e e, (e e) e, (e e) (e e)
//   min, max of term over kept;   D2 = sum over the pairs of (term(t + 1) - term(t))^2
// The file is built without FMA contraction: every operation above is one float64 rounding.
//
// mrx_tod_segment_moments.  One wave takes one (row, segment) and owns all of its sums, as in segment_normal_kernel, but
// a lane owns four consecutive samples of every chunk of 256: lane o of chunk c the samples 256 c + 4 o .. + 3, read with
// one 16-byte copy (x, the model) and one 4-byte copy (the flags) of no alignment beyond the element's, which the
// compiler turns into the widest loads the target allows at that alignment; the last, partial chunk is read sample by
// sample.  Either way a sample goes to the same lane and the same place in that lane's order: chunk after chunk, the
// four samples ascending, then the 64 lanes meet (mrx_tod_dev.h: wave_sum_all), after which every lane holds every sum.
// The order is a function of L alone.  The segment is read twice: the first pass gives n, p, the sum, min, max and D2,
// the second, with mu = sum / n known to every lane, the central sums (its reads come from cache: a segment of a scan is
// a few tens of KiB).  Three of a lane's four pairs lie inside the lane; the pair across the seam takes the last sample
// of the lane before it by a rotation of the wave, and lane 0 that of lane 63 of the chunk before (carried over).
// A flagged sample enters every sum as 0.0 (selected, never multiplied), min and max by selects that let a NaN through.
//
// mrx_tod_segment_flag.  A streaming pass over (row, tile of 4096 flags), thread o the sixteen bytes 16 o .. 16 o + 15 (one
// 16-byte access where pointer and pitch allow it, bytes otherwise).  A thread finds its sample's segment as
// mrx_tod_segment_apply does (find_segment, kept while the following samples stay inside) and
// writes only where it has set something: a thread with no masked segment reads and leaves.
#include "mrx_internal.h"
#include "mrx_tod_dev.h"

#include <algorithm>

namespace {

using mrx_tod::clamp_bound;
using mrx_tod::find_segment;
using mrx_tod::kThreads;
using mrx_tod::kWave;
using mrx_tod::kWaves;
using mrx_tod::wave_sum_all;

constexpr int kOwn = 4;                 // consecutive samples of a lane in a chunk
constexpr int kChunk = kWave * kOwn;    // 256 samples
constexpr int kFlight = 2;              // chunks whose loads go out together
constexpr int kFlagOwn = 16;            // consecutive flags of a thread of the flagging pass
constexpr int kFlagTile = kThreads * kFlagOwn;

// A lane's four samples of the chunk that starts `rem` samples before the segment's end: term, selected to 0.0
// where the sample is flagged or past the end, and keep.  xs, ms, fs point at the chunk's first sample.  A chunk past the
// segment's end has rem <= 0: nothing is kept and nothing is read.
template <bool kModel, bool kFlags>
__device__ __forceinline__ void load_own(const float* __restrict__ xs, const float* __restrict__ ms, const unsigned char* __restrict__ fs, int rem,
                                         int lane, double (&term)[kOwn], bool (&keep)[kOwn]) {
  const int k = kOwn * lane;
  float xv[kOwn], mv[kOwn];
  unsigned char fv[kOwn];
  if (k + kOwn <= rem) {
    __builtin_memcpy(xv, xs + k, sizeof(xv));
    if (kModel) __builtin_memcpy(mv, ms + k, sizeof(mv));
    if (kFlags) __builtin_memcpy(fv, fs + k, sizeof(fv));
#pragma unroll
    for (int j = 0; j < kOwn; ++j) keep[j] = !kFlags || fv[j] == 0;
  } else {
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      const bool in = k + j < rem;
      xv[j] = in ? xs[k + j] : 0.0f;
      if (kModel) mv[j] = in ? ms[k + j] : 0.0f;
      keep[j] = in && (!kFlags || fs[k + j] == 0);
    }
  }
#pragma unroll
  for (int j = 0; j < kOwn; ++j) {
    const double t = kModel ? (double)xv[j] - (double)mv[j] : (double)xv[j];
    term[j] = keep[j] ? t : 0.0;
  }
}

// a NaN goes through: t < NaN is false, so that a NaN once taken stays
__device__ __forceinline__ double nan_min(double a, double t) { return (t < a || t != t) ? t : a; }
__device__ __forceinline__ double nan_max(double a, double t) { return (t > a || t != t) ? t : a; }

template <bool kModel, bool kFlags>
__global__ __launch_bounds__(kThreads) void segment_moments_kernel(const float* __restrict__ x, size_t ld_x, const float* __restrict__ model,
                                                                   size_t ld_m, const unsigned char* __restrict__ flags, size_t ld_f, int T,
                                                                   const int* __restrict__ bound, int S, double* __restrict__ stat,
                                                                   unsigned* __restrict__ count, long long n_items) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int before = (lane + kWave - 1) & (kWave - 1);
  for (long long item = (long long)blockIdx.x * kWaves + wave; item < n_items; item += (long long)gridDim.x * kWaves) {
    const long long d = item / S;
    const int s = (int)(item - d * S);
    const int lo = clamp_bound(bound[s], T), hi = clamp_bound(bound[s + 1], T);
    const int L = hi - lo;  // <= 0: empty, the loops below do not run
    const float* const xr = x + (size_t)d * ld_x + lo;
    const float* const mr = kModel ? model + (size_t)d * ld_m + lo : nullptr;
    const unsigned char* const fr = kFlags ? flags + (size_t)d * ld_f + lo : nullptr;
    double sum = 0.0, d2 = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
    unsigned n = 0, p = 0;
    double carry_term = 0.0;  // lane 63's last sample of the chunk before: lane 0's neighbour
    int carry_keep = 0;
    // the bounds of both loops are the wave's, not the lane's: every lane takes part in every exchange
    for (long long base = 0; base < L; base += kFlight * kChunk) {  // 64 bits: base passes L, which may be near 2^31
      double term[kFlight][kOwn];
      bool keep[kFlight][kOwn];
#pragma unroll
      for (int c = 0; c < kFlight; ++c) {
        const long long off = base + c * kChunk;
        const int rem = (int)min((long long)L - off, (long long)kChunk);  // <= 0: a chunk past the end, nothing kept
        load_own<kModel, kFlags>(xr + off, kModel ? mr + off : nullptr, kFlags ? fr + off : nullptr, rem, lane, term[c], keep[c]);
      }
#pragma unroll
      for (int c = 0; c < kFlight; ++c) {
        const double rot_term = __shfl(term[c][kOwn - 1], before, kWave);
        const int rot_keep = __shfl((int)keep[c][kOwn - 1], before, kWave);
        double prev_term = lane == 0 ? carry_term : rot_term;
        bool prev_keep = (lane == 0 ? carry_keep : rot_keep) != 0;
        carry_term = rot_term, carry_keep = rot_keep;
#pragma unroll
        for (int j = 0; j < kOwn; ++j) {
          const double t = term[c][j];
          const bool k = keep[c][j];
          sum = sum + t;
          n += k ? 1u : 0u;
          mn = k ? nan_min(mn, t) : mn;
          mx = k ? nan_max(mx, t) : mx;
          const bool both = k && prev_keep;
          const double diff = both ? t - prev_term : 0.0;
          d2 = d2 + diff * diff;
          p += both ? 1u : 0u;
          prev_term = t, prev_keep = k;
        }
      }
    }
    wave_sum_all(sum);
    wave_sum_all(d2);
    wave_sum_all(n);
    wave_sum_all(p);
#pragma unroll
    for (int o = kWave / 2; o >= 1; o >>= 1) {  // the same butterfly: every lane ends with the same minimum and maximum
      mn = nan_min(mn, __shfl_xor(mn, o, kWave));
      mx = nan_max(mx, __shfl_xor(mx, o, kWave));
    }
    const double mu = n ? sum / (double)n : 0.0;
    double m2 = 0.0, m3 = 0.0, m4 = 0.0;
    if (n) {
      for (long long base = 0; base < L; base += kFlight * kChunk) {  // 64 bits: base passes L, which may be near 2^31
        double term[kFlight][kOwn];
        bool keep[kFlight][kOwn];
#pragma unroll
        for (int c = 0; c < kFlight; ++c) {
          const long long off = base + c * kChunk;
          const int rem = (int)min((long long)L - off, (long long)kChunk);
          load_own<kModel, kFlags>(xr + off, kModel ? mr + off : nullptr, kFlags ? fr + off : nullptr, rem, lane, term[c], keep[c]);
        }
#pragma unroll
        for (int c = 0; c < kFlight; ++c) {
#pragma unroll
          for (int j = 0; j < kOwn; ++j) {
            const double e = keep[c][j] ? term[c][j] - mu : 0.0;
            const double e2 = e * e;
            m2 = m2 + e2;
            m3 = m3 + e2 * e;
            m4 = m4 + e2 * e2;
          }
        }
      }
      wave_sum_all(m2);
      wave_sum_all(m3);
      wave_sum_all(m4);
    }
    // lane j stores value j, picked by selects
    double v = 0.0;
    v = lane == 0 ? mu : v;
    v = lane == 1 ? m2 : v;
    v = lane == 2 ? m3 : v;
    v = lane == 3 ? m4 : v;
    v = lane == 4 ? (n ? mn : 0.0) : v;
    v = lane == 5 ? (n ? mx : 0.0) : v;
    v = lane == 6 ? d2 : v;
    if (lane < 8) stat[(size_t)item * 8 + lane] = v;
    if (lane < 2) count[(size_t)item * 2 + lane] = lane == 0 ? n : p;
  }
}

__global__ __launch_bounds__(kThreads) void segment_flag_kernel(unsigned char* flags, size_t ld_f, int T, const int* __restrict__ bound, int S,
                                                                const unsigned char* __restrict__ mask, unsigned value, int wide,
                                                                int tiles_per_row, long long n_tiles) {
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / tiles_per_row;
    const int q = (int)(tile - row * tiles_per_row) * kFlagTile + kFlagOwn * (int)threadIdx.x;
    if (q >= T) continue;
    unsigned char* const fr = flags + (size_t)row * ld_f;
    const unsigned char* const mr = mask + (size_t)row * S;
    unsigned w[kFlagOwn / 4] = {0u, 0u, 0u, 0u};  // the bits to set, four flags a word
    int lo = 0, hi = 0;
    bool on = false, any = false;
#pragma unroll
    for (int k = 0; k < kFlagOwn; ++k) {
      const int t = q + k;
      if (t < T) {
        if (!(t >= lo && t < hi)) {
          const int s = find_segment(bound, S, T, t, lo, hi);
          on = s >= 0 && mr[s] != 0;
        }
        const bool set = on && t >= lo && t < hi;
        w[k / 4] |= set ? value << (8 * (k % 4)) : 0u;
        any = any || set;
      }
    }
    if (!any) continue;
    if (wide && q + kFlagOwn <= T) {
      uint4* const at = reinterpret_cast<uint4*>(fr + q);
      uint4 f = *at;
      f.x |= w[0], f.y |= w[1], f.z |= w[2], f.w |= w[3];
      *at = f;
    } else {
#pragma unroll
      for (int k = 0; k < kFlagOwn; ++k) {
        const unsigned b = (w[k / 4] >> (8 * (k % 4))) & 0xffu;
        if (b) fr[q + k] = (unsigned char)(fr[q + k] | b);  // b != 0 only where q + k < T
      }
    }
  }
}

template <bool kModel, bool kFlags>
void launch_moments(mrx_ctx* ctx, const float* x, size_t ld_x, const float* model, size_t ld_m, const uint8_t* flags, size_t ld_f, int T,
                    const int32_t* bound, int S, double* stat, uint32_t* count, long long n_items) {
  hipLaunchKernelGGL((segment_moments_kernel<kModel, kFlags>), dim3(mrx_resident_blocks(ctx, (n_items + kWaves - 1) / kWaves)), dim3(kThreads), 0,
                     ctx->stream, x, ld_x, model, ld_m, flags, ld_f, T, bound, S, stat, count, n_items);
}

}  // namespace

extern "C" {

int mrx_tod_segment_moments(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m, const uint8_t* d_flags, size_t ld_f,
                            int D, int T, const int32_t* d_bound, int S, double* d_stat, uint32_t* d_count) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_bound && d_stat && d_count, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, S >= 1, "need S >= 1 segments");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && (!d_model || ld_m >= (size_t)T) && (!d_flags || ld_f >= (size_t)T), "ld_x, ld_m or ld_f smaller than T");
  const long long n_items = (long long)D * S;
  if (d_model && d_flags)
    launch_moments<true, true>(ctx, d_x, ld_x, d_model, ld_m, d_flags, ld_f, T, d_bound, S, d_stat, d_count, n_items);
  else if (d_model)
    launch_moments<true, false>(ctx, d_x, ld_x, d_model, ld_m, d_flags, ld_f, T, d_bound, S, d_stat, d_count, n_items);
  else if (d_flags)
    launch_moments<false, true>(ctx, d_x, ld_x, d_model, ld_m, d_flags, ld_f, T, d_bound, S, d_stat, d_count, n_items);
  else
    launch_moments<false, false>(ctx, d_x, ld_x, d_model, ld_m, d_flags, ld_f, T, d_bound, S, d_stat, d_count, n_items);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_tod_segment_flag(mrx_ctx* ctx, uint8_t* d_flags, size_t ld_f, int D, int T, const int32_t* d_bound, int S, const uint8_t* d_mask,
                         int value) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_flags && d_bound && d_mask, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1, "need D >= 1 rows of T >= 1 samples");
  MRX_REQUIRE(ctx, S >= 1, "need S >= 1 segments");
  MRX_REQUIRE(ctx, value >= 1 && value <= 255, "value must be in 1 .. 255");
  MRX_REQUIRE(ctx, ld_f >= (size_t)T, "ld_f smaller than T");
  const mrx_tile_grid_t g = mrx_tile_grid(ctx, D, T, kFlagTile);
  const int wide = mrx_aligned(d_flags, ld_f, 16);
  hipLaunchKernelGGL(segment_flag_kernel, dim3(g.blocks), dim3(kThreads), 0, ctx->stream, d_flags, ld_f, T, d_bound, S, d_mask, (unsigned)value,
                     wide, g.tiles_per_row, g.n_tiles);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

}  // extern "C"
