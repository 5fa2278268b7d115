// The map operators on the sampler's pointing, for gfx950: everything that goes from a TOD to the map or applies P and
// its transpose, on the pointing matrix of mrx_map_sample.hip (steps 1-4 there; mrx_map_pointing.h holds steps 1-3 and
// the arguments both files share).  In this order:
//   * axis_weights: a map axis' two pixels and weight for a detector sample (the sampler's own form is axis_cell_t there);
//   * the binning, P^T W d and P^T W 1 (mappers/bin_mapper.py:84-120): the atomic form (bin_atomic_kernel) and the routed
//     form (pass A bin_bucket_body, the order of the regions, pass B bin_accumulate_body), driven by routed_bin;
//   * the maximum-likelihood map-maker's operators: P x (map_project_kernel), P^T W P x (normal_bucket_kernel,
//     normal_accumulate_kernel), the block diagonal of P^T W P and its per-pixel solve (block_solve_kernel);
//   * the destriper's two operators: the baseline reduction and the binning of baselines.
// Tile = 16 detectors x 1024 samples, four consecutive samples a thread (MapTile), except the routed bilinear pass A.
// Built without FMA contraction, like mrx_map_sample.hip and mrx_beamfit.hip: the three inline the same pointing code and
// must give the same bits (csrc/Makefile).
#include <cmath>
#include <type_traits>

#include "mrx_internal.h"
#include "mrx_map_pointing.h"  // steps 1-3: MapArgs, map_args, DetConst, SampleConst, sample_const, sample_offsets, make_det_const; the tile

namespace {

// one axis of utils/linalg.py:25-41: the two pixels and the weight of the upper one.
// With u = (x - first) / step the reference's np.digitize bin is floor(u) + 1 and its weight
// (x - side[b-1]) / (side[b] - side[b-1]) is the fractional part of u; at a node the two
// conventions (bin b with p = 0, bin b - 1 with p = 1) give the same interpolated value, so the
// nodes themselves need not be read.
__device__ __forceinline__ void axis_weights(const Axis& a, float x, bool bilinear, int& i0, int& i1, float& p) {
  // Round 6: the float32 split form of axis_cell_t (mrx_map_sample.hip) instead of a float64 position (measured equal in the binning's
  // pass A, which does not wait for its arithmetic -- kept so that the file has ONE rule for cell and weight).  The offset
  // is first clamped INTO the axis (a NaN goes to the low end): beyond the ends the reference's weights are
  // (x + inf)/inf = nan -> 0 and finite/inf = 0, i.e. the edge pixel alone -- here the first cell with p = 0 or the last
  // with p = 1, the same pixels and weights.  k: the cell, kept inside the axis; frac: the position inside it, good to
  // 1e-7 pixel (the float64 form's fraction to float32 rounding) -- so the nearest pixel flips against the float64 form
  // only within 1e-7 pixel of a pixel's edge, and a bilinear weight moves by 1e-7.
  const float xc = __builtin_amdgcn_fmed3f(x, a.x_min, a.x_max);
  const float k = __builtin_amdgcn_fmed3f(floorf(fmaf(xc, a.inv_hi, a.c_frac)), a.k_lo, a.k_hi);
  const float frac = fmaf(xc, a.inv_hi, -k) + fmaf(xc, a.inv_lo, a.c_frac);
  const int cell = (int)(k + a.c_int);  // 0 .. n - 2
  // bilinear: the cell's two nodes and the weight of the upper one (at a node the weight 0 or 1 names it either way);
  // nearest (np.digitize on the midpoints): the node on this side or the far side of the cell's middle
  const int up = frac >= 0.5f ? 1 : 0;
  i0 = bilinear ? cell : cell + up;
  i1 = bilinear ? cell + 1 : cell + up;
  p = bilinear ? __builtin_amdgcn_fmed3f(frac, 0.0f, 1.0f) : 0.0f;
}

// ---- binning: the transpose of the same pointing matrix (mappers/bin_mapper.py:84-120) ----
struct BinArgs {
  const float* tod;     // [D][ld_tod] signal
  size_t ld_tod;
  const float* weight;  // [D][ld_w] or null (ones)
  size_t ld_w;
  const int32_t* channel;  // [D] map channel of each detector, or null (0)
  double* sum;          // [S][C][n_eta][n_xi]
  double* wgt;
};

__device__ __forceinline__ int det_channel(const MapArgs& g, const BinArgs& b, int d) {  // the map channel of detector d
  return b.channel ? min(max(b.channel[d], 0), g.C - 1) : 0;
}

__device__ __forceinline__ double sample_weight(const BinArgs& b, int d, int s) {  // W of sample s of detector d
  return b.weight ? (double)b.weight[(size_t)d * b.ld_w + s] : 1.0;
}

// ---- bucketed binning: no global atomics on scattered addresses ---------------------------
// Scattered float atomics execute at the memory side at a tenth of the contiguous rate
// (MI355X_MICROARCH.md, Global float atomics), and the focal plane is sparser than the map, so
// privatising tiles in LDS merges next to nothing.  Instead the samples are routed
// to the map: pass A computes every sample's pixel(s) once, sorts its tile's contributions by
// map region (64 x 32 pixels of one plane) with an LDS counting sort and writes them, region by
// region, into the tile's slot of the work buffer plus one word per (region, tile) that says
// where; pass B gives every region to a few workgroups that read the region's segments,
// accumulate in LDS (float64 ds_add) and add the finished block to the map: atomics again, but
// on whole rows of 64 pixels.  The result equals mrx_bin_map's to float64 rounding (the order of
// the sums differs).  Nearest pixel: a tile is 16 detectors x 1024 samples, one contribution per
// sample.  Bilinear: 8 detectors x 256 samples, up to four contributions per sample (corners of
// zero weight are dropped); the float32 offsets of the tile's samples stay in LDS between the
// two sweeps so that the weights are formed once more without the pointing.
constexpr int kBinBx = 64, kBinBy = 32;
constexpr int kBinRegionPx = kBinBx * kBinBy;  // 2048 pixels: 11 bits
constexpr int kBinMaxRegions = 2048;
constexpr uint32_t kBinNone = 0xffffffffu;

template <bool kBil>
struct BinTile {
#ifndef MRX_BIN_DET
#define MRX_BIN_DET 16
#define MRX_BIN_SPT 4
#endif
  static constexpr int kDet = kBil ? 8 : MRX_BIN_DET;     // detectors per tile (< 32: five bits of an entry)
  static constexpr int kSpt = kBil ? 1 : MRX_BIN_SPT;     // samples per thread
  static constexpr int kCorners = kBil ? 4 : 1;
  static constexpr int kSamples = kBlock * kSpt;
  static constexpr int kEntries = kDet * kSamples * kCorners;  // 16 384 / 8 192 contributions per tile at most
};

// A routed contribution.  Bilinear: pixel, signal, sample weight x corner weight in float64 (16 bytes).
// Nearest pixel (the mapper's default; corner weight 1): the sample weight as the float32 it is (12 bytes), or
// nothing at all when the caller passed no weights (8 bytes: pass A writes and pass B reads half the bytes).
template <int kBytes>
struct BinEntryT;
template <>
struct BinEntryT<16> {
  uint32_t local;  // pixel inside the region, (eta & 31) << 6 | (xi & 63), | detector within the tile << 11
  float d;         // signal
  double ww;       // sample weight x corner weight
  __device__ __forceinline__ double weight() const { return ww; }
  __device__ __forceinline__ void set_weight(double w) { ww = w; }
};
template <>
struct BinEntryT<12> {
  uint32_t local;
  float d;
  float w;
  __device__ __forceinline__ double weight() const { return (double)w; }
  __device__ __forceinline__ void set_weight(double x) { w = (float)x; }
};
template <>
struct BinEntryT<8> {
  uint32_t local;
  float d;
  __device__ __forceinline__ double weight() const { return 1.0; }
  __device__ __forceinline__ void set_weight(double) {}
};
static_assert(sizeof(BinEntryT<16>) == 16 && sizeof(BinEntryT<12>) == 12 && sizeof(BinEntryT<8>) == 8, "entry sizes");
constexpr int bin_entry_bytes(bool bilinear, bool weights) { return bilinear ? 16 : weights ? 12 : 8; }

struct BucketArgs {
  int nbx, nby, R;     // regions per row / per column of a plane, in all (channels x nby x nbx)
  int s0, s1;          // samples [s0, s1) of this time chunk
  int tiles_x;         // sample tiles of the chunk; tile = blockIdx.y * tiles_x + blockIdx.x
  int n_tiles;
  int tile_det, tile_entries;  // BinTile<>::kDet, kEntries of the form in use
  uint32_t* tab;       // [R][n_tiles]: (first entry of the region in the tile's slot) << 16 | count
  uint32_t* totals;    // [R]: contributions per region in this chunk (pass A adds, bin_order_kernel reads)
  const int* order;    // [R]: regions by falling total (pass B takes the heavy ones first: its tail is then made of light ones)
  void* entries;       // [n_tiles][tile_entries] BinEntryT<entry_bytes>
};

// the contributions of one sample: pixel (region << 11 | local) and weight per corner
template <bool kBil>
__device__ __forceinline__ void bin_corners(const MapArgs& g, const BucketArgs& k, const Axis& ax_eta, const Axis& ax_xi,
                                            float ox, float oy, int chan, uint32_t (&word)[BinTile<kBil>::kCorners],
                                            double (&wc)[BinTile<kBil>::kCorners]) {
  int e0, e1, x0, x1;
  float pef, pxf;
  axis_weights(ax_eta, oy, kBil, e0, e1, pef);
  axis_weights(ax_xi, ox, kBil, x0, x1, pxf);
  const double pe = (double)pef, px = (double)pxf;  // the products below in float64, as ml_corners forms them
  auto pixel = [&](int e, int x) {
    const uint32_t r = (uint32_t)((chan * k.nby + (e >> 5)) * k.nbx + (x >> 6));
    return (r << 11) | (uint32_t)(((e & 31) << 6) | (x & 63));
  };
  if constexpr (kBil) {
    // the order and the weights of ml_corners: (e0,x0), (e1,x0), (e0,x1), (e1,x1)
    word[0] = pixel(e0, x0); wc[0] = (1.0 - pe) * (1.0 - px);
    word[1] = pixel(e1, x0); wc[1] = pe * (1.0 - px);
    word[2] = pixel(e0, x1); wc[2] = (1.0 - pe) * px;
    word[3] = pixel(e1, x1); wc[3] = pe * px;
  } else {
    word[0] = pixel(e0, x0);
    wc[0] = 1.0;
  }
}

// ---- the maximum-likelihood map-maker's operators: P x, P^T W P x, the block diagonal of P^T W P ----
// The pointing matrix is the binning's, signed: a sample's row holds w_k(d) b_c at pixel c of plane (k, channel), with
// the pixels and float32 corner weights of axis_weights and the corner order and float64 products of ml_corners.
struct MlArgs {
  const double* x;           // [S][C][n_eta][n_xi] the map the operator is applied to
  const double* det_weight;  // [D] or null (ones): the per-detector factor of W
  double* y;                 // the operator's map output: P^T W P x (added), or the blocks [S(S+1)/2][C][n_eta][n_xi]
  float* out;                // mrx_map_project: [D][ld_out]
  size_t ld_out;
  double alpha, beta;
  // the destriper's operators: baseline b of a detector covers samples [b L, min((b + 1) L, T))
  const double* amp;         // mrx_bin_map_baselines: [D][nb] baseline amplitudes a
  int L, nb;                 // baseline length in samples, baselines per detector ceil(T / L)
  const uint8_t* mask;       // mrx_baseline_reduce: [C][n_eta][n_xi] 1 where the pixel's block is solved, or null (ones)
  double* hits;              // mrx_baseline_reduce: [D][nb] sum of W mu, or null
};

__device__ __forceinline__ double det_weight(const MlArgs& m, int d) { return m.det_weight ? m.det_weight[d] : 1.0; }

// a sample's pixels and corner weights (in float64, from axis_weights' float32 ones): corners (e0,x0), (e1,x0), (e0,x1),
// (e1,x1).  The pixels are the key of a run of samples in bin_atomic_kernel.
struct MlCorners {
  int o[4];     // pixel offsets in a plane
  double w[4];  // corner weights (nearest pixel: 1, 0, 0, 0)
};

__device__ __forceinline__ MlCorners ml_corners(const MapArgs& g, const Axis& ax_eta, const Axis& ax_xi, float ox, float oy) {
  int e0, e1, x0, x1;
  float pef, pxf;
  axis_weights(ax_eta, oy, g.bilinear, e0, e1, pef);
  axis_weights(ax_xi, ox, g.bilinear, x0, x1, pxf);
  const double pe = (double)pef, px = (double)pxf;
  MlCorners c;
  c.o[0] = e0 * g.n_xi + x0; c.o[1] = e1 * g.n_xi + x0; c.o[2] = e0 * g.n_xi + x1; c.o[3] = e1 * g.n_xi + x1;
  c.w[0] = (1.0 - pe) * (1.0 - px); c.w[1] = pe * (1.0 - px); c.w[2] = (1.0 - pe) * px; c.w[3] = pe * px;
  return c;
}

// (P x)_s = sum_k w_k sum_c b_c x[k][chan][pix_c], float64; corners of zero weight are not read
__device__ __forceinline__ double ml_gather(const MapArgs& g, const MlArgs& m, const DetConst& dc, int chan, const MlCorners& c) {
  const size_t plane = (size_t)g.n_eta * g.n_xi;
  const int corners = g.bilinear ? 4 : 1;
  double v = 0.0;
  for (int k = 0; k < g.S; ++k) {
    const double* xk = m.x + ((size_t)k * g.C + chan) * plane;
    double s = 0.0;
    for (int q = 0; q < corners; ++q)
      if (c.w[q] != 0.0) s = fma(c.w[q], xk[c.o[q]], s);
    v = fma(dc.w[k], s, v);
  }
  return v;
}

// what pass A and bin_atomic_kernel bin: the TOD (the binning), W (P x)_s (the normal operator), W a[d][s / L] (the
// destriper's P^T W F a) or W b_c (the block diagonal of P^T W P: bin_atomic_kernel only)
enum BinSource { kSrcTod = 0, kSrcNormal = 1, kSrcBaselines = 2, kSrcBlocks = 3 };

template <bool kChain, bool kBil, bool kW, int kSrc>
__device__ __forceinline__ void bin_bucket_body(const MapArgs& g, const BinArgs& b, const BucketArgs& k, const MlArgs& m) {
  constexpr bool kNormal = kSrc != kSrcTod;
  using Tile = BinTile<kBil>;
  // the normal operator routes W (P x)_s b_c, a float64, in the 16-byte entry (its signal field holds 1); so does the
  // destriper's W a_b
  using Entry = BinEntryT<kNormal ? 16 : bin_entry_bytes(kBil, kW)>;
  constexpr int kDet = Tile::kDet, kSpt = Tile::kSpt, kCorners = Tile::kCorners;
  __shared__ DetConst dets[kDet];
  __shared__ uint32_t part[kBlock];
  extern __shared__ uint32_t bucket_lds[];
  // A contribution's sort word, region << 11 | pixel-in-region, is 22 bits: kept as its low 16 bits and its high byte
  // in two arrays (0xff in the high byte: no contribution), 48 KB a tile instead of 64 -- with the histogram doubling
  // as the cursors that lets THREE workgroups share a CU's LDS instead of two (the kernel waits on its pointing
  // arithmetic and its LDS atomics: occupancy is what it lacks; pass A 16.9 -> 13.1 ms onto 1024^2).  A thread's four
  // words of one detector are neighbours in both arrays: one 8-byte and one 4-byte LDS access each way.
  constexpr int kGroup = kSpt * kCorners;  // sort words per thread and detector: 4, or 2
  static_assert(kGroup == 4 || kGroup == 2, "two or four sort words per thread and detector");
  using Lo = std::conditional_t<kGroup == 4, uint2, uint32_t>;     // kGroup x uint16
  using Hi = std::conditional_t<kGroup == 4, uint32_t, uint16_t>;  // kGroup x uint8
  Lo* lo16 = reinterpret_cast<Lo*>(bucket_lds);                   // [kEntries / kGroup], by (detector, thread)
  Hi* hi8 = reinterpret_cast<Hi*>(bucket_lds + Tile::kEntries / 2);  // [kEntries / kGroup]
  uint32_t* hist = bucket_lds + Tile::kEntries / 2 + Tile::kEntries / 4;  // [R]: counts, then (after the scan) cursors
  float2* oxy = reinterpret_cast<float2*>(hist + k.R);  // bilinear: [kDet][kSamples] offsets of the samples
  const int d0 = blockIdx.y * kDet;
  const int sb = k.s0 + blockIdx.x * Tile::kSamples + threadIdx.x * kSpt;
  const int nd = min(kDet, g.D - d0);
  const int tile = blockIdx.y * k.tiles_x + blockIdx.x;
  if ((int)threadIdx.x < nd) dets[threadIdx.x] = make_det_const(g, d0 + threadIdx.x);
  for (int i = threadIdx.x; i < k.R; i += kBlock) hist[i] = 0u;
  const Axis ax_eta = g.eta, ax_xi = g.xi;
  SampleConst sc[kSpt];
#pragma unroll
  for (int q = 0; q < kSpt; ++q) {
    sample_const(g, sb + q, kChain, sc[q]);
    sc[q].s = min(max(sb + q, 0), g.T - 1);
  }
  __syncthreads();
  // sweep 1: the pixels of every sample, the tile's histogram over regions
  for (int dl = 0; dl < nd; ++dl) {
    const DetConst dc = dets[dl];
    const int d = d0 + dl;
    const int chan = det_channel(g, b, d);
    uint32_t grp[kGroup];
#pragma unroll
    for (int q = 0; q < kSpt; ++q) {
      uint32_t word[kCorners];
      double wc[kCorners];
#pragma unroll
      for (int c = 0; c < kCorners; ++c) word[c] = kBinNone;
      if (sb + q < k.s1) {
        float ox, oy, el_d;
        sample_offsets<kChain, false>(g, dc, sc[q], ox, oy, el_d);
        if (kBil) oxy[(dl * kBlock + threadIdx.x) * kSpt + q] = make_float2(ox, oy);
        bin_corners<kBil>(g, k, ax_eta, ax_xi, ox, oy, chan, word, wc);
#pragma unroll
        for (int c = 0; c < kCorners; ++c) {
          if (wc[c] == 0.0) word[c] = kBinNone;  // a corner of zero weight adds nothing (np.abs(P) entries that are 0)
          else atomicAdd(&hist[word[c] >> 11], 1u);
        }
      }
#pragma unroll
      for (int c = 0; c < kCorners; ++c) grp[q * kCorners + c] = word[c];
    }
    // (kBinNone >> 16 = 0xffff: its high byte reads 0xff, which no region's does -- R <= 2048 leaves 6 bits there)
    if constexpr (kGroup == 4) {
      lo16[dl * kBlock + threadIdx.x] = make_uint2((grp[0] & 0xffffu) | (grp[1] << 16), (grp[2] & 0xffffu) | (grp[3] << 16));
      hi8[dl * kBlock + threadIdx.x] = ((grp[0] >> 16) & 0xffu) | (((grp[1] >> 16) & 0xffu) << 8) | (((grp[2] >> 16) & 0xffu) << 16) |
                                       (((grp[3] >> 16) & 0xffu) << 24);
    } else {
      lo16[dl * kBlock + threadIdx.x] = (grp[0] & 0xffffu) | (grp[1] << 16);
      hi8[dl * kBlock + threadIdx.x] = (uint16_t)(((grp[0] >> 16) & 0xffu) | (((grp[1] >> 16) & 0xffu) << 8));
    }
  }
  __syncthreads();
  // exclusive scan of the histogram: where each region's contributions start in the tile's slot
  const int per = (k.R + kBlock - 1) / kBlock;
  const int r_lo = threadIdx.x * per, r_hi = min(r_lo + per, k.R);
  uint32_t mine = 0;
  for (int r = r_lo; r < r_hi; ++r) mine += hist[r];
  part[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {
    const uint32_t add = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  uint32_t run = part[threadIdx.x] - mine;
  for (int r = r_lo; r < r_hi; ++r) {
    const uint32_t c = hist[r];
    hist[r] = run;  // the region's cursor from here on
    if (c) {
      k.tab[(size_t)r * k.n_tiles + tile] = (run << 16) | c;
      atomicAdd(&k.totals[r], c);
    }
    run += c;
  }
  __syncthreads();
  // sweep 2: every contribution to its place
  Entry* slot = reinterpret_cast<Entry*>(k.entries) + (size_t)tile * Tile::kEntries;
  for (int dl = 0; dl < nd; ++dl) {
    const int d = d0 + dl;
    const int chan = det_channel(g, b, d);
    double det_w = 1.0;
    if constexpr (kNormal) det_w = det_weight(m, d);
    uint32_t grp[kGroup];
    if constexpr (kGroup == 4) {
      const uint2 l2 = lo16[dl * kBlock + threadIdx.x];
      const uint32_t h4 = hi8[dl * kBlock + threadIdx.x];
      grp[0] = (l2.x & 0xffffu) | ((h4 & 0xffu) << 16);
      grp[1] = (l2.x >> 16) | (((h4 >> 8) & 0xffu) << 16);
      grp[2] = (l2.y & 0xffffu) | (((h4 >> 16) & 0xffu) << 16);
      grp[3] = (l2.y >> 16) | ((h4 >> 24) << 16);
    } else {
      const uint32_t l2 = lo16[dl * kBlock + threadIdx.x];
      const uint32_t h2 = hi8[dl * kBlock + threadIdx.x];
      grp[0] = (l2 & 0xffffu) | ((h2 & 0xffu) << 16);
      grp[1] = (l2 >> 16) | ((h2 >> 8) << 16);
    }
#pragma unroll
    for (int q = 0; q < kSpt; ++q) {
      if (sb + q >= k.s1) continue;
      uint32_t word[kCorners];
      double wc[kCorners];
      if (kBil) {
        const float2 o = oxy[(dl * kBlock + threadIdx.x) * kSpt + q];
        bin_corners<kBil>(g, k, ax_eta, ax_xi, o.x, o.y, chan, word, wc);
      } else {
        wc[0] = 1.0;
      }
      double W = kW || kBil ? sample_weight(b, d, sb + q) : 1.0;
      float D;
      if constexpr (kSrc == kSrcBaselines) {
        // W a[d][s / L] in place of W D (nearest pixel only: the corner weight is 1)
        W = sample_weight(b, d, sb + q) * det_w * m.amp[(size_t)d * m.nb + (sb + q) / m.L];
        D = 1.0f;
      } else if constexpr (kNormal) {
        // W (P x)_s in place of W D: the sample's pixels again -- bilinear from its offsets, nearest from its sort word
        MlCorners pc;
        if constexpr (kBil) {
          const float2 o = oxy[(dl * kBlock + threadIdx.x) * kSpt + q];
          pc = ml_corners(g, ax_eta, ax_xi, o.x, o.y);
        } else {
          const uint32_t wd = grp[q];
          const int rem = (int)(wd >> 11) - chan * k.nby * k.nbx, by = rem / k.nbx, bx = rem - by * k.nbx;
          const int e = (by << 5) + (int)((wd >> 6) & 31u), x = (bx << 6) + (int)(wd & 63u);
          pc.o[0] = e * g.n_xi + x;
          pc.w[0] = 1.0;
          pc.w[1] = pc.w[2] = pc.w[3] = 0.0;
        }
        W = sample_weight(b, d, sb + q) * det_w * ml_gather(g, m, dets[dl], chan, pc);
        D = 1.0f;
      } else {
        D = b.tod[(size_t)d * b.ld_tod + sb + q];
      }
#pragma unroll
      for (int c = 0; c < kCorners; ++c) {
        const uint32_t wd = grp[q * kCorners + c];
        if ((wd >> 16) == 0xffu) continue;
        const uint32_t pos = atomicAdd(&hist[wd >> 11], 1u);
        Entry en;
        en.local = (wd & (uint32_t)(kBinRegionPx - 1)) | ((uint32_t)dl << 11);
        en.d = D;
        en.set_weight(W * wc[c]);
        slot[pos] = en;
      }
    }
  }
}

// (the MlArgs of every pass A and pass B: the one signature of routed_bin's kernels; the binning has no use for it)
template <bool kChain, bool kBil, bool kW>
// (168 registers instead of 174: measured 21.3 -> 19.7 ms)
#ifndef MRX_BIN_WAVES
#define MRX_BIN_WAVES 3
#endif
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(MRX_BIN_WAVES, MRX_BIN_WAVES))) void bin_bucket_kernel(MapArgs g, BinArgs b, BucketArgs k, MlArgs) {
  bin_bucket_body<kChain, kBil, kW, kSrcTod>(g, b, k, MlArgs{});
}

// pass A of mrx_map_normal_apply: W (P x)_s b_c routed as pass A of the binning routes W D b_c (without the binning's cap of
// three waves a SIMD: the gather of (P x)_s does not fit its 168 registers)
template <bool kChain, bool kBil>
__global__ __launch_bounds__(kBlock) void normal_bucket_kernel(MapArgs g, BinArgs b, BucketArgs k, MlArgs m) {
  bin_bucket_body<kChain, kBil, true, kSrcNormal>(g, b, k, m);
}

// pass A of mrx_bin_map_baselines: W a[d][s / L] routed the same way (nearest pixel; pass B is normal_accumulate_kernel's)
template <bool kChain>
__global__ __launch_bounds__(kBlock) void baseline_bucket_kernel(MapArgs g, BinArgs b, BucketArgs k, MlArgs m) {
  bin_bucket_body<kChain, false, true, kSrcBaselines>(g, b, k, m);
}

// between the passes: the regions by falling number of contributions (rank by counting: R <= 2048), so that pass B's
// grid meets the regions under the scan's centre -- several times the mean -- first and ends on light ones
__global__ __launch_bounds__(1024) void bin_order_kernel(const uint32_t* __restrict__ totals, int R, int* __restrict__ order) {
  __shared__ uint32_t t[kBinMaxRegions];
  for (int i = threadIdx.x; i < R; i += blockDim.x) t[i] = totals[i];
  __syncthreads();
  for (int i = threadIdx.x; i < R; i += blockDim.x) {
    const uint32_t mine = t[i];
    int rank = 0;
    for (int j = 0; j < R; ++j) rank += (t[j] > mine) || (t[j] == mine && j < i);
    order[rank] = i;
  }
}

// pass B: block (region, split): the region's segments of the split's tiles into LDS, then the
// block of 64 x 32 pixels into the map
template <int kEntryBytes, bool kNormal>
__device__ __forceinline__ void bin_accumulate_body(const MapArgs& g, const BinArgs& b, const BucketArgs& k, int splits, const MlArgs& ml) {
  using Entry = BinEntryT<kEntryBytes>;
  const Entry* entries = reinterpret_cast<const Entry*>(k.entries);
  extern __shared__ double bin_acc[];  // [S][2][kBinRegionPx]: sum, weight (the normal operator: [S][kBinRegionPx], its sum)
  constexpr int kPlanes = kNormal ? 1 : 2;
  __shared__ uint32_t seg_cnt[kBlock];   // a batch's non-empty segments: count,
  __shared__ uint32_t seg_base[kBlock];  // index of the first entry in the work buffer minus its place in the batch's list,
  __shared__ int seg_d0[kBlock];         // first detector of the tile,
  __shared__ int seg_end[kBlock];        // inclusive scan of the counts
  __shared__ int n_seg;
  // workgroup b runs on XCD b mod 8: with the region straight from blockIdx.x and a power-of-two
  // number of regions per map row, an XCD would own whole columns of the map -- and the columns
  // under the scan's centre hold several times the samples of those at its rim (measured: 20 ms
  // against 9 ms for this kernel).  Rotating by the split spreads every column over the XCDs.
  const int r = k.order[(blockIdx.x + blockIdx.y) % (unsigned)k.R];
  for (int i = threadIdx.x; i < g.S * kPlanes * kBinRegionPx; i += kBlock) bin_acc[i] = 0.0;
  const int per = (k.n_tiles + splits - 1) / splits;
  const int t0 = blockIdx.y * per, t1 = min(k.n_tiles, t0 + per);
  const uint32_t* row = k.tab + (size_t)r * k.n_tiles;
  bool any = false;
  for (int base = t0; base < t1; base += kBlock) {
    if (threadIdx.x == 0) n_seg = 0;
    __syncthreads();
    const int tile = base + threadIdx.x;
    const uint32_t v = tile < t1 ? row[tile] : 0u;
    if (v & 0xffffu) {
      const int at = atomicAdd(&n_seg, 1);
      seg_cnt[at] = v & 0xffffu;
      seg_base[at] = (uint32_t)tile * (uint32_t)k.tile_entries + (v >> 16);  // < 2^32: the host bounds the chunk
      seg_d0[at] = (tile / k.tiles_x) * k.tile_det;
    }
    __syncthreads();
    const int n = n_seg;
    if (n == 0) continue;  // uniform
    any = true;
    // the batch's segments as one list of entries: an inclusive scan of the counts, then every
    // thread strides through the list (its segment index only ever moves forward) -- all lanes
    // busy and the loads of successive entries independent, instead of one wave per segment
    // waiting out the memory latency of each
    seg_end[threadIdx.x] = (int)threadIdx.x < n ? (int)seg_cnt[threadIdx.x] : 0;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
      const int add = (int)threadIdx.x >= off ? seg_end[threadIdx.x - off] : 0;
      __syncthreads();
      seg_end[threadIdx.x] += add;
      __syncthreads();
    }
    if ((int)threadIdx.x < n) seg_base[threadIdx.x] -= (uint32_t)(seg_end[threadIdx.x] - (int)seg_cnt[threadIdx.x]);
    __syncthreads();
    const int total = seg_end[n - 1];
    // kPer entries per thread and trip, kBlock apart: every load instruction reads 1 KiB of
    // consecutive entries (lanes on consecutive entries; 16-byte loads at a 64-byte lane stride
    // ran 40 % slower), and the loads of a trip are issued together -- the kernel is bound by
    // memory latency, not by bytes
    constexpr int kPer = 4;
    int cur = 0;
    auto fetch = [&](int j0, Entry (&en)[kPer], int (&det)[kPer]) {
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        const int j = j0 + i * kBlock;
        en[i].local = kBinNone;
        det[i] = 0;
        if (j < total) {
          while (j >= seg_end[cur]) ++cur;
          en[i] = entries[seg_base[cur] + (uint32_t)j];
          det[i] = seg_d0[cur] + (int)(en[i].local >> 11);
        }
      }
    };
    auto weights = [&](const Entry (&en)[kPer], const int (&det)[kPer], int s, double (&m)[kPer]) {
#pragma unroll
      for (int i = 0; i < kPer; ++i) m[i] = en[i].local != kBinNone ? g.stokes_w[(size_t)det[i] * g.S + s] : 0.0;
    };
    auto add = [&](const Entry (&en)[kPer], int s, const double (&m)[kPer]) {
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        if (m[i] == 0.0) continue;  // zero weight: nothing to add (np.abs(P) entries that are 0); padding
        const uint32_t px = en[i].local & (uint32_t)(kBinRegionPx - 1);
        const double ww = en[i].weight();
        if constexpr (kNormal) {
          atomicAdd(&bin_acc[s * kBinRegionPx + px], m[i] * ww);
        } else {
          atomicAdd(&bin_acc[(s * 2) * kBinRegionPx + px], m[i] * (ww * (double)en[i].d));
          atomicAdd(&bin_acc[(s * 2 + 1) * kBinRegionPx + px], fabs(m[i]) * ww);
        }
      }
    };
    // Two trips in flight.  An entry needs a second, dependent load (its detector's Stokes weight); loads return
    // in order, so the weights of this trip are requested FIRST and the next trip's entries after them: waiting
    // for the weights then leaves the entries in flight (14.1 -> 12.6 ms at 10 000 x 240 000; the other order,
    // or one trip at a time, gains nothing).
    auto trip = [&](const Entry (&en)[kPer], const int (&det)[kPer], bool more, int j_next, Entry (&en_n)[kPer], int (&det_n)[kPer]) {
      double m[kPer];
      weights(en, det, 0, m);
      __builtin_amdgcn_sched_barrier(0);
      if (more) fetch(j_next, en_n, det_n);
      __builtin_amdgcn_sched_barrier(0);
      add(en, 0, m);
      for (int s = 1; s < g.S; ++s) {
        weights(en, det, s, m);
        add(en, s, m);
      }
    };
    Entry ea[kPer], eb[kPer];
    int da[kPer], db[kPer];
    constexpr int kTrip = kBlock * kPer;
    int j0 = threadIdx.x;
    if (j0 < total) fetch(j0, ea, da);
    while (j0 < total) {
      const bool more_b = j0 + kTrip < total;
      trip(ea, da, more_b, j0 + kTrip, eb, db);
      if (!more_b) break;
      const bool more_a = j0 + 2 * kTrip < total;
      trip(eb, db, more_a, j0 + 2 * kTrip, ea, da);
      if (!more_a) break;
      j0 += 2 * kTrip;
    }
    __syncthreads();
  }
  if (!any) return;  // uniform: n_seg is read by every thread between barriers
  const int per_plane = k.nby * k.nbx;
  const int chan = r / per_plane, rem = r - chan * per_plane;
  const int by = rem / k.nbx, bx = rem - by * k.nbx;
  const size_t plane = (size_t)g.n_eta * g.n_xi;
  for (int s = 0; s < g.S; ++s) {
    const size_t base = ((size_t)s * g.C + chan) * plane;
    for (int i = threadIdx.x; i < kBinRegionPx; i += kBlock) {
      const int e = (by << 5) + (i >> 6), x = (bx << 6) + (i & 63);
      if constexpr (kNormal) {
        const double v = bin_acc[s * kBinRegionPx + i];
        if (v == 0.0 || e >= g.n_eta || x >= g.n_xi) continue;
        atomicAdd(ml.y + base + (size_t)e * g.n_xi + x, v);
      } else {
        const double wv = bin_acc[(s * 2 + 1) * kBinRegionPx + i];
        if (wv == 0.0 || e >= g.n_eta || x >= g.n_xi) continue;
        atomicAdd(b.sum + base + (size_t)e * g.n_xi + x, bin_acc[(s * 2) * kBinRegionPx + i]);
        atomicAdd(b.wgt + base + (size_t)e * g.n_xi + x, wv);
      }
    }
  }
}

template <int kEntryBytes>
__global__ __launch_bounds__(kBlock) void bin_accumulate_kernel(MapArgs g, BinArgs b, BucketArgs k, int splits, MlArgs) {
  bin_accumulate_body<kEntryBytes, false>(g, b, k, splits, MlArgs{});
}

// pass B of mrx_map_normal_apply: the routed W (P x)_s b_c times w_k(d), summed per pixel in LDS, into y
__global__ __launch_bounds__(kBlock) void normal_accumulate_kernel(MapArgs g, BinArgs b, BucketArgs k, int splits, MlArgs m) {
  bin_accumulate_body<16, true>(g, b, k, splits, m);
}

// The tile of the atomic operators (bin_atomic_kernel, map_project_kernel, baseline_reduce_kernel): 16 detectors x 1024
// samples, four consecutive samples a thread.  The rows' constants go to the kernel's LDS (dets), the thread's samples'
// to registers (none without point), then the barrier.
template <bool kChain>
struct MapTile {
  int d0, nd, sb;  // the tile's first detector and its rows, the thread's first sample
  SampleConst sc[kSamplesPerThread];
  __device__ __forceinline__ MapTile(const MapArgs& g, DetConst* dets, bool point = true) {
    d0 = blockIdx.y * kTileDet;
    nd = min(kTileDet, g.D - d0);
    sb = blockIdx.x * kTileSamples + threadIdx.x * kSamplesPerThread;
    if ((int)threadIdx.x < nd) dets[threadIdx.x] = make_det_const(g, d0 + threadIdx.x);
    if (point) {
#pragma unroll
      for (int q = 0; q < kSamplesPerThread; ++q) {
        sample_const(g, sb + q, kChain, sc[q]);
        sc[q].s = min(max(sb + q, 0), g.T - 1);
      }
    }
    __syncthreads();
  }
  // the pixels and corner weights of the thread's sample q in row dc
  __device__ __forceinline__ MlCorners corners(const MapArgs& g, const DetConst& dc, int q) const {
    float ox, oy, el_d;
    sample_offsets<kChain, false>(g, dc, sc[q], ox, oy, el_d);
    return ml_corners(g, g.eta, g.xi, ox, oy);
  }
};

// mrx_map_project: out[d][s] = beta out[d][s] + alpha (P x)_s
template <bool kChain>
__global__ __launch_bounds__(kBlock) void map_project_kernel(MapArgs g, BinArgs b, MlArgs m) {
  __shared__ DetConst dets[kTileDet];
  const MapTile<kChain> t(g, dets);
  if (t.sb >= g.T) return;
  for (int dl = 0; dl < t.nd; ++dl) {
    const DetConst dc = dets[dl];
    const int d = t.d0 + dl;
    const int chan = det_channel(g, b, d);
    float* row = m.out + (size_t)d * m.ld_out;
#pragma unroll
    for (int q = 0; q < kSamplesPerThread; ++q) {
      const int s = t.sb + q;
      if (s >= g.T) break;
      double v = m.alpha * ml_gather(g, m, dc, chan, t.corners(g, dc, q));
      if (m.beta != 0.0) v = fma(m.beta, (double)row[s], v);  // (beta = 0: out is not read)
      row[s] = (float)v;
    }
  }
}

// ---- the destriper's baseline reduction ----
// mrx_baseline_reduce: y[d][b] += sum_{s in b} W mu (tod_s - alpha (P x)_s), hits[d][b] += sum_{s in b} W mu, on the tile
// of the atomic operators (MapTile).  With L >= 16 a thread's four samples lie in at most two baselines; each wave sums
// every baseline's run of lanes in float64 with a segmented shuffle reduction, the run's first lane adds the sum to the
// tile's LDS row, and the tile sends one float64 atomic per (detector, baseline) it touches: none per sample.
constexpr int kBaseMinL = 16;
constexpr int kBaseTileSeg = kTileSamples / kBaseMinL + 2;  // baselines a tile of 1024 samples meets at most

// the sums over a wave's runs of equal keys (each key's lanes contiguous): the run's first lane ends with the run's sums
template <bool kHits>
__device__ __forceinline__ void seg_sum(int key, double& v, double& h) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int ko = __shfl_down(key, off, 64);
    const double vo = __shfl_down(v, off, 64);
    double ho = 0.0;
    if (kHits) ho = __shfl_down(h, off, 64);
    if (lane + off < 64 && ko == key) {
      v += vo;
      if (kHits) h += ho;
    }
  }
}

template <bool kChain, bool kHits>
__global__ __launch_bounds__(kBlock) void baseline_reduce_kernel(MapArgs g, BinArgs b, MlArgs m) {
  __shared__ DetConst dets[kTileDet];
  __shared__ double acc[kHits ? 2 : 1][kTileDet][kBaseTileSeg];
  for (int i = threadIdx.x; i < (kHits ? 2 : 1) * kTileDet * kBaseTileSeg; i += kBlock) (&acc[0][0][0])[i] = 0.0;
  const bool point = m.x || m.mask;  // (uniform) the TOD alone, unmasked, needs no pixels
  const MapTile<kChain> t(g, dets, point);
  const int t0 = blockIdx.x * kTileSamples, sb = t.sb;
  const int b0 = t0 / m.L, nseg = (min(t0 + kTileSamples, g.T) - 1) / m.L - b0 + 1;  // the tile's baselines [b0, b0 + nseg)
  // (no early exit: every lane takes part in the shuffles; lanes past T add nothing, under a key of their own)
  const int kA = sb < g.T ? sb / m.L : 0x7ffffff0;
  const int lane = threadIdx.x & 63;
  const int prevA = __shfl_up(kA, 1, 64);
  const size_t plane = (size_t)g.n_eta * g.n_xi;
  for (int dl = 0; dl < t.nd; ++dl) {
    const DetConst dc = dets[dl];
    const int d = t.d0 + dl;
    const int chan = det_channel(g, b, d);
    const double det_w = det_weight(m, d);
    double vA = 0.0, hA = 0.0, vB = 0.0, hB = 0.0;  // the samples in baseline kA, and in kA + 1
#pragma unroll
    for (int q = 0; q < kSamplesPerThread; ++q) {
      const int s = sb + q;
      if (s >= g.T) break;
      double W = sample_weight(b, d, s) * det_w;
      double v = b.tod ? (double)b.tod[(size_t)d * b.ld_tod + s] : 0.0;
      if (point) {
        const MlCorners pc = t.corners(g, dc, q);
        if (m.mask && !m.mask[chan * plane + pc.o[0]]) W = 0.0;
        if (m.x) v = fma(-m.alpha, ml_gather(g, m, dc, chan, pc), v);
      }
      if (s / m.L == kA) {
        vA = fma(W, v, vA);
        hA += W;
      } else {
        vB = fma(W, v, vB);
        hB += W;
      }
    }
    seg_sum<kHits>(kA, vA, hA);
    seg_sum<kHits>(kA + 1, vB, hB);
    // run heads: the A keys run over the wave's lanes, and so do the B keys (kA + 1 steps with kA)
    if (lane == 0 || prevA != kA) {
      const int j = kA - b0;
      if (j >= 0 && j < nseg) {
        atomicAdd(&acc[0][dl][j], vA);
        if (kHits) atomicAdd(&acc[kHits ? 1 : 0][dl][j], hA);
      }
      const int jb = j + 1;
      if (jb >= 0 && jb < nseg) {
        atomicAdd(&acc[0][dl][jb], vB);
        if (kHits) atomicAdd(&acc[kHits ? 1 : 0][dl][jb], hB);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < t.nd * nseg; i += kBlock) {
    const int dl = i / nseg, j = i - dl * nseg;
    const size_t at = (size_t)(t.d0 + dl) * m.nb + (b0 + j);
    if (m.y && acc[0][dl][j] != 0.0) atomicAdd(m.y + at, acc[0][dl][j]);
    if (kHits && acc[kHits ? 1 : 0][dl][j] != 0.0) atomicAdd(m.hits + at, acc[kHits ? 1 : 0][dl][j]);
  }
}

// One run of a thread's consecutive samples with the same pixels (bin_atomic_kernel): the corners' sums go out with one
// atomic per corner, plane and product
template <int kSrc>
__device__ __forceinline__ void flush_corners(const MapArgs& g, const BinArgs& b, const MlArgs& m, const DetConst& dc, int chan,
                                              const int (&o)[4], const double (&A)[4], const double (&B)[4]) {
  const size_t plane = (size_t)g.n_eta * g.n_xi;
  const int corners = g.bilinear ? 4 : 1;
  if constexpr (kSrc == kSrcTod) {
    for (int k = 0; k < g.S; ++k) {
      const size_t base = ((size_t)k * g.C + chan) * plane;
      const double w = dc.w[k];
      for (int c = 0; c < corners; ++c) {
        if (B[c] == 0.0) continue;  // zero weight: nothing to add (np.abs(P) entries that are 0)
        atomicAdd(b.sum + base + o[c], w * A[c]);
        atomicAdd(b.wgt + base + o[c], fabs(w) * B[c]);
      }
    }
  } else if constexpr (kSrc == kSrcBlocks) {
    int idx = 0;  // H[k, l], k <= l, row-major
    for (int k = 0; k < g.S; ++k)
      for (int l = k; l < g.S; ++l, ++idx) {
        const double wkl = dc.w[k] * dc.w[l];
        double* h = m.y + ((size_t)idx * g.C + chan) * plane;
        for (int c = 0; c < corners; ++c)
          if (A[c] != 0.0 && wkl != 0.0) atomicAdd(h + o[c], wkl * A[c]);
      }
  } else {
    for (int k = 0; k < g.S; ++k) {
      if (dc.w[k] == 0.0) continue;
      double* y = m.y + ((size_t)k * g.C + chan) * plane;
      for (int c = 0; c < corners; ++c)
        if (A[c] != 0.0) atomicAdd(y + o[c], dc.w[k] * A[c]);
    }
  }
}

// The atomic form of the binning and of the map-maker's operators: float64 atomics with run merging -- a thread's
// consecutive samples of a row that share their pixels are summed per corner and flushed once.  Per source, A[c] =
// kSrcTod: sum W D b_c, with B[c] = sum W b_c (the binning's two maps; a corner goes out where B[c] != 0);
// kSrcNormal: sum W (P x)_s b_c;  kSrcBaselines: sum W a[d][s / L] b_c;  kSrcBlocks: sum W b_c^2 (the block diagonal)
template <bool kChain, int kSrc>
__global__ __launch_bounds__(kBlock) void bin_atomic_kernel(MapArgs g, BinArgs b, MlArgs m) {
  __shared__ DetConst dets[kTileDet];
  const MapTile<kChain> t(g, dets);
  if (t.sb >= g.T) return;
  for (int dl = 0; dl < t.nd; ++dl) {
    const DetConst dc = dets[dl];
    const int d = t.d0 + dl;
    const int chan = det_channel(g, b, d);
    const double det_w = kSrc == kSrcTod ? 1.0 : det_weight(m, d);
    int o[4] = {0, 0, 0, 0};
    double A[4] = {0.0, 0.0, 0.0, 0.0}, B[4] = {0.0, 0.0, 0.0, 0.0};
    bool open = false;
#pragma unroll
    for (int q = 0; q < kSamplesPerThread; ++q) {
      const int s = t.sb + q;
      if (s >= g.T) break;
      const MlCorners pc = t.corners(g, dc, q);
      double W = sample_weight(b, d, s) * det_w;
      if constexpr (kSrc == kSrcBaselines) W *= m.amp[(size_t)d * m.nb + s / m.L];
      if constexpr (kSrc == kSrcNormal) W *= ml_gather(g, m, dc, chan, pc);
      const double WD = kSrc == kSrcTod ? W * (double)b.tod[(size_t)d * b.ld_tod + s] : 0.0;
      if (open && (pc.o[0] != o[0] || pc.o[1] != o[1] || pc.o[2] != o[2] || pc.o[3] != o[3])) {
        flush_corners<kSrc>(g, b, m, dc, chan, o, A, B);
        open = false;
      }
      if (!open) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          o[c] = pc.o[c];
          A[c] = B[c] = 0.0;
        }
        open = true;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if constexpr (kSrc == kSrcTod) {
          A[c] = fma(WD, pc.w[c], A[c]);
          B[c] = fma(W, pc.w[c], B[c]);
        } else {
          A[c] = fma(W, kSrc == kSrcBlocks ? pc.w[c] * pc.w[c] : pc.w[c], A[c]);
        }
      }
    }
    if (open) flush_corners<kSrc>(g, b, m, dc, chan, o, A, B);
  }
}

// mrx_map_block_solve: one thread per (channel, pixel); H [S(S+1)/2][n], r and z [S][n], n = C x pixels
__global__ __launch_bounds__(kBlock) void block_solve_kernel(int S, long long n, const double* __restrict__ H, const double* r,
                                                             double rcond, int nan_invalid, double* z, uint8_t* __restrict__ mask) {
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    double a[3][3] = {}, inv[3][3] = {};
    for (int k = 0, idx = 0; k < S; ++k)
      for (int l = k; l < S; ++l, ++idx) a[k][l] = a[l][k] = H[(size_t)idx * n + i];
    // H = L D L^T (L unit lower triangular), then H^-1 column by column: a rank-deficient block leaves a pivot at rounding
    // level and a huge inverse (its adjugate and determinant would both vanish, their ratio meaning nothing)
    double L[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}}, dg[3] = {1.0, 1.0, 1.0};
    bool ok = a[0][0] > 0.0 && isfinite(a[0][0]);
    for (int j = 0; j < S && ok; ++j) {
      double dj = a[j][j];
      for (int m = 0; m < j; ++m) dj -= L[j][m] * L[j][m] * dg[m];
      dg[j] = dj;
      ok = dj > 0.0;
      for (int r2 = j + 1; r2 < S && ok; ++r2) {
        double v = a[r2][j];
        for (int m = 0; m < j; ++m) v -= L[r2][m] * L[j][m] * dg[m];
        L[r2][j] = v / dj;
      }
    }
    if (ok) {
      for (int c = 0; c < S; ++c) {  // solve L D L^T x = e_c
        double y[3];
        for (int r2 = 0; r2 < S; ++r2) {
          double v = r2 == c ? 1.0 : 0.0;
          for (int m = 0; m < r2; ++m) v -= L[r2][m] * y[m];
          y[r2] = v;
        }
        for (int r2 = 0; r2 < S; ++r2) y[r2] /= dg[r2];
        for (int r2 = S - 1; r2 >= 0; --r2) {
          double v = y[r2];
          for (int m = r2 + 1; m < S; ++m) v -= L[m][r2] * inv[m][c];
          inv[r2][c] = v;
        }
      }
      // reciprocal condition number in the 1-norm, 1 / (|H|_1 |H^-1|_1) (LAPACK's, exact for S <= 3)
      double na = 0.0, ni = 0.0;
      for (int l = 0; l < S; ++l) {
        double ca = 0.0, ci = 0.0;
        for (int k = 0; k < S; ++k) {
          ca += fabs(a[k][l]);
          ci += fabs(inv[k][l]);
        }
        na = fmax(na, ca);
        ni = fmax(ni, ci);
      }
      ok = isfinite(ni) && 1.0 / (na * ni) >= rcond;
    }
    double rv[3] = {}, zv[3];
    for (int k = 0; k < S; ++k) rv[k] = r[(size_t)k * n + i];
    for (int k = 0; k < S; ++k) {
      double v = 0.0;
      for (int l = 0; l < S; ++l) v = fma(inv[k][l], rv[l], v);
      zv[k] = ok ? v : (nan_invalid ? __builtin_nan("") : 0.0);
    }
    for (int k = 0; k < S; ++k) z[(size_t)k * n + i] = zv[k];  // (after every read of r: z may be r)
    if (mask) mask[i] = ok ? 1 : 0;
  }
}

}  // namespace

extern "C" {

// The arguments of the operators on the binning's pointing (the binning, the map-maker's and the destriper's): the map,
// the pointing, the TOD (or null), the sample weights (or null) and the per-detector weights (or null).
static int op_args(mrx_ctx* ctx, const mrx_sky_map* map, const float* d_tod, size_t ld_tod, const float* d_weight, size_t ld_weight,
                   const double* d_det_weight, const float* d_az, const float* d_el, int T, const double* d_transform,
                   const float* d_dx, const float* d_dy, const double* d_stokes_w, const int32_t* d_channel, int D, MapArgs& g,
                   BinArgs& b, MlArgs& m) {
  MRX_REQUIRE(ctx, map && d_az && d_el && d_dx && d_dy && d_stokes_w, "null pointer");
  MRX_REQUIRE(ctx, map->n_channels >= 1 && map->n_stokes >= 1 && map->n_stokes <= kMaxStokes &&
                       map->n_eta >= 2 && map->n_xi >= 2,
              "need n_channels >= 1, 1 <= n_stokes <= 4, n_eta >= 2, n_xi >= 2");
  MRX_REQUIRE(ctx, map->deta != 0.0 && map->dxi != 0.0, "map axes need a non-zero step");
  MRX_REQUIRE(ctx, (long long)map->n_eta * map->n_xi < (1LL << 31), "a map plane must hold fewer than 2^31 pixels");
  MRX_REQUIRE(ctx, (!d_tod || ld_tod >= (size_t)T) && (!d_weight || ld_weight >= (size_t)T), "leading dimension smaller than T");
  MRX_REQUIRE(ctx, mrx_ceil_div(D, kTileDet) <= 65535, "D too large for one launch");
  g = map_args(map, d_az, d_el, T, d_transform, d_dx, d_dy, d_stokes_w, D);
  b = BinArgs{d_tod, ld_tod, d_weight, ld_weight, d_channel, nullptr, nullptr};
  m = MlArgs{};
  m.det_weight = d_det_weight;
  return MRX_OK;
}

// a kernel on the tile grid of the atomic operators (MapTile), in the pointing form the context selects
typedef void (*TileKernel)(MapArgs, BinArgs, MlArgs);
static int launch_tiles(mrx_ctx* ctx, TileKernel chain_form, TileKernel composed_form, const MapArgs& g, const BinArgs& b,
                        const MlArgs& m) {
  const dim3 grid(mrx_ceil_div(g.T, kTileSamples), mrx_ceil_div(g.D, kTileDet));
  hipLaunchKernelGGL(ctx->options[MRX_OPT_POINTING_CHAIN] ? chain_form : composed_form, grid, dim3(kBlock), 0, ctx->stream, g, b, m);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_bin_map(mrx_ctx* ctx, const mrx_sky_map* map, const float* d_tod, size_t ld_tod,
                const float* d_weight, size_t ld_weight, const float* d_az, const float* d_el, int T,
                const double* d_transform, const float* d_dx, const float* d_dy,
                const double* d_stokes_w, const int32_t* d_channel, int D, double* d_sum,
                double* d_wgt) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, D >= 0 && T >= 0, "negative size");
  if (D == 0 || T == 0) return MRX_OK;
  MRX_REQUIRE(ctx, d_tod && d_sum && d_wgt, "null pointer");
  MapArgs g;
  BinArgs b;
  MlArgs m;
  const int rc = op_args(ctx, map, d_tod, ld_tod, d_weight, ld_weight, nullptr, d_az, d_el, T, d_transform, d_dx, d_dy, d_stokes_w,
                         d_channel, D, g, b, m);
  if (rc != MRX_OK) return rc;
  b.sum = d_sum;
  b.wgt = d_wgt;
  return launch_tiles(ctx, bin_atomic_kernel<true, kSrcTod>, bin_atomic_kernel<false, kSrcTod>, g, b, m);
}

// regions of a map for the bucketed form, or 0 when it does not apply
static int bin_regions(const mrx_sky_map* map, int* nbx, int* nby) {
  if (!map || map->n_eta < 2 || map->n_xi < 2 || map->n_channels < 1) return 0;
  *nbx = mrx_ceil_div(map->n_xi, kBinBx);
  *nby = mrx_ceil_div(map->n_eta, kBinBy);
  const long long R = (long long)map->n_channels * *nbx * *nby;
  return R <= kBinMaxRegions ? (int)R : 0;
}

// tile geometry of the form a map takes
struct BinGeometry {
  int tile_det, tile_samples, tile_entries;
  size_t lds_a;
};

static BinGeometry bin_geometry(bool bilinear, int R) {
  BinGeometry q;
  if (bilinear) {
    q.tile_det = BinTile<true>::kDet;
    q.tile_samples = BinTile<true>::kSamples;
    q.tile_entries = BinTile<true>::kEntries;
  } else {
    q.tile_det = BinTile<false>::kDet;
    q.tile_samples = BinTile<false>::kSamples;
    q.tile_entries = BinTile<false>::kEntries;
  }
  // sort words at 3 bytes each (two arrays), one word per region (count, then cursor), the bilinear form's offsets
  q.lds_a = (size_t)q.tile_entries * 3 + (size_t)R * sizeof(uint32_t) +
            (bilinear ? (size_t)q.tile_det * q.tile_samples * sizeof(float2) : 0);
  return q;
}

int mrx_bin_map_work_bytes(const mrx_sky_map* map, int D, int T, size_t* min_bytes, size_t* full_bytes) {
  int nbx, nby;
  const int R = bin_regions(map, &nbx, &nby);
  if (!R || D < 1 || T < 1 || !min_bytes || !full_bytes) return R ? MRX_ERR_INVALID : MRX_ERR_UNSUPPORTED;
  const BinGeometry q = bin_geometry(map->bilinear != 0, R);
  // one column of tiles (all detectors x one tile of samples): its slots and its words of the table
  // (sized for the largest entry: the nearest-pixel forms need 12 or 8 of the 16 bytes)
  const size_t col = (size_t)mrx_ceil_div(D, q.tile_det) * ((size_t)q.tile_entries * 16 + (size_t)R * sizeof(uint32_t));
  *min_bytes = col;
  *full_bytes = col * (size_t)mrx_ceil_div(T, q.tile_samples);
  return MRX_OK;
}

// The routed form (mrx_bin_map_bucketed, mrx_map_normal_apply, mrx_bin_map_baselines): the time axis in chunks of
// whole columns of tiles, as many as the work buffer holds; per chunk pass A routes the contributions to the map's
// regions, bin_order_kernel ranks the regions and pass B sums each region in LDS into the map.  entry_bytes: of a routed
// contribution; lds_b: pass B's dynamic LDS; too_small: the message for a buffer below one column, which names the
// caller's sizing function.
typedef void (*PassA)(MapArgs, BinArgs, BucketArgs, MlArgs);
typedef void (*PassB)(MapArgs, BinArgs, BucketArgs, int, MlArgs);
static int routed_bin(mrx_ctx* ctx, const MapArgs& g, const BinArgs& b, const MlArgs& m, BucketArgs k, PassA pass_a,
                      PassB pass_b, int entry_bytes, size_t lds_b, void* d_work, size_t work_bytes, const char* too_small) {
  const BinGeometry q = bin_geometry(g.bilinear != 0, k.R);
  k.tile_det = q.tile_det;
  k.tile_entries = q.tile_entries;
  const int tiles_y = mrx_ceil_div(g.D, q.tile_det);
  MRX_REQUIRE(ctx, tiles_y <= 65535, "D too large for one launch");
  const size_t col = (size_t)tiles_y * ((size_t)q.tile_entries * entry_bytes + (size_t)k.R * sizeof(uint32_t));
  MRX_REQUIRE(ctx, d_work && (reinterpret_cast<uintptr_t>(d_work) & 15u) == 0 && work_bytes >= col, too_small);
  const int cols_total = mrx_ceil_div(g.T, q.tile_samples);
  int cols = (int)(work_bytes / col < (size_t)cols_total ? work_bytes / col : (size_t)cols_total);
  // pass B indexes the entries of a chunk with 32 bits
  while ((long long)cols * tiles_y * q.tile_entries > (1LL << 32) - 1) cols = (cols + 1) / 2;
  MRX_LDS_CAP(ctx, pass_a, q.lds_a);
  MRX_LDS_CAP(ctx, pass_b, lds_b);
  if (!ctx->d_bin_order) MRX_HIP(ctx, hipMalloc(&ctx->d_bin_order, sizeof(uint32_t) * 2 * kBinMaxRegions));
  k.totals = ctx->d_bin_order;
  k.order = reinterpret_cast<const int*>(ctx->d_bin_order + kBinMaxRegions);
  // enough workgroups per region to fill the chip: the regions under the scan hold most samples
  // (round 4, onto 1024^2, regions in dispatch order: 8192 items 28.4 ms, 16384 26.8, 32768 25.6, 65536 25.3, 131072 26.2 for
  //  the call; heaviest regions first: 23.6 / 22.5 / 22.6 / 22.3 / 23.1 from 16384 to 262144)
  const int splits = 65536 / k.R < 1 ? 1 : 65536 / k.R;
  // the table right behind the entries is 16-byte aligned whatever the entry size (8, 12 or 16 bytes)
  static_assert(BinTile<true>::kEntries % 4 == 0 && BinTile<false>::kEntries % 4 == 0, "a tile holds a multiple of 4 entries");
  for (int c0 = 0; c0 < cols_total; c0 += cols) {
    const int nc = cols_total - c0 < cols ? cols_total - c0 : cols;
    k.tiles_x = nc;
    k.n_tiles = nc * tiles_y;
    k.s0 = c0 * q.tile_samples;
    k.s1 = (long long)(c0 + nc) * q.tile_samples < (long long)g.T ? (c0 + nc) * q.tile_samples : g.T;
    k.entries = d_work;
    k.tab = reinterpret_cast<uint32_t*>(static_cast<char*>(d_work) + (size_t)k.n_tiles * q.tile_entries * entry_bytes);
    MRX_HIP(ctx, hipMemsetAsync(k.tab, 0, (size_t)k.R * k.n_tiles * sizeof(uint32_t), ctx->stream));
    MRX_HIP(ctx, hipMemsetAsync(k.totals, 0, (size_t)k.R * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(pass_a, dim3(nc, tiles_y), dim3(kBlock), q.lds_a, ctx->stream, g, b, k, m);
    hipLaunchKernelGGL(bin_order_kernel, dim3(1), dim3(1024), 0, ctx->stream, k.totals, k.R, const_cast<int*>(k.order));
    const int sp = splits < k.n_tiles ? splits : k.n_tiles;
    hipLaunchKernelGGL(pass_b, dim3(k.R, sp), dim3(kBlock), lds_b, ctx->stream, g, b, k, sp, m);
    MRX_CHECK_LAUNCH(ctx);
  }
  return MRX_OK;
}

int mrx_bin_map_bucketed(mrx_ctx* ctx, const mrx_sky_map* map, const float* d_tod, size_t ld_tod,
                         const float* d_weight, size_t ld_weight, const float* d_az, const float* d_el, int T,
                         const double* d_transform, const float* d_dx, const float* d_dy,
                         const double* d_stokes_w, const int32_t* d_channel, int D, double* d_sum,
                         double* d_wgt, void* d_work, size_t work_bytes) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, D >= 0 && T >= 0, "negative size");
  if (D == 0 || T == 0) return MRX_OK;
  BucketArgs k{};
  k.R = bin_regions(map, &k.nbx, &k.nby);
  if (!k.R)
    return mrx_fail(ctx, MRX_ERR_UNSUPPORTED, "mrx_bin_map_bucketed: maps of at most %d regions of %d x %d pixels (use mrx_bin_map)",
                    kBinMaxRegions, kBinBx, kBinBy);
  MRX_REQUIRE(ctx, d_tod && d_sum && d_wgt, "null pointer");
  MapArgs g;
  BinArgs b;
  MlArgs m;
  const int rc = op_args(ctx, map, d_tod, ld_tod, d_weight, ld_weight, nullptr, d_az, d_el, T, d_transform, d_dx, d_dy, d_stokes_w,
                         d_channel, D, g, b, m);
  if (rc != MRX_OK) return rc;
  b.sum = d_sum;
  b.wgt = d_wgt;
  const bool bil = map->bilinear != 0, wts = d_weight != nullptr, chain = ctx->options[MRX_OPT_POINTING_CHAIN] != 0;
  const PassA pass_a = bil ? (chain ? bin_bucket_kernel<true, true, true> : bin_bucket_kernel<false, true, true>)
                       : wts ? (chain ? bin_bucket_kernel<true, false, true> : bin_bucket_kernel<false, false, true>)
                             : (chain ? bin_bucket_kernel<true, false, false> : bin_bucket_kernel<false, false, false>);
  const PassB pass_b = bil ? bin_accumulate_kernel<16> : wts ? bin_accumulate_kernel<12> : bin_accumulate_kernel<8>;
  return routed_bin(ctx, g, b, m, k, pass_a, pass_b, bin_entry_bytes(bil, wts), (size_t)g.S * 2 * kBinRegionPx * sizeof(double),
                    d_work, work_bytes, "work buffer: 16-byte aligned, at least mrx_bin_map_work_bytes' minimum");
}

// ---- the maximum-likelihood map-maker's operators ----

int mrx_map_project(mrx_ctx* ctx, const mrx_sky_map* map, const double* d_x, const float* d_az, const float* d_el, int T,
                    const double* d_transform, const float* d_dx, const float* d_dy, const double* d_stokes_w,
                    const int32_t* d_channel, int D, double alpha, double beta, float* d_out, size_t ld_out) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, D >= 0 && T >= 0, "negative size");
  if (D == 0 || T == 0) return MRX_OK;
  MRX_REQUIRE(ctx, d_x && d_out, "null pointer");
  MRX_REQUIRE(ctx, ld_out >= (size_t)T, "ld_out smaller than T");
  MapArgs g;
  BinArgs b;
  MlArgs m;
  const int rc = op_args(ctx, map, nullptr, 0, nullptr, 0, nullptr, d_az, d_el, T, d_transform, d_dx, d_dy, d_stokes_w, d_channel,
                         D, g, b, m);
  if (rc != MRX_OK) return rc;
  m.x = d_x;
  m.out = d_out;
  m.ld_out = ld_out;
  m.alpha = alpha;
  m.beta = beta;
  return launch_tiles(ctx, map_project_kernel<true>, map_project_kernel<false>, g, b, m);
}

// the routed form of an operator that routes a float64 per sample (mrx_map_normal_apply, mrx_bin_map_baselines): 16-byte
// entries, pass B normal_accumulate_kernel
static int ml_routed(mrx_ctx* ctx, const MapArgs& g, const BinArgs& b, const MlArgs& m, const BucketArgs& k, PassA pass_a,
                     void* d_work, size_t work_bytes) {
  return routed_bin(ctx, g, b, m, k, pass_a, normal_accumulate_kernel, 16, (size_t)g.S * kBinRegionPx * sizeof(double), d_work,
                    work_bytes, "work buffer: 16-byte aligned, at least mrx_map_normal_work_bytes' minimum (or NULL: the atomic form)");
}

int mrx_map_normal_work_bytes(const mrx_sky_map* map, int D, int T, size_t* min_bytes, size_t* full_bytes) {
  int nbx, nby;
  if (!min_bytes || !full_bytes) return MRX_ERR_INVALID;
  if (map && !bin_regions(map, &nbx, &nby)) {  // the atomic form: no buffer
    *min_bytes = *full_bytes = 0;
    return map->n_eta >= 2 && map->n_xi >= 2 && map->n_channels >= 1 ? MRX_OK : MRX_ERR_INVALID;
  }
  return mrx_bin_map_work_bytes(map, D, T, min_bytes, full_bytes);  // (sized for 16-byte entries: the ones this form routes)
}

int mrx_map_normal_apply(mrx_ctx* ctx, const mrx_sky_map* map, const double* d_x, const float* d_weight, size_t ld_weight,
                         const double* d_det_weight, const float* d_az, const float* d_el, int T, const double* d_transform,
                         const float* d_dx, const float* d_dy, const double* d_stokes_w, const int32_t* d_channel, int D,
                         double* d_y, void* d_work, size_t work_bytes) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, D >= 0 && T >= 0, "negative size");
  if (D == 0 || T == 0) return MRX_OK;
  MRX_REQUIRE(ctx, d_x && d_y, "null pointer");
  MapArgs g;
  BinArgs b;
  MlArgs m;
  const int rc = op_args(ctx, map, nullptr, 0, d_weight, ld_weight, d_det_weight, d_az, d_el, T, d_transform, d_dx, d_dy,
                         d_stokes_w, d_channel, D, g, b, m);
  if (rc != MRX_OK) return rc;
  m.x = d_x;
  m.y = d_y;
  BucketArgs k{};
  k.R = bin_regions(map, &k.nbx, &k.nby);
  if (!k.R || !d_work) return launch_tiles(ctx, bin_atomic_kernel<true, kSrcNormal>, bin_atomic_kernel<false, kSrcNormal>, g, b, m);
  const bool bil = map->bilinear != 0, chain = ctx->options[MRX_OPT_POINTING_CHAIN] != 0;
  const PassA pass_a = bil ? (chain ? normal_bucket_kernel<true, true> : normal_bucket_kernel<false, true>)
                           : (chain ? normal_bucket_kernel<true, false> : normal_bucket_kernel<false, false>);
  return ml_routed(ctx, g, b, m, k, pass_a, d_work, work_bytes);
}

int mrx_bin_map_blocks(mrx_ctx* ctx, const mrx_sky_map* map, const float* d_weight, size_t ld_weight,
                       const double* d_det_weight, const float* d_az, const float* d_el, int T, const double* d_transform,
                       const float* d_dx, const float* d_dy, const double* d_stokes_w, const int32_t* d_channel, int D,
                       double* d_blocks) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, D >= 0 && T >= 0, "negative size");
  if (D == 0 || T == 0) return MRX_OK;
  MRX_REQUIRE(ctx, d_blocks, "null pointer");
  MapArgs g;
  BinArgs b;
  MlArgs m;
  const int rc = op_args(ctx, map, nullptr, 0, d_weight, ld_weight, d_det_weight, d_az, d_el, T, d_transform, d_dx, d_dy,
                         d_stokes_w, d_channel, D, g, b, m);
  if (rc != MRX_OK) return rc;
  m.y = d_blocks;
  return launch_tiles(ctx, bin_atomic_kernel<true, kSrcBlocks>, bin_atomic_kernel<false, kSrcBlocks>, g, b, m);
}

int mrx_map_block_solve(mrx_ctx* ctx, int n_stokes, int n_channels, long long n_pix, const double* d_blocks,
                        const double* d_rhs, double rcond, int nan_invalid, double* d_z, uint8_t* d_mask) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, n_stokes >= 1 && n_stokes <= 3 && n_channels >= 1 && n_pix >= 0, "need 1 <= n_stokes <= 3, n_channels >= 1");
  if (n_pix == 0) return MRX_OK;
  MRX_REQUIRE(ctx, d_blocks && d_rhs && d_z, "null pointer");
  const long long n = (long long)n_channels * n_pix;
  const unsigned blocks = (unsigned)std::min<long long>((n + kBlock - 1) / kBlock, 65536LL);
  hipLaunchKernelGGL(block_solve_kernel, dim3(blocks), dim3(kBlock), 0, ctx->stream, n_stokes, n, d_blocks, d_rhs, rcond,
                     nan_invalid, d_z, d_mask);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

// ---- the destriper's operators ----

// what the destriper's operators take: L >= 16 samples, nearest-pixel pointing
static int baseline_check(mrx_ctx* ctx, const mrx_sky_map* map, int L) {
  if (L < kBaseMinL) return mrx_fail(ctx, MRX_ERR_INVALID, "baseline length %d samples: at least %d", L, kBaseMinL);
  if (map && map->bilinear) return mrx_fail(ctx, MRX_ERR_UNSUPPORTED, "the destriper's operators take nearest-pixel pointing only");
  return MRX_OK;
}

int mrx_baseline_reduce(mrx_ctx* ctx, const mrx_sky_map* map, const float* d_tod, size_t ld_tod, const double* d_x,
                        double alpha, const float* d_weight, size_t ld_weight, const double* d_det_weight,
                        const uint8_t* d_mask, int L, const float* d_az, const float* d_el, int T, const double* d_transform,
                        const float* d_dx, const float* d_dy, const double* d_stokes_w, const int32_t* d_channel, int D,
                        double* d_y, double* d_hits) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, D >= 0 && T >= 0, "negative size");
  const int brc = baseline_check(ctx, map, L);
  if (brc != MRX_OK) return brc;
  const int nb = (int)(((long long)T + L - 1) / L);
  if (D == 0 || T == 0) return MRX_OK;
  MRX_REQUIRE(ctx, d_y || d_hits, "null pointer: neither d_y nor d_hits");
  MapArgs g;
  BinArgs b;
  MlArgs m;
  const int rc = op_args(ctx, map, d_tod, ld_tod, d_weight, ld_weight, d_det_weight, d_az, d_el, T, d_transform, d_dx, d_dy,
                         d_stokes_w, d_channel, D, g, b, m);
  if (rc != MRX_OK) return rc;
  m.x = d_x;
  m.alpha = alpha;
  m.mask = d_mask;
  m.L = L;
  m.nb = nb;
  m.y = d_y;
  m.hits = d_hits;
  return d_hits ? launch_tiles(ctx, baseline_reduce_kernel<true, true>, baseline_reduce_kernel<false, true>, g, b, m)
                : launch_tiles(ctx, baseline_reduce_kernel<true, false>, baseline_reduce_kernel<false, false>, g, b, m);
}

int mrx_bin_map_baselines(mrx_ctx* ctx, const mrx_sky_map* map, const double* d_amp, int L, const float* d_weight,
                          size_t ld_weight, const double* d_det_weight, const float* d_az, const float* d_el, int T,
                          const double* d_transform, const float* d_dx, const float* d_dy, const double* d_stokes_w,
                          const int32_t* d_channel, int D, double* d_y, void* d_work, size_t work_bytes) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, D >= 0 && T >= 0, "negative size");
  const int brc = baseline_check(ctx, map, L);
  if (brc != MRX_OK) return brc;
  const int nb = (int)(((long long)T + L - 1) / L);
  if (D == 0 || T == 0) return MRX_OK;
  MRX_REQUIRE(ctx, d_amp && d_y, "null pointer");
  MapArgs g;
  BinArgs b;
  MlArgs m;
  const int rc = op_args(ctx, map, nullptr, 0, d_weight, ld_weight, d_det_weight, d_az, d_el, T, d_transform, d_dx, d_dy,
                         d_stokes_w, d_channel, D, g, b, m);
  if (rc != MRX_OK) return rc;
  m.amp = d_amp;
  m.L = L;
  m.nb = nb;
  m.y = d_y;
  BucketArgs k{};
  k.R = bin_regions(map, &k.nbx, &k.nby);
  if (!k.R || !d_work) return launch_tiles(ctx, bin_atomic_kernel<true, kSrcBaselines>, bin_atomic_kernel<false, kSrcBaselines>, g, b, m);
  return ml_routed(ctx, g, b, m, k, ctx->options[MRX_OPT_POINTING_CHAIN] ? baseline_bucket_kernel<true> : baseline_bucket_kernel<false>,
                   d_work, work_bytes);
}

}  // extern "C"
