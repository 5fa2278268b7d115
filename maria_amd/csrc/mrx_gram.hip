// The flag-aware Gram matrix of the rows of a [D, T] TOD on the matrix cores (maria_amd/covariance.py):
//   term(d, t) = (double)x[d][t] - (double)model[d][t]                       (plain (double)x without a model)
//   z(d, t)    = flags[d][t] == 0 ? (float)(term(d, t) - center[d]) : 0.0f   (one float64 subtraction, one rounding)
//   G[i][j]    = sum over t of z(rows[i], t) * z(rows[j], t),   n[i][j] = |{ t : both unflagged }|
// The file is built without FMA contraction: the subtractions and the float64 additions are one rounding each.
//
// A workgroup of 256 threads (four waves) takes one 128 x 128 block (bi, bj) of G with bj >= bi and walks ALL of time in
// panels of 32 samples.  A panel of each of the two row blocks is staged through LDS as z, [row][parity][16]: model, centre
// and flag select happen once per element on the way in; a diagonal block stages one panel.  The loads of the next panel are
// issued before the multiplications of this one and waited for after them.  Rows past R, rows the list
// names outside 0 .. D - 1 and samples past T are staged as zeros and never loaded.  Staging ownership does not depend on
// alignment: thread o owns the four samples 4 (o & 7) .. + 3 of the rows (o >> 3) + 32 p, p = 0 .. 3, of a panel, one
// 16-byte load (flags: 4-byte) where pointer and pitch allow it, four otherwise.
//
// Wave w holds the 64 x 64 quadrant (w >> 1, w & 1) as 2 x 2 tiles of 32 x 32, 64 float32 accumulators a lane, fed by
// v_mfma_f32_32x32x2_f32: lane l gives A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31], both read from the z
// panels, and holds C/D at col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).  The instruction is bit for bit the
// float32 fmaf chain in ascending k, so an accumulator is the chain over ascending t.  Every MRX_GRAM_BLOCK samples from
// t = 0, and at the end, each accumulator is added to its float64 shadow (one rounding) and set to 0.0f: the order is a
// function of T alone.  No atomics, no split of time across workgroups.  The block below the diagonal is the mirror of
// the one above it, written by the same lanes from the same registers; inside a diagonal block both halves are
// computed, a * b and b * a being the same product.
//
// The counts are a second instance of the kernel on the 0/1 weights (z = unflagged ? 1.0f : 0.0f, no read of x): a
// block's float32 sums are integers <= MRX_GRAM_BLOCK, exact, and their shadows are uint32.  Without flags the counts are
// T or 0 and a fill kernel writes them; without d_n nothing is launched for them.
#include "mrx_internal.h"

#include <type_traits>

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 128;   // rows and columns of G a workgroup holds
constexpr int kPanel = 32;   // samples staged at a time
constexpr int kOwn = 4;      // consecutive samples of a thread in the staging
// a panel in LDS is [row][parity][16]: the sample t0 + 2 j + parity of a row at j, so that a lane's 16 operands of a
// panel (its row, its half of the wave as the parity) are four 16-byte reads.  36 floats between rows: 16 consecutive
// lanes then cover the 64 banks once
constexpr int kRowStride = kPanel + 4;
constexpr int kPast = -2;    // a row past R: nothing is written for it
constexpr int kNoRow = -1;   // a row the list names outside 0 .. D - 1: zeros
static_assert(MRX_GRAM_BLOCK % kPanel == 0 && MRX_GRAM_BLOCK <= 1024 && (MRX_GRAM_BLOCK & (MRX_GRAM_BLOCK - 1)) == 0,
              "MRX_GRAM_BLOCK: a power of two <= 1024 and a multiple of the panel");

enum : int { kWideX = 1, kWideM = 2, kWideF = 4 };

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x16 mfma_32x32x2(float a, float b, f32x16 c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
#else
  return c;
#endif
}

// The staging is two phases.  The LOAD phase only loads: it computes nothing from a loaded value and gives no register a
// default, so that no load waits for another; what it leaves unset (a row that is not there, a sample past T) is never
// looked at, because the STORE phase repeats the same tests before it takes a value.

// may the thread's four samples q .. q + 3 be one access?
__device__ __forceinline__ bool whole(long long q, int T, int wide, int bit) { return (wide & bit) && q + kOwn <= T; }

// (not mrx_tod_dev.h's load_own, which gives a sample past T the default 0: see above)
__device__ __forceinline__ void load4(const float* row, long long q, int T, bool one, float (&v)[kOwn]) {
  if (one) {
    const float4 w = *reinterpret_cast<const float4*>(row + q);
    v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
  } else {
#pragma unroll
    for (int k = 0; k < kOwn; ++k)
      if (q + k < T) v[k] = row[q + k];
  }
}

// the flags as loaded: one word in f[0], or a byte in each f[k]
__device__ __forceinline__ void load4(const unsigned char* row, long long q, int T, bool one, unsigned (&f)[kOwn]) {
  if (one) {
    f[0] = *reinterpret_cast<const unsigned*>(row + q);
  } else {
#pragma unroll
    for (int k = 0; k < kOwn; ++k)
      if (q + k < T) f[k] = row[q + k];
  }
}

// eight consecutive floats of LDS, 16-byte aligned
__device__ __forceinline__ void read8(const float* p, float (&v)[8]) {
  const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
  v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w, v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
}

// a thread's share of one panel of 128 rows x 32 samples, as loaded: four rows of four samples
struct Staged {
  float xv[kTile / 32][kOwn], mv[kTile / 32][kOwn];
  unsigned fv[kTile / 32][kOwn];
};

// the loads of a panel from t0 on.  A row that is not there and a sample past T are never loaded
template <bool kCount>
__device__ __forceinline__ void load_panel(Staged& st, const int* __restrict__ s_row, const float* __restrict__ x, size_t ld_x,
                                           const float* __restrict__ model, size_t ld_m, const unsigned char* __restrict__ flags, size_t ld_f,
                                           long long t0, int T, int wide, int tid) {
  const long long q = t0 + kOwn * (tid & 7);
#pragma unroll
  for (int p = 0; p < kTile / 32; ++p) {
    const int d = s_row[32 * p + (tid >> 3)];
    if (d >= 0 && q < T) {
      if (flags) load4(flags + (size_t)d * ld_f, q, T, whole(q, T, wide, kWideF), st.fv[p]);
      if (!kCount) {
        load4(x + (size_t)d * ld_x, q, T, whole(q, T, wide, kWideX), st.xv[p]);
        if (model) load4(model + (size_t)d * ld_m, q, T, whole(q, T, wide, kWideM), st.mv[p]);
      }
    }
  }
}

// the loaded panel as z into s[row][parity][16]: model, centre and flag select, once per element
template <bool kCount>
__device__ __forceinline__ void store_panel(float* __restrict__ s, const Staged& st, const int* __restrict__ s_row,
                                            const double* __restrict__ s_center, bool has_model, bool has_flags, long long t0, int T, int wide,
                                            int tid) {
  const int kq = kOwn * (tid & 7);
  const long long q = t0 + kq;
  const bool packed = whole(q, T, wide, kWideF);
#pragma unroll
  for (int p = 0; p < kTile / 32; ++p) {
    const int rl = 32 * p + (tid >> 3);
    const bool there = s_row[rl] >= 0;
    const double c = kCount ? 0.0 : s_center[rl];
    float zs[kOwn];
#pragma unroll
    for (int k = 0; k < kOwn; ++k) {
      bool keep = there && q + k < T;
      if (keep && has_flags) keep = (packed ? (st.fv[p][0] >> (8 * k)) & 255u : st.fv[p][k]) == 0;
      float z = 0.0f;
      if (keep) {  // selected, never multiplied
        if (kCount) {
          z = 1.0f;
        } else {
          const double term = has_model ? (double)st.xv[p][k] - (double)st.mv[p][k] : (double)st.xv[p][k];
          z = (float)(term - c);
        }
      }
      zs[k] = z;
    }
    *reinterpret_cast<float2*>(s + rl * kRowStride + kq / 2) = make_float2(zs[0], zs[2]);                // even samples
    *reinterpret_cast<float2*>(s + rl * kRowStride + kPanel / 2 + kq / 2) = make_float2(zs[1], zs[3]);  // odd samples
  }
}

template <bool kCount>
__global__ __launch_bounds__(kThreads) void gram_kernel(const float* __restrict__ x, size_t ld_x, const float* __restrict__ model, size_t ld_m,
                                                        const unsigned char* __restrict__ flags, size_t ld_f, int D, int T,
                                                        const int* __restrict__ rows, int R, const double* __restrict__ center,
                                                        std::conditional_t<kCount, unsigned, double>* __restrict__ out, int wide) {
  using Sum = std::conditional_t<kCount, unsigned, double>;
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;  // the whole workgroup: the mirror block writes this one
  __shared__ __attribute__((aligned(16))) float s_z[2][kTile * kRowStride];
  __shared__ int s_row[2][kTile];
  __shared__ double s_center[2][kTile];
  const int tid = threadIdx.x;
  const bool diag = bi == bj;
  {
    const int side = tid >> 7, rl = tid & (kTile - 1);
    const int i = (side ? bj : bi) * kTile + rl;
    int d = kPast;
    if (i < R) {
      d = rows ? rows[i] : i;
      if ((unsigned)d >= (unsigned)D) d = kNoRow;
    }
    s_row[side][rl] = d;
    s_center[side][rl] = d >= 0 && center ? center[d] : 0.0;
  }
  __syncthreads();
  const float* const s_a = s_z[0];
  const float* const s_b = diag ? s_z[0] : s_z[1];
  const int lane = tid & 63, wave = tid >> 6;
  const int ra = 64 * (wave >> 1) + (lane & 31), rb = 64 * (wave & 1) + (lane & 31), kh = lane >> 5;

  f32x16 acc[2][2];
  Sum sum[2][2][16];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc[a][b][r] = 0.0f;
        sum[a][b][r] = (Sum)0;
      }
    }
  }
  constexpr int kPanelsPerBlock = MRX_GRAM_BLOCK / kPanel;
  const int n_panels = (int)(((long long)T + kPanel - 1) / kPanel);
  Staged st_a, st_b;  // the next panel, in flight while this one is multiplied
  load_panel<kCount>(st_a, s_row[0], x, ld_x, model, ld_m, flags, ld_f, 0, T, wide, tid);
  if (!diag) load_panel<kCount>(st_b, s_row[1], x, ld_x, model, ld_m, flags, ld_f, 0, T, wide, tid);
  for (int p = 0; p < n_panels; ++p) {
    store_panel<kCount>(s_z[0], st_a, s_row[0], s_center[0], model != nullptr, flags != nullptr, (long long)p * kPanel, T, wide, tid);
    if (!diag) store_panel<kCount>(s_z[1], st_b, s_row[1], s_center[1], model != nullptr, flags != nullptr, (long long)p * kPanel, T, wide, tid);
    __syncthreads();
    if (p + 1 < n_panels) {
      const long long t1 = (long long)(p + 1) * kPanel;
      load_panel<kCount>(st_a, s_row[0], x, ld_x, model, ld_m, flags, ld_f, t1, T, wide, tid);
      if (!diag) load_panel<kCount>(st_b, s_row[1], x, ld_x, model, ld_m, flags, ld_f, t1, T, wide, tid);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // eight k-steps at a time: 32 operand registers
      float a0[8], a1[8], b0[8], b1[8];
      read8(s_a + ra * kRowStride + 16 * kh + 8 * h, a0);
      read8(s_a + (ra + 32) * kRowStride + 16 * kh + 8 * h, a1);
      read8(s_b + rb * kRowStride + 16 * kh + 8 * h, b0);
      read8(s_b + (rb + 32) * kRowStride + 16 * kh + 8 * h, b1);
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {  // k-step 8 h + ks: the samples 2 (8 h + ks) and + 1, in this order
        acc[0][0] = mfma_32x32x2(a0[ks], b0[ks], acc[0][0]);
        acc[0][1] = mfma_32x32x2(a0[ks], b1[ks], acc[0][1]);
        acc[1][0] = mfma_32x32x2(a1[ks], b0[ks], acc[1][0]);
        acc[1][1] = mfma_32x32x2(a1[ks], b1[ks], acc[1][1]);
      }
    }
    __syncthreads();  // the panels are read: the next round may overwrite them
    if ((p + 1) % kPanelsPerBlock == 0 || p + 1 == n_panels) {
#pragma unroll
      for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            sum[a][b][r] = sum[a][b][r] + (Sum)acc[a][b][r];
            acc[a][b][r] = 0.0f;
          }
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int jl = 64 * (wave & 1) + 32 * b + (lane & 31);
      const int dj = s_row[1][jl];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int il = 64 * (wave >> 1) + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * kh;
        const int di = s_row[0][il];
        if (di == kPast || dj == kPast) continue;
        const Sum v = di >= 0 && dj >= 0 ? sum[a][b][r] : (Sum)0;
        const size_t i = (size_t)bi * kTile + il, j = (size_t)bj * kTile + jl;
        out[i * (size_t)R + j] = v;
        if (!diag) out[j * (size_t)R + i] = v;
      }
    }
  }
}

// the counts without flags: T where both rows are in range, 0 otherwise
__global__ __launch_bounds__(kThreads) void gram_count_fill_kernel(int D, int T, const int* __restrict__ rows, int R, unsigned* __restrict__ n,
                                                                   long long total) {
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
    const int i = (int)(e / R), j = (int)(e - (long long)i * R);
    const int di = rows ? rows[i] : i, dj = rows ? rows[j] : j;
    n[e] = (unsigned)di < (unsigned)D && (unsigned)dj < (unsigned)D ? (unsigned)T : 0u;
  }
}

}  // namespace

extern "C" {

int mrx_tod_gram(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m, const uint8_t* d_flags, size_t ld_f, int D,
                 int T, const int32_t* d_rows, int R, const double* d_center, double* d_G, uint32_t* d_n) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, d_x && d_G, "null pointer");
  MRX_REQUIRE(ctx, D >= 1 && T >= 1 && R >= 1, "need D >= 1 rows of T >= 1 samples and R >= 1 rows in the list");
  MRX_REQUIRE(ctx, ld_x >= (size_t)T && (!d_model || ld_m >= (size_t)T) && (!d_flags || ld_f >= (size_t)T), "ld_x, ld_m or ld_f smaller than T");
  const int wide = (mrx_aligned(d_x, ld_x * 4, 16) ? kWideX : 0) | (d_model && mrx_aligned(d_model, ld_m * 4, 16) ? kWideM : 0) |
                   (d_flags && mrx_aligned(d_flags, ld_f, 4) ? kWideF : 0);
  const unsigned nb = (unsigned)(((long long)R + kTile - 1) / kTile);
  hipLaunchKernelGGL(gram_kernel<false>, dim3(nb, nb), dim3(kThreads), 0, ctx->stream, d_x, ld_x, d_model, ld_m, d_flags, ld_f, D, T, d_rows, R,
                     d_center, d_G, wide);
  MRX_CHECK_LAUNCH(ctx);
  if (d_n && d_flags) {
    hipLaunchKernelGGL(gram_kernel<true>, dim3(nb, nb), dim3(kThreads), 0, ctx->stream, d_x, ld_x, (const float*)nullptr, (size_t)0, d_flags, ld_f,
                       D, T, d_rows, R, (const double*)nullptr, d_n, wide);
    MRX_CHECK_LAUNCH(ctx);
  } else if (d_n) {
    const long long total = (long long)R * R;
    hipLaunchKernelGGL(gram_count_fill_kernel, dim3(mrx_resident_blocks(ctx, (total + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream, D,
                       T, d_rows, R, d_n, total);
    MRX_CHECK_LAUNCH(ctx);
  }
  return MRX_OK;
}

}  // extern "C"
