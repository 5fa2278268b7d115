// TOD pre-processing for the mappers (tod/processing.py:91-204): the streaming passes of
// process_tod on a [D][T] float32 TOD in place --
//   remove_slope   D -= linspace(D[:, 0], D[:, -1], T)                (processing.py:99-105)
//   window         D *= w[t]                                          (processing.py:139-146)
//   filter         remove_slope, then scipy.signal.sosfilt of the Bessel low / high pass
//                  sections along time                                (processing.py:148-176,
//                                                                      utils/signal/filters.py:46-69)
// The GEMM-shaped operations (remove_spline, remove_modes) are plain library products and
// stay with the host side (maria_amd/tod_processing.py, torch.matmul / eigh).
//
// sosfilt is a recursion along time; here it is made time-parallel in the standard way for
// a linear recurrence s[n+1] = A s[n] + B x[n]: (1) every chunk of 256 samples is run from a
// zero state and leaves its end state; (2) one thread per detector chains the chunks,
// s_in(c+1) = A^256 s_in(c) + s_zero(c) (A^256 from the host, float64); (3) every chunk is
// run again from its true initial state and writes the output.  Arithmetic is float64 in the
// transposed direct form II of scipy's _sosfilt; the result differs from the serial loop by
// float64 rounding only.  Lanes are consecutive chunks of one detector: each lane streams
// its own 1 KiB with 16-byte loads.
#include <vector>

#include "mrx_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 256;      // samples per chunk
constexpr int kMaxSections = 8;  // biquads in the cascade (low + high pass up to order 3)

typedef float vfloat4 __attribute__((ext_vector_type(4)));

struct SosArgs {
  double b0[kMaxSections], b1[kMaxSections], b2[kMaxSections], a1[kMaxSections], a2[kMaxSections];
  int n_sections;
  const float* in;
  size_t ld_in;
  float* out;
  size_t ld_out;
  int D, T, n_chunks;
  int remove_slope;   // subtract the line through the first and last sample first
  const double* anchors;  // [D][2] (first, last) of the input rows
  double* states;     // [D][n_chunks][2 * n_sections]
  const double* M;    // [2S][2S] = A^kChunk, row-major (state' = M state)
  const double* resp;  // the transpose with remove_slope: H a at [0, T), H b at [round4(T), round4(T) + T) (get_slope_resp)
};

// np.linspace(a, b, T)[t] = a + t (b - a)/(T - 1), with the last point set to b exactly
__device__ __forceinline__ double line_at(double first, double last, double step, int t, int T) {
  return t == T - 1 ? last : first + step * (double)t;
}

// (first, last) of every row, read before anything is overwritten: anchors[2 d], [2 d + 1]
__global__ __launch_bounds__(kBlock) void anchors_kernel(const float* __restrict__ data, size_t ld, int D, int T,
                                                       double* __restrict__ anchors) {
  const int d = blockIdx.x * kBlock + threadIdx.x;
  if (d >= D) return;
  anchors[2 * d] = (double)data[(size_t)d * ld];
  anchors[2 * d + 1] = (double)data[(size_t)d * ld + T - 1];
}

// One workgroup = 256 consecutive chunks of one detector (65536 samples), one thread per chunk.
// A thread walks its chunk sequentially, but the workgroup moves the data 32 samples of every
// chunk at a time through LDS: global loads and stores are whole 128-byte lines (8 lanes x 16
// bytes per chunk), and a thread reads its own LDS row (pitch 33 words: conflict-free).
constexpr int kSub = 32;            // samples of every chunk per stage
constexpr int kPitch = kSub + 1;

//
// kRev is the transpose H^T = J H J (J: time reversal): the same chunks, aligned from sample 0, each walked from its
// last sample to its first.  With remove_slope the write pass then also takes, per row, the two sums of S^T,
// <a, u> and <b, u> of u = H^T in with a_t = 1 - t/(T-1), b_t = t/(T-1), as <H a, in> and <H b, in> of the samples it
// loads (one pair per workgroup, a tree in LDS, left in the state slot of the workgroup's first chunk), and keeps u_0 and
// u_{T-1} in float64 for slope_transpose_kernel.  Summing the outputs themselves would add up the chained states'
// float64 rounding, which the chunk matrix (entries up to 200) lifts to 1e-9 of the input and a pole next to 1 keeps
// at one sign over a whole row; H a and H b come from a serial loop (get_slope_resp) and the input is exact.
template <int S, bool kWrite, bool kRev>
__global__ __launch_bounds__(kBlock) void sos_chunk_kernel(SosArgs g) {
  __shared__ float stage[kBlock * kPitch];
  const int c0 = blockIdx.x * kBlock;              // first chunk of the workgroup
  const int c = c0 + threadIdx.x;                  // this thread's chunk
  const int d = blockIdx.y;
  const float* row = g.in + (size_t)d * g.ld_in;
  float* orow = g.out + (size_t)d * g.ld_out;
  double first = 0.0, last = 0.0;
  if constexpr (!kRev) {
    first = g.anchors[2 * d];
    last = g.anchors[2 * d + 1];
  }
  const double step = g.T > 1 ? (last - first) / (double)(g.T - 1) : 0.0;
  const bool live = c < g.n_chunks;
  double z0[S], z1[S];
  double* st = g.states + ((size_t)d * g.n_chunks + (live ? c : 0)) * (2 * S);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    z0[s] = (kWrite && live) ? st[2 * s] : 0.0;
    z1[s] = (kWrite && live) ? st[2 * s + 1] : 0.0;
  }
  // cooperative tile moves: lane group of 8 handles one chunk's 32 samples (4 per lane)
  const int part = threadIdx.x & 7, rowgrp = threadIdx.x >> 3;  // 32 chunks per pass of the block
  const bool vec_in = (g.ld_in % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.in) & 15u) == 0);
  const bool vec_out = (g.ld_out % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.out) & 15u) == 0);
  [[maybe_unused]] double sum_a = 0.0, sum_b = 0.0;  // kRev: this thread's share of the two row sums
  [[maybe_unused]] const double* resp_b = g.resp + (size_t)(g.T + 3) / 4 * 4;
  for (int jj = 0; jj < kChunk / kSub; ++jj) {
    const int j = kRev ? kChunk / kSub - 1 - jj : jj;
    // ---- load stage j of all 256 chunks
    for (int cc = rowgrp; cc < kBlock; cc += kBlock / 8) {
      const long long t = (long long)(c0 + cc) * kChunk + j * kSub + part * 4;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (t + 4 <= g.T && vec_in) {
        const vfloat4 q = *reinterpret_cast<const vfloat4*>(row + t);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (t + k < g.T) v[k] = row[t + k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) stage[cc * kPitch + part * 4 + k] = v[k];
      if constexpr (kRev && kWrite) {
        if (g.remove_slope) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (t + k < g.T) {
              sum_a = fma(g.resp[t + k], (double)v[k], sum_a);
              sum_b = fma(resp_b[t + k], (double)v[k], sum_b);
            }
        }
      }
    }
    __syncthreads();
    // ---- every thread: 32 steps of its own chunk
    const int tb = c * kChunk + j * kSub;
    if (live) {
#pragma unroll 4
      for (int ii = 0; ii < kSub; ++ii) {
        const int i = kRev ? kSub - 1 - ii : ii;
        const int t = tb + i;
        if (t >= g.T) {
          if constexpr (kRev) continue; else break;
        }
        double x = (double)stage[threadIdx.x * kPitch + i];
        if constexpr (!kRev)
          if (g.remove_slope) x -= line_at(first, last, step, t, g.T);  // utils/signal/__init__.py:151-152
#pragma unroll
        for (int s = 0; s < S; ++s) {
          // scipy/signal/_sosfilt.pyx: transposed direct form II
          const double y = g.b0[s] * x + z0[s];
          z0[s] = g.b1[s] * x - g.a1[s] * y + z1[s];
          z1[s] = g.b2[s] * x - g.a2[s] * y;
          x = y;
        }
        if (kWrite) stage[threadIdx.x * kPitch + i] = (float)x;
        if constexpr (kRev && kWrite) {
          if (g.remove_slope) {
            double* ends = const_cast<double*>(g.anchors) + 2 * d;
            if (t == 0) ends[0] = x;
            if (t == g.T - 1) ends[1] = x;
          }
        }
      }
    }
    __syncthreads();
    if (kWrite) {
      // ---- store stage j
      for (int cc = rowgrp; cc < kBlock; cc += kBlock / 8) {
        const long long t = (long long)(c0 + cc) * kChunk + j * kSub + part * 4;
        if (t >= g.T) continue;
        const float* v = stage + cc * kPitch + part * 4;
        if (t + 4 <= g.T && vec_out) {
          *reinterpret_cast<vfloat4*>(orow + t) = vfloat4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (t + k < g.T) orow[t + k] = v[k];
        }
      }
      __syncthreads();
    }
  }
  if (!kWrite && live) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      st[2 * s] = z0[s];
      st[2 * s + 1] = z1[s];
    }
  }
  if constexpr (kRev && kWrite) {
    if (g.remove_slope) {  // every thread read its state at the top: the first chunk's slot is free
      __shared__ double red[2 * kBlock];
      red[threadIdx.x] = sum_a;
      red[kBlock + threadIdx.x] = sum_b;
      __syncthreads();
      for (int n = kBlock / 2; n > 0; n >>= 1) {
        if ((int)threadIdx.x < n) {
          red[threadIdx.x] += red[threadIdx.x + n];
          red[kBlock + threadIdx.x] += red[kBlock + threadIdx.x + n];
        }
        __syncthreads();
      }
      if (threadIdx.x == 0) {
        double* slot = g.states + ((size_t)d * g.n_chunks + c0) * (2 * S);
        slot[0] = red[0];
        slot[1] = red[kBlock];
      }
    }
  }
}

// S^T after the reversed write pass: out[0] = u_0 - sum_a, out[T-1] = u_{T-1} - sum_b, the sums over the row's
// workgroups in their order, the end samples from their float64 values (one rounding to float32)
__global__ __launch_bounds__(kBlock) void slope_transpose_kernel(const double* __restrict__ ends,
                                                               const double* __restrict__ states, int n_chunks,
                                                               int state_doubles, float* __restrict__ out, size_t ld,
                                                               int D, int T) {
  const int d = blockIdx.x * kBlock + threadIdx.x;
  if (d >= D) return;
  double sum_a = 0.0, sum_b = 0.0;
  for (int c0 = 0; c0 < n_chunks; c0 += kBlock) {
    const double* slot = states + ((size_t)d * n_chunks + c0) * state_doubles;
    sum_a += slot[0];
    sum_b += slot[1];
  }
  float* row = out + (size_t)d * ld;
  if (T == 1) {
    row[0] = 0.f;  // a = 0, b = 1: S = 0 on a single sample, and so is S^T, exactly
  } else {
    row[0] = (float)(ends[2 * d] - sum_a);
    row[T - 1] = (float)(ends[2 * d + 1] - sum_b);
  }
}

// chains the chunks of one detector: states[c] <- initial state of chunk c
// (kRev: from the last chunk down to the first; the short last chunk starts from the zero state, so A^kChunk serves)
template <int S, bool kRev>
__global__ __launch_bounds__(kBlock) void sos_scan_kernel(SosArgs g) {
  const int d = blockIdx.x * kBlock + threadIdx.x;
  if (d >= g.D) return;
  constexpr int N = 2 * S;
  double M[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) M[i][j] = g.M[i * N + j];
  double s[N];
#pragma unroll
  for (int i = 0; i < N; ++i) s[i] = 0.0;
  double* st = g.states + (size_t)d * g.n_chunks * N;
  for (int k = 0; k < g.n_chunks; ++k) {
    const int c = kRev ? g.n_chunks - 1 - k : k;
    double zs[N], nxt[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      zs[i] = st[(size_t)c * N + i];
      st[(size_t)c * N + i] = s[i];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double acc = zs[i];
#pragma unroll
      for (int j = 0; j < N; ++j) acc = fma(M[i][j], s[j], acc);
      nxt[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = nxt[i];
  }
}

// np.linspace(first, last, T)[t] of float32 end points, as numpy >= 2 evaluates it: in float32,
// step = (last - first) / (T - 1), then t * step + first, each operation rounded (no fma), the
// last point set to `last`.  The float32 division is done in float64 and rounded once: a float64
// quotient of two floats rounds to the correctly rounded float32 quotient.
__device__ __forceinline__ float line_at_f32(float first, float last, int t, int T) {
#pragma clang fp contract(off)
  if (t == T - 1) return last;
  const float step = T > 1 ? (float)((double)(last - first) / (double)(T - 1)) : 0.f;
  return (float)t * step + first;
}

// remove_slope and / or window in place: v = float32(x - line); v = float32(v * w[t])
__global__ __launch_bounds__(kBlock) void detrend_window_kernel(float* __restrict__ data, size_t ld, int D, int T,
                                                              int remove_slope, const double* __restrict__ window,
                                                              const double* __restrict__ anchors) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= T) return;
  const int d0 = blockIdx.y * 16;
  const double wt = window ? window[t] : 1.0;
  for (int d = d0; d < min(d0 + 16, D); ++d) {
    float* row = data + (size_t)d * ld;
    float v = row[t];
    if (remove_slope) v -= line_at_f32((float)anchors[2 * d], (float)anchors[2 * d + 1], t, T);
    if (window) v = (float)((double)v * wt);
    row[t] = v;
  }
}

template <int S, bool kRev>
int launch_sos(mrx_ctx* ctx, const SosArgs& g) {
  const dim3 grid(mrx_ceil_div(g.n_chunks, kBlock), g.D);
  const dim3 rows(mrx_ceil_div(g.D, kBlock));
  hipLaunchKernelGGL((sos_chunk_kernel<S, false, kRev>), grid, dim3(kBlock), 0, ctx->stream, g);
  hipLaunchKernelGGL((sos_scan_kernel<S, kRev>), rows, dim3(kBlock), 0, ctx->stream, g);
  hipLaunchKernelGGL((sos_chunk_kernel<S, true, kRev>), grid, dim3(kBlock), 0, ctx->stream, g);
  if (kRev && g.remove_slope)
    hipLaunchKernelGGL(slope_transpose_kernel, rows, dim3(kBlock), 0, ctx->stream, g.anchors, g.states, g.n_chunks, 2 * S,
                       g.out, g.ld_out, g.D, g.T);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

template <bool kRev>
int launch_sos_sections(mrx_ctx* ctx, const SosArgs& g) {
  switch (g.n_sections) {
    case 1: return launch_sos<1, kRev>(ctx, g);
    case 2: return launch_sos<2, kRev>(ctx, g);
    case 3: return launch_sos<3, kRev>(ctx, g);
    case 4: return launch_sos<4, kRev>(ctx, g);
    case 5: return launch_sos<5, kRev>(ctx, g);
    case 6: return launch_sos<6, kRev>(ctx, g);
    case 7: return launch_sos<7, kRev>(ctx, g);
    default: return launch_sos<8, kRev>(ctx, g);
  }
}

// H a and H b for S^T after H^T: <a, H^T y> = <H a, y>, so the two row sums of the transposed slope removal are dot
// products of the INPUT row with two vectors that depend on the cascade and T alone.  a_t = 1 - b_t, b_t = t/(T-1) (the
// last point 1 exactly, as line_at has it); H in the arithmetic of the kernels, but serially from sample 0, on the host in
// float64; cached per (cascade, T) like the screen's taps, so that a repeated call neither computes nor copies.
int get_slope_resp(mrx_ctx* ctx, SosArgs& g) {
  double coef[40] = {0.0};
  for (int s = 0; s < g.n_sections; ++s) {
    coef[5 * s + 0] = g.b0[s]; coef[5 * s + 1] = g.b1[s]; coef[5 * s + 2] = g.b2[s];
    coef[5 * s + 3] = g.a1[s]; coef[5 * s + 4] = g.a2[s];
  }
  for (auto& slot : ctx->slope_resp)
    if (slot.d_resp && slot.T == g.T && slot.n_sections == g.n_sections && !std::memcmp(slot.coef, coef, sizeof(coef))) {
      g.resp = slot.d_resp;
      return MRX_OK;
    }
  const size_t pitch = ((size_t)g.T + 3) / 4 * 4;
  std::vector<double> h(2 * pitch, 0.0);
  double za[kMaxSections][2] = {{0.0}}, zb[kMaxSections][2] = {{0.0}};
  for (int t = 0; t < g.T; ++t) {
    const double wb = t == g.T - 1 ? 1.0 : (double)t / (double)(g.T - 1);
    double xa = 1.0 - wb, xb = wb;
    for (int s = 0; s < g.n_sections; ++s) {
      const double ya = g.b0[s] * xa + za[s][0], yb = g.b0[s] * xb + zb[s][0];
      za[s][0] = g.b1[s] * xa - g.a1[s] * ya + za[s][1];
      zb[s][0] = g.b1[s] * xb - g.a1[s] * yb + zb[s][1];
      za[s][1] = g.b2[s] * xa - g.a2[s] * ya;
      zb[s][1] = g.b2[s] * xb - g.a2[s] * yb;
      xa = ya;
      xb = yb;
    }
    h[(size_t)t] = xa;
    h[pitch + (size_t)t] = xb;
  }
  auto& slot = ctx->slope_resp[ctx->slope_resp_next];
  ctx->slope_resp_next = (ctx->slope_resp_next + 1) % mrx_ctx::kSlopeRespSlots;
  if (slot.d_resp) {  // a kernel in flight may still read the evicted vectors
    MRX_HIP(ctx, hipDeviceSynchronize());
    (void)hipFree(slot.d_resp);
    slot.d_resp = nullptr;
  }
  MRX_HIP(ctx, hipMalloc(&slot.d_resp, h.size() * sizeof(double)));
  MRX_HIP(ctx, hipMemcpyAsync(slot.d_resp, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  MRX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // h goes out of scope
  std::memcpy(slot.coef, coef, sizeof(coef));
  slot.n_sections = g.n_sections;
  slot.T = g.T;
  g.resp = slot.d_resp;
  return MRX_OK;
}

// the checks and the arguments mrx_sosfilt and mrx_sosfilt_transpose share; MRX_OK with g.D = 0 for an empty call
int sos_args(mrx_ctx* ctx, const double* sos, int n_sections, const double* d_chunk_matrix, const float* d_in, size_t ld_in,
             int D, int T, int remove_slope, float* d_out, size_t ld_out, double* d_work, SosArgs& g) {
  MRX_REQUIRE(ctx, D >= 0 && T >= 0, "negative size");
  if (D == 0 || T == 0) return MRX_OK;
  MRX_REQUIRE(ctx, sos && d_chunk_matrix && d_in && d_out && d_work, "null pointer");
  MRX_REQUIRE(ctx, n_sections >= 1 && n_sections <= kMaxSections, "1 <= n_sections <= 8");
  MRX_REQUIRE(ctx, ld_in >= (size_t)T && ld_out >= (size_t)T, "leading dimension smaller than T");
  MRX_REQUIRE(ctx, D <= 65535, "D too large for one launch");
  for (int s = 0; s < n_sections; ++s) {
    const double a0 = sos[6 * s + 3];
    MRX_REQUIRE(ctx, a0 != 0.0, "a0 of a section is zero");
    g.b0[s] = sos[6 * s + 0] / a0;  // scipy normalises by a0 (1 for the filters built here)
    g.b1[s] = sos[6 * s + 1] / a0;
    g.b2[s] = sos[6 * s + 2] / a0;
    g.a1[s] = sos[6 * s + 4] / a0;
    g.a2[s] = sos[6 * s + 5] / a0;
  }
  g.n_sections = n_sections;
  g.in = d_in;
  g.ld_in = ld_in;
  g.out = d_out;
  g.ld_out = ld_out;
  g.D = D;
  g.T = T;
  g.n_chunks = mrx_ceil_div(T, kChunk);
  g.remove_slope = remove_slope;
  g.anchors = d_work;             // [D][2]
  g.states = d_work + 2 * (size_t)D;
  g.M = d_chunk_matrix;
  return MRX_OK;
}

// x = S^T diag(w) y in place, one workgroup per row: u = w y in float64, written back as float32, the two sums of S^T
// taken of it on the way (a tree in LDS), then the end samples set from their float64 values (one rounding)
__global__ __launch_bounds__(kBlock) void detrend_window_transpose_kernel(float* __restrict__ data, size_t ld, int T,
                                                                        int remove_slope,
                                                                        const double* __restrict__ window) {
  __shared__ double red[2 * kBlock];
  __shared__ double ends[2];
  float* row = data + (size_t)blockIdx.x * ld;
  double sum_a = 0.0, sum_b = 0.0;
  for (int t = threadIdx.x; t < T; t += kBlock) {
    double u = (double)row[t];
    if (window) {
      u *= window[t];
      row[t] = (float)u;
    }
    if (remove_slope) {
      const double wb = t == T - 1 ? 1.0 : (double)t / (double)(T - 1);
      sum_a += (1.0 - wb) * u;
      sum_b += wb * u;
      if (t == 0) ends[0] = u;
      if (t == T - 1) ends[1] = u;
    }
  }
  if (!remove_slope) return;
  red[threadIdx.x] = sum_a;
  red[kBlock + threadIdx.x] = sum_b;
  __syncthreads();
  for (int n = kBlock / 2; n > 0; n >>= 1) {
    if ((int)threadIdx.x < n) {
      red[threadIdx.x] += red[threadIdx.x + n];
      red[kBlock + threadIdx.x] += red[kBlock + threadIdx.x + n];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (T == 1) {
      row[0] = (float)(ends[0] - red[0] - red[kBlock]);
    } else {
      row[0] = (float)(ends[0] - red[0]);
      row[T - 1] = (float)(ends[1] - red[kBlock]);
    }
  }
}

}  // namespace

extern "C" {

int mrx_tod_detrend_window(mrx_ctx* ctx, float* d_data, size_t ld, int D, int T, int remove_slope,
                           const double* d_window, double* d_work) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, D >= 0 && T >= 0, "negative size");
  if (D == 0 || T == 0 || (!remove_slope && !d_window)) return MRX_OK;
  MRX_REQUIRE(ctx, d_data && ld >= (size_t)T, "null pointer or ld smaller than T");
  MRX_REQUIRE(ctx, !remove_slope || d_work, "remove_slope needs 2 * D doubles of scratch");
  if (remove_slope)  // the anchors are themselves rewritten: read them first
    hipLaunchKernelGGL(anchors_kernel, dim3(mrx_ceil_div(D, kBlock)), dim3(kBlock), 0, ctx->stream, d_data, ld, D, T,
                       d_work);
  const dim3 grid(mrx_ceil_div(T, kBlock), mrx_ceil_div(D, 16));
  MRX_REQUIRE(ctx, grid.y <= 65535u, "D too large for one launch");
  hipLaunchKernelGGL(detrend_window_kernel, grid, dim3(kBlock), 0, ctx->stream, d_data, ld, D, T, remove_slope,
                     d_window, d_work);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_sosfilt_work_doubles(int D, int T, int n_sections, size_t* doubles) {
  if (D < 0 || T < 0 || n_sections < 1 || n_sections > kMaxSections || !doubles) return MRX_ERR_INVALID;
  *doubles = 2 * (size_t)D + (size_t)D * (size_t)mrx_ceil_div(T > 0 ? T : 1, kChunk) * (size_t)(2 * n_sections) + 16;
  return MRX_OK;
}

int mrx_sosfilt(mrx_ctx* ctx, const double* sos, int n_sections, const double* d_chunk_matrix,
                const float* d_in, size_t ld_in, int D, int T, int remove_slope, float* d_out,
                size_t ld_out, double* d_work) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  SosArgs g{};
  const int rc = sos_args(ctx, sos, n_sections, d_chunk_matrix, d_in, ld_in, D, T, remove_slope, d_out, ld_out, d_work, g);
  if (rc != MRX_OK || g.D == 0) return rc;
  hipLaunchKernelGGL(anchors_kernel, dim3(mrx_ceil_div(D, kBlock)), dim3(kBlock), 0, ctx->stream, d_in, ld_in, D, T,
                     d_work);
  return launch_sos_sections<false>(ctx, g);
}

int mrx_sosfilt_transpose(mrx_ctx* ctx, const double* sos, int n_sections, const double* d_chunk_matrix,
                          const float* d_in, size_t ld_in, int D, int T, int remove_slope, float* d_out,
                          size_t ld_out, double* d_work) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  SosArgs g{};
  const int rc = sos_args(ctx, sos, n_sections, d_chunk_matrix, d_in, ld_in, D, T, remove_slope, d_out, ld_out, d_work, g);
  if (rc != MRX_OK || g.D == 0) return rc;
  if (remove_slope) {
    const int rr = get_slope_resp(ctx, g);
    if (rr != MRX_OK) return rr;
  }
  return launch_sos_sections<true>(ctx, g);
}

int mrx_tod_detrend_window_transpose(mrx_ctx* ctx, float* d_data, size_t ld, int D, int T, int remove_slope,
                                     const double* d_window) {
  MRX_ENTER(ctx);
  if (!ctx) return MRX_ERR_INVALID;
  MRX_REQUIRE(ctx, D >= 0 && T >= 0, "negative size");
  if (D == 0 || T == 0 || (!remove_slope && !d_window)) return MRX_OK;
  MRX_REQUIRE(ctx, d_data && ld >= (size_t)T, "null pointer or ld smaller than T");
  hipLaunchKernelGGL(detrend_window_transpose_kernel, dim3(D), dim3(kBlock), 0, ctx->stream, d_data, ld, T, remove_slope,
                     d_window);
  MRX_CHECK_LAUNCH(ctx);
  return MRX_OK;
}

int mrx_sosfilt_chunk(void) { return kChunk; }

}  // extern "C"
