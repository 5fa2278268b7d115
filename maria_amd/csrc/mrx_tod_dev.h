// Device code the kernels of [D, T] TODs share: a thread's own samples, the segment of a sample, the
// normal equations of a wave.  Each contract is stated here once; a file that calls these says only what is its own.
//
// Floating-point contraction.  rhs_add multiplies and adds, and a header function is compiled with the flags
// of the file that includes it: every file that calls it is built with -ffp-contract=off (csrc/Makefile), so that a
// product and its addition are two roundings in all of them.  A file built with contraction on (mrx_hwp.hip) takes only
// the loads and stores, which do no arithmetic.
#pragma once

#include <hip/hip_runtime.h>

namespace mrx_tod {

constexpr int kWave = 64;
// The streaming tile: a workgroup of kThreads threads takes kTileSamples consecutive samples of a row, thread o the kOwn
// samples kOwn o .. kOwn o + kOwn - 1 of them, whatever the alignment.  A file with another tile keeps its own constants.
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kOwn = 4;
constexpr int kTileSamples = kThreads * kOwn;

// A thread's OWN (4 or 2) consecutive samples q .. q + OWN - 1 of a row of T: ONE access of 4 OWN bytes where `wide` (the
// row's pointer and pitch are multiples of 4 OWN bytes and q of OWN: mrx_aligned) and the samples all lie inside the row,
// OWN accesses otherwise.  Nothing is read or written past T; a sample past T loads as 0.  q is an int or, where a row's
// last tile may pass 2^31, a long long.
template <int OWN, class Q>
__device__ __forceinline__ void load_own(const float* row, Q q, int T, bool wide, float (&v)[OWN]) {
  static_assert(OWN == 4 || OWN == 2, "one 16-byte or one 8-byte access");
  if (wide && q + OWN <= (Q)T) {
    if constexpr (OWN == 4) {
      const float4 w = *reinterpret_cast<const float4*>(row + q);
      v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
    } else {
      const float2 w = *reinterpret_cast<const float2*>(row + q);
      v[0] = w.x, v[1] = w.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < OWN; ++k) v[k] = q + k < (Q)T ? row[q + k] : 0.0f;
  }
}

template <int OWN, class Q>
__device__ __forceinline__ void store_own(float* row, Q q, int T, bool wide, const float (&v)[OWN]) {
  static_assert(OWN == 4 || OWN == 2, "one 16-byte or one 8-byte access");
  if (wide && q + OWN <= (Q)T) {
    if constexpr (OWN == 4)
      *reinterpret_cast<float4*>(row + q) = make_float4(v[0], v[1], v[2], v[3]);
    else
      *reinterpret_cast<float2*>(row + q) = make_float2(v[0], v[1]);
  } else {
#pragma unroll
    for (int k = 0; k < OWN; ++k)
      if (q + k < (Q)T) row[q + k] = v[k];
  }
}

// Their flags: one word of OWN bytes where `wide` (pointer and pitch multiples of OWN), bytes otherwise.  A sample past T
// is FLAGGED (1), so that it enters no sum.
template <int OWN, class Q>
__device__ __forceinline__ void load_own(const unsigned char* row, Q q, int T, bool wide, unsigned char (&f)[OWN]) {
  static_assert(OWN == 4 || OWN == 2, "one 4-byte or one 2-byte access");
  if (wide && q + OWN <= (Q)T) {
    unsigned w;
    if constexpr (OWN == 4)
      w = *reinterpret_cast<const unsigned*>(row + q);
    else
      w = *reinterpret_cast<const unsigned short*>(row + q);
#pragma unroll
    for (int k = 0; k < OWN; ++k) f[k] = (unsigned char)((w >> (8 * k)) & 255u);
  } else {
#pragma unroll
    for (int k = 0; k < OWN; ++k) f[k] = q + k < (Q)T ? row[q + k] : (unsigned char)1;
  }
}

// The flags of a call that may have none (row == nullptr): then 0 inside T and 1 past it.  The null test is here and
// not in load_own, which kernels compiled per "flags given" instantiate.
template <int OWN, class Q>
__device__ __forceinline__ void load_own_or_none(const unsigned char* row, Q q, int T, bool wide, unsigned char (&f)[OWN]) {
  if (row && wide && q + OWN <= (Q)T) {
    load_own<OWN>(row, q, T, true, f);  // the one word
  } else {
#pragma unroll
    for (int k = 0; k < OWN; ++k) f[k] = q + k < (Q)T ? (row ? row[q + k] : (unsigned char)0) : (unsigned char)1;
  }
}

// Segment s of bound [S + 1] is [clamp_bound(bound[s]), clamp_bound(bound[s + 1])): whatever the array holds, every index
// made from it is inside the row.
__device__ __forceinline__ int clamp_bound(int b, int T) { return min(max(b, 0), T); }

// The segment of sample t, by bisection over the clamped bounds: s, and its [lo, hi); -1 with lo = hi = 0 when t is in
// none.  With bounds that do not ascend a sample may take another segment than the caller meant, never an index outside.
__device__ __forceinline__ int find_segment(const int* __restrict__ bound, int S, int T, int t, int& lo, int& hi) {
  int a = 0, b = S;  // the largest a in 0 .. S - 1 with bound[a] <= t, or 0
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (clamp_bound(bound[m], T) <= t)
      a = m;
    else
      b = m;
  }
  lo = clamp_bound(bound[a], T), hi = clamp_bound(bound[a + 1], T);
  if (t >= lo && t < hi) return a;
  lo = hi = 0;
  return -1;
}

// One sample into the right-hand side r [K]: r[i] = r[i] + b[i] * term, i ascending, with b = keep ? B : 0.  A sample
// that is not kept enters as a row of zeros: selected, never multiplied by what it holds.  The caller selects term.
template <int K>
__device__ __forceinline__ void rhs_add(double* r, const double (&B)[K], bool keep, double term) {
#pragma unroll
  for (int i = 0; i < K; ++i) r[i] = r[i] + (keep ? B[i] : 0.0) * term;
}

// (The upper triangle of N, acc[a] = acc[a] + b[i] * b[j] row after row, stays written out in its three kernels, on a
// row b selected in the kernel's own scope: behind a call the compiler keeps b in another form, which costs
// segment_normal_kernel and line_normal_kernel registers, up to a wave of occupancy, and reorders the loop of
// regress_normal_kernel.  DESIGN 3.32 has the figures.)

// One step of the butterfly: v = v + (the value of lane ^ o), for a number or for every element of an array
template <class V>
__device__ __forceinline__ void xor_add(V& v, int o) {
  v = v + __shfl_xor(v, o, kWave);
}
template <class V, int N>
__device__ __forceinline__ void xor_add(V (&v)[N], int o) {
#pragma unroll
  for (int a = 0; a < N; ++a) v[a] = v[a] + __shfl_xor(v[a], o, kWave);
}

// The 64 lanes' values added in a butterfly, xor 32, 16 .. 1: every lane ends with the same sum (a + b is b + a), in an
// order that is the same on every call.  v: a double, an int or an unsigned, or an array of them; the second form takes
// sums and their counter through the same steps together.
template <class V>
__device__ __forceinline__ void wave_sum_all(V& v) {
#pragma unroll
  for (int o = kWave / 2; o >= 1; o >>= 1) xor_add(v, o);
}
template <class V, class C>
__device__ __forceinline__ void wave_sum_all(V& v, C& n) {
#pragma unroll
  for (int o = kWave / 2; o >= 1; o >>= 1) {
    xor_add(v, o);
    xor_add(n, o);
  }
}

// After wave_sum_all: lane i K + j stores N[i][j] to N_item [K][K], lane i stores r[i] to r_item [K].  A lane picks its
// value by selects over compile-time indices: the accumulators are never indexed by a lane's number, so that they
// stay in registers.  The empty asm hides the lane from the compiler, so that the comparisons are made here,
// call by call: hoisted out of the caller's item loop their K K masks would not fit the scalar registers.
template <int K>
__device__ __forceinline__ void store_normal_by_lane(const double (&acc)[K * (K + 1) / 2 + K], int lane, double* N_item, double* r_item) {
  constexpr int NP = K * (K + 1) / 2;
  int me = lane;
  asm volatile("" : "+v"(me));
  double vN = 0.0, vr = 0.0;
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int p = i < j ? i : j, q = i < j ? j : i;
      vN = me == i * K + j ? acc[p * K - p * (p - 1) / 2 + (q - p)] : vN;
    }
    vr = me == i ? acc[NP + i] : vr;
  }
  if (lane < K * K) N_item[lane] = vN;
  if (lane < K) r_item[lane] = vr;
}

}  // namespace mrx_tod
