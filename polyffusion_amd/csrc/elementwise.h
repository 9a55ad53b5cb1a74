// elementwise.h - the two shapes every memory-bound map and row reduction of the library is written in (sampler_steps.hip, loss.hip and the
// posterior samplers of small_kernels.hip):
//   ew_kernel<V, Body>     a grid-stride loop over groups of V in {1, 4} floats; the body holds the operands and the arithmetic
//   row_reduce_store<N>    workgroup = (row, chunk of PF_MSE_CHUNK elements): N per-lane sums -> one partial N-tuple, in a fixed order
//                          (row_reduce_store_dd<N>: the same order with double-double additions, for sums held to an ulp)
// Every operation of the bodies is individually rounded (noise.h) and the reduction order is fixed by (row_elems, element index) alone, so
// the width of an access never changes a bit of a result.
#pragma once
#include <initializer_list>
#include "noise.h"

namespace pf {

// at most 2048 workgroups of 256 lanes; the grid-stride loop does the rest
static inline dim3 ew_grid(size_t n) { return dim3((unsigned)min((size_t)2048, (n + 255) / 256)); }
static inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + b_bytes && pb < pa + a_bytes;
}
static inline size_t chunks_of(size_t row_elems, size_t chunk) { return (row_elems + chunk - 1) / chunk; }
// every pointer of the list 16-byte aligned; an absent (null) operand counts as aligned
static inline bool aligned16(std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  return (bits & 15) == 0;
}

// ---- whole-tensor access: V consecutive floats at p, one 16-byte access (V = 4, p aligned) or one element (V = 1)
template <int V>
__device__ __forceinline__ void ew_ld(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else {
    v[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void ew_st(float* p, const float (&v)[V]) {
  if constexpr (V == 4) {
    const f32x4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p) = t;
  } else {
    *p = v[0];
  }
}
// ---- bounded row access: four consecutive elements of a row starting at element e (a multiple of 4): one 16-byte access when the tensor
// allows it (VEC), else element by element; elements at or past `n` read as 0 / are not written
template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* p, size_t e, size_t n) {
  if (VEC) return *reinterpret_cast<const f32x4*>(p + e);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (e + j < n) v[j] = p[e + j];
  return v;
}
template <bool VEC>
__device__ __forceinline__ void store4(float* p, size_t e, size_t n, f32x4 v) {
  if (VEC) { *reinterpret_cast<f32x4*>(p + e) = v; return; }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (e + j < n) p[e + j] = v[j];
}

// ---- the map.  Body: a struct passed by value with the operand pointers and coefficients, begin() - once per lane before the loop (what
// is uniform over the launch: a table row, a draw index) - and at<V>(g), which handles floats [V * g, V * g + V).
template <int V, class Body>
__global__ void ew_kernel(Body body, size_t groups) {
  body.begin();
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) body.template at<V>(g);
}
template <int V, class Body>
static int ew_launch_v(const Body& body, size_t n, hipStream_t s) {
  hipLaunchKernelGGL((ew_kernel<V, Body>), ew_grid(n / V), dim3(256), 0, s, body, n / V);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}
// n floats as 16-byte groups (vec: the caller has checked n % 4 == 0 and its pointers with aligned16) or one by one
template <class Body>
static int ew_launch(bool vec, const Body& body, size_t n, hipStream_t s) {
  return vec ? ew_launch_v<4>(body, n, s) : ew_launch_v<1>(body, n, s);
}

// ---- the row reduction.  A workgroup of kRowThreads lanes owns chunk `chunk` of row `row`; lane l owns the 16-byte groups l, l + 256, ...
// of the chunk (row_group_elem) and adds its terms in element order.  row_reduce_store then combines the lanes of a wave by a butterfly
// (every lane ends with the same sum) and the four waves in wave order, and writes the workgroup's N sums to
// out[(row * chunks + chunk) * N + k]; row_partials_sum adds a row's N-tuples in chunk order.  No atomics anywhere.
constexpr int kRowThreads = 256;
constexpr int kRowGroups = PF_MSE_CHUNK / 4 / kRowThreads;   // 16-byte groups of a chunk per lane
static_assert(PF_MSE_CHUNK == 4 * kRowThreads * kRowGroups, "PF_MSE_CHUNK must be a whole number of 16-byte groups per lane");
__device__ __forceinline__ size_t row_group_elem(unsigned chunk, int k) { return (size_t)chunk * PF_MSE_CHUNK + 4 * ((size_t)k * kRowThreads + threadIdx.x); }

template <int N, class T>
__device__ __forceinline__ void row_reduce_store(T (&acc)[N], T* __restrict__ out, unsigned row, unsigned chunks, unsigned chunk) {
  __shared__ T wave_sum[kRowThreads / 64][N];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] += __shfl_xor(acc[k], m, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) wave_sum[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    T s = wave_sum[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kRowThreads / 64; ++w) s += wave_sum[w][threadIdx.x];
    out[((size_t)row * chunks + chunk) * N + threadIdx.x] = s;
  }
}
template <int N>
__device__ __forceinline__ void row_partials_sum(const double* __restrict__ partial, unsigned row, unsigned chunks, double (&s)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] = 0.0;
  for (unsigned c = 0; c < chunks; ++c) {
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] += partial[((size_t)row * chunks + c) * N + k];
  }
}

// ---- the same reduction, in the same order, with every addition carried out in double-double: a sum is an unevaluated pair hi + lo
// (|lo| <= ulp(hi) / 2), an addition keeps the rounding error of hi + hi exactly (Knuth's TwoSum) and folds it into lo, so a row sum of
// n <= 2^31 terms is good to about n * 2^-104 of sum |term| and its hi is the correctly rounded sum but for near-ties - where a plain
// float64 sum in this order is one to several ulps off.  For callers whose tolerance is an ulp of the sum (pf_cfg_rescale).  dd_add is
// symmetric in its operands, so both lanes of a butterfly step form the same pair.  Partials: out[((row * chunks + chunk) * N + k) * 2 + {0: hi, 1: lo}].
struct dd { double hi, lo; };
__device__ __forceinline__ dd dd_renorm(double s, double e) {
#pragma clang fp contract(off)
  const double hi = s + e;
  return dd{hi, e - (hi - s)};
}
__device__ __forceinline__ dd dd_add(dd x, dd y) {
#pragma clang fp contract(off)
  const double s = x.hi + y.hi, bb = s - x.hi;
  const double e = (x.hi - (s - bb)) + (y.hi - bb);      // the rounding error of s, exactly
  return dd_renorm(s, e + (x.lo + y.lo));
}
__device__ __forceinline__ dd dd_add(dd x, double t) { return dd_add(x, dd{t, 0.0}); }

template <int N>
__device__ __forceinline__ void row_reduce_store_dd(dd (&acc)[N], double* __restrict__ out, unsigned row, unsigned chunks, unsigned chunk) {
  __shared__ dd wave_sum[kRowThreads / 64][N];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = dd_add(acc[k], dd{__shfl_xor(acc[k].hi, m, 64), __shfl_xor(acc[k].lo, m, 64)});
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) wave_sum[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    dd s = wave_sum[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kRowThreads / 64; ++w) s = dd_add(s, wave_sum[w][threadIdx.x]);
    double* dst = out + (((size_t)row * chunks + chunk) * N + threadIdx.x) * 2;
    dst[0] = s.hi;
    dst[1] = s.lo;
  }
}
// a row's pairs added in chunk order; s[k] = hi of the total
template <int N>
__device__ __forceinline__ void row_partials_sum_dd(const double* __restrict__ partial, unsigned row, unsigned chunks, double (&s)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    dd t{0.0, 0.0};
    for (unsigned c = 0; c < chunks; ++c) {
      const double* src = partial + (((size_t)row * chunks + c) * N + k) * 2;
      t = dd_add(t, dd{src[0], src[1]});
    }
    s[k] = t.hi;
  }
}

}  // namespace pf
