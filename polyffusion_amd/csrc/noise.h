// noise.h - device helpers shared by the elementwise kernels of sampler_steps.hip, small_kernels.hip and loss.hip: the individually rounded fp32
// operations and the counter-based Gaussian generator.  Every translation unit that includes this compiles the SAME bodies, which is
// what makes "noise drawn in the kernel" bit-identical to pf_randn wherever it is drawn.
#pragma once
#include "pf_internal.h"

namespace pf {

// Individually rounded fp32 operations the optimiser cannot merge.  __fmul_rn / __fadd_rn are plain * and + in this toolchain (no
// OCML_BASIC_ROUNDED_OPERATIONS) and `#pragma clang fp contract(off)` does not survive inlining + SLP vectorisation here (the *_step_rng
// kernels came out with v_pk_fma_f32 where the scalar kernels had separate multiplies and adds: last-bit differences between two
// kernels that must agree).  One opaque VALU instruction per operation: every kernel that inlines the update computes the same bits,
// in the reference's operation order (each product rounded, then the sum).
__device__ __forceinline__ float mul_rn(float a, float b) { float r; asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float add_rn(float a, float b) { float r; asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float sub_rn(float a, float b) { float r; asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

// ------------------------------------------------------------------ Philox4x32-10 + Box-Muller
__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
  c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}
// the four standard normals of group g (elements 4g .. 4g+3 of the global tensor) of draw `sid`: counter = (g lo, g hi, sid lo, sid hi),
// key = (seed lo, seed hi), (z0, z1) = r(u0) (cos, sin)(2 pi u1), (z2, z3) = r(u2) (cos, sin)(2 pi u3), r(u) = sqrt(-2 ln u).
// The uniforms are NOT the open interval the form suggests: with m = c >> 8, m + 0.5f is an fp32 number only below 2^23 (u = (2 m + 1) 2^-25);
// from 2^23 on it rounds to even, so in [0.5, 1] the uniforms lie on the grid of 2^-23 and m = 2^24 - 1 gives u = 1.0 exactly.  The real
// range is [2^-25, 1]: u is never 0 (largest radius sqrt(50 ln 2) = 5.887, no draw is infinite or NaN), and u0 = 1.0 - 2^-24 of all pairs -
// gives radius 0 and a pair of exact (+-)0.  Harmless, and goldens, recorded parity runs and users' seeds depend on this stream bit for bit:
// do not "clean up" the mapping.  tests/noise_matrix.py states it exactly and tests/test_gpu_noise_matrix.py holds every site to it.
// NOT inlined: randn_kernel and the kernels that draw their own noise must produce the same bits for the same (g, sid, seed), and the
// generated code of logf / sincosf / the products around them depends on its surroundings when inlined (measured: two calls in one kernel
// differ from the stand-alone kernel in the last bit of ~20 % of the draws) - one shared body is the same arithmetic by construction.
__device__ __noinline__ f32x4 philox_normal4v(uint64_t g, uint64_t sid, uint64_t seed) {
#pragma clang fp contract(off)
  float z[4];
  uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32), c2 = (uint32_t)sid, c3 = (uint32_t)(sid >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) { philox_round(c0, c1, c2, c3, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
  const float u0 = ((float)(c0 >> 8) + 0.5f) * (1.0f / 16777216.0f), u1 = ((float)(c1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = ((float)(c2 >> 8) + 0.5f) * (1.0f / 16777216.0f), u3 = ((float)(c3 >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float ra = sqrtf(-2.0f * logf(u0)), rb = sqrtf(-2.0f * logf(u2));
  float sa, ca, sb, cb;
  sincosf(6.283185307179586f * u1, &sa, &ca);
  sincosf(6.283185307179586f * u3, &sb, &cb);
  z[0] = ra * ca; z[1] = ra * sa; z[2] = rb * cb; z[3] = rb * sb;
  return f32x4{z[0], z[1], z[2], z[3]};
}
__device__ __forceinline__ void philox_normal4(uint64_t g, uint64_t sid, uint64_t seed, float (&z)[4]) {
  const f32x4 v = philox_normal4v(g, sid, seed);
  z[0] = v[0]; z[1] = v[1]; z[2] = v[2]; z[3] = v[3];
}

}  // namespace pf
