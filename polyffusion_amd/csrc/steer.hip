// steer.hip - steering a population of candidates while it is sampled (gfx950; include/pfhip.h: pf_x0_predict, pf_steer_resample,
// pf_rows_gather; DESIGN.md 3, "Steering by resampling").  Feynman-Kac / SMC steering of a diffusion sampler (Singhal et al. 2025; Wu et
// al. 2023): every few reverse steps the predicted clean image of every candidate is scored, the population of each group is resampled in
// proportion to exp(lambda * reward gain), and the copies of a survivor diverge again because every row draws its own noise.
//   pf_x0_predict      the predicted clean image of every row, on the elementwise.h skeleton; the expression is x0_predict.h's, which
//                      pf_x0_threshold evaluates too
//   pf_steer_resample  ONE workgroup of 256 lanes per group of n <= 256 particles: weights in parallel (one lane per particle), the sums
//                      and the running sum serially in index order on lane 0, the search of every particle's ancestor in parallel again.
//                      Every float64 operation is one opaque instruction: nothing is contracted, the restatement in numpy is exact.
//   pf_rows_gather     dst row = src row of the ancestor, up to four tensors in one launch; workgroup = (row, chunk of PF_MSE_CHUNK)
// No atomics, no allocation, no host sync; all three are capturable.
#include <cmath>
#include "elementwise.h"
#include "x0_predict.h"

namespace pf {

namespace {

// ------------------------------------------------------------------------------------------------------------------- pf_x0_predict
struct x0_predict_body {
  const float* __restrict__ x; size_t x_row_stride;
  const float* __restrict__ eps;
  const int64_t* __restrict__ t; int32_t t_stride;
  const float* __restrict__ table; int32_t n_table;
  float* __restrict__ x0; size_t row_elems;
  __device__ __forceinline__ void begin() {}
  template <int V>
  __device__ __forceinline__ void at(size_t g) const {           // (V = 4: row_elems % 4 == 0, a group never straddles two rows)
    const size_t i = g * V, row = i / row_elems, col = i - row * row_elems;
    const float* r = x0_table_row(t, t_stride, table, n_table, (unsigned)row);
    const float cx = r[0], ce = r[1];
    float xv[V], ev[V], o[V];
    ew_ld<V>(x + row * x_row_stride + col, xv);
    ew_ld<V>(eps + i, ev);
#pragma unroll
    for (int q = 0; q < V; ++q) o[q] = x0_of(cx, ce, xv[q], ev[q]);
    ew_st<V>(x0 + i, o);
  }
};

// ------------------------------------------------------------------------------------------------------------------- pf_steer_resample
// float64 operations the optimiser cannot merge or reorder (noise.h says why a pragma is not enough)
__device__ __forceinline__ double dmul_rn(double a, double b) { double r; asm("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double dadd_rn(double a, double b) { double r; asm("v_add_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double dsub_rn(double a, double b) { double r; asm("v_add_f64 %0, %1, -%2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ bool dfinite(double v) { return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll; }

constexpr uint32_t kSteerKeyTag = 0x53544552u;       // "STER": the steering stream's key differs from every noise stream's of the same seed

// the first output word of Philox4x32-10 (noise.h's round and key schedule) for counter (g, event) under the tagged key
__device__ __forceinline__ uint32_t steer_word(uint64_t g, uint64_t event, uint64_t seed) {
  uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32), c2 = (uint32_t)event, c3 = (uint32_t)(event >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ kSteerKeyTag;
#pragma unroll
  for (int r = 0; r < 10; ++r) { philox_round(c0, c1, c2, c3, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
  return c0;
}

struct steer_params {
  const double* reward; double* base;
  double lambda, ess_frac;
  uint64_t seed, group_offset, event;
  int32_t* ancestors; double* weights; double* stats;
  int32_t n;
};

__global__ __launch_bounds__(PF_STEER_MAX_N) void steer_resample_kernel(steer_params a) {
  __shared__ double rw[PF_STEER_MAX_N], lw[PF_STEER_MAX_N], cum[PF_STEER_MAX_N];     // reward, log weight -> weight, running sum
  __shared__ double sh_m, sh_u, sh_step;
  __shared__ int sh_flag;
  const int n = a.n, i = threadIdx.x;
  const size_t at = (size_t)blockIdx.x * n;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (i < n) {
    const double r = a.reward[at + i], l = dmul_rn(a.lambda, dsub_rn(r, a.base[at + i]));
    rw[i] = r;
    lw[i] = dfinite(r) && dfinite(l) ? l : nan;                  // NaN marks "weight 0" from here on
  }
  __syncthreads();
  if (i == 0) {                                                  // the maximum of the finite log weights (order-free)
    double m = nan;
    for (int k = 0; k < n; ++k) {
      const double l = lw[k];
      if (l == l && !(m >= l)) m = l;
    }
    sh_m = m;
  }
  __syncthreads();
  if (i < n) {
    const double l = lw[i], w = l == l ? exp(dsub_rn(l, sh_m)) : 0.0;
    lw[i] = w;
    a.weights[at + i] = w;
  }
  __syncthreads();
  if (i == 0) {                                                  // S, Q and the running sum, serially in index order
    double S = 0.0, Q = 0.0;
    for (int k = 0; k < n; ++k) {
      const double w = lw[k];
      S = dadd_rn(S, w);
      Q = dadd_rn(Q, dmul_rn(w, w));
      cum[k] = S;
    }
    const double ess = dmul_rn(S, S) / Q;                        // (0 / 0 = NaN when no particle has a finite weight)
    const double u = (double)steer_word(a.group_offset + blockIdx.x, a.event, a.seed) * (1.0 / 4294967296.0);      // exact: 32 bits
    const int flag = sh_m == sh_m ? (ess <= dmul_rn(a.ess_frac, (double)n) ? 1 : 0) : 2;
    double* st = a.stats + (size_t)blockIdx.x * 4;
    st[0] = ess; st[1] = S; st[2] = (double)flag; st[3] = u;
    sh_u = u;
    sh_step = S / (double)n;
    sh_flag = flag;
  }
  __syncthreads();
  if (i >= n) return;
  int anc = i;
  if (sh_flag == 1) {
    // p_j < S strictly (include/pfhip.h), and cum[] never decreases (w >= 0, a rounded sum is monotone): the first index with
    // cum > p by bisection is the one a scan from 0 finds
    const double p = dmul_rn(dadd_rn((double)i, sh_u), sh_step);
    int lo = 0, hi = n - 1;                                      // the answer lies in [lo, hi]; hi = n - 1 is the clamp
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cum[mid] > p) hi = mid; else lo = mid + 1;
    }
    anc = lo;
    a.base[at + i] = rw[anc];
  }
  a.ancestors[at + i] = anc;
}

// ------------------------------------------------------------------------------------------------------------------- pf_rows_gather
struct gather_params {
  const float* src[PF_GATHER_MAX_TENSORS]; float* dst[PF_GATHER_MAX_TENSORS];
  size_t row_elems[PF_GATHER_MAX_TENSORS];
  unsigned vec_mask;                  // bit k: tensor k moves as 16-byte vectors
  const int32_t* ancestors;
  int32_t n, per;
  unsigned chunks;                    // of the longest row; a workgroup past its tensor's last chunk leaves
};

template <bool VEC>
__device__ __forceinline__ void gather_chunk(const float* __restrict__ s, float* __restrict__ d, size_t n, unsigned chunk) {
#pragma unroll
  for (int g = 0; g < kRowGroups; ++g) {
    const size_t e = row_group_elem(chunk, g);
    if (e < n) store4<VEC>(d, e, n, load4<VEC>(s, e, n));
  }
}

__global__ __launch_bounds__(kRowThreads) void rows_gather_kernel(gather_params a) {
  const unsigned k = blockIdx.y, row = blockIdx.x / a.chunks, chunk = blockIdx.x - row * a.chunks;
  const size_t re = a.row_elems[k];
  if ((size_t)chunk * PF_MSE_CHUNK >= re) return;
  const unsigned particle = row / (unsigned)a.per, sub = row - particle * (unsigned)a.per;
  const unsigned group = particle / (unsigned)a.n;
  int anc = a.ancestors[particle];
  anc = anc < 0 ? 0 : (anc > a.n - 1 ? a.n - 1 : anc);           // a corrupt table cannot make the kernel read outside its inputs
  const size_t from = ((size_t)group * a.n + anc) * a.per + sub;
  const float* s = a.src[k] + from * re;
  float* d = a.dst[k] + (size_t)row * re;
  if (a.vec_mask >> k & 1) gather_chunk<true>(s, d, re, chunk);
  else gather_chunk<false>(s, d, re, chunk);
}

}  // namespace

int launch_x0_predict(const pf_x0_predict_args& a, hipStream_t s) {
  PF_REQUIRE(a.x && a.eps && a.t && a.table && a.x0, "x0_predict: null x, eps, t, table or x0");
  PF_REQUIRE(a.rows > 0 && a.row_elems > 0, "x0_predict: %d rows of %zu elements", a.rows, a.row_elems);
  PF_REQUIRE(a.x_row_stride >= a.row_elems, "x0_predict: x_row_stride %zu below row_elems %zu", a.x_row_stride, a.row_elems);
  PF_REQUIRE(a.t_stride >= 0 && a.n_table > 0, "x0_predict: t_stride %d, n_table %d", a.t_stride, a.n_table);
  const size_t bytes = (size_t)a.rows * a.row_elems * sizeof(float);
  PF_REQUIRE(!ranges_overlap(a.x0, bytes, a.eps, bytes), "x0_predict: x0 overlaps eps");
  PF_REQUIRE(!ranges_overlap(a.x0, bytes, a.x, ((size_t)(a.rows - 1) * a.x_row_stride + a.row_elems) * sizeof(float)), "x0_predict: x0 overlaps x");
  PF_REQUIRE(!ranges_overlap(a.x0, bytes, a.table, (size_t)a.n_table * 4 * sizeof(float)), "x0_predict: x0 overlaps table");
  PF_REQUIRE(!ranges_overlap(a.x0, bytes, a.t, ((size_t)(a.rows - 1) * a.t_stride + 1) * sizeof(int64_t)), "x0_predict: x0 overlaps t");
  // 16-byte accesses: every row of x, eps and x0 then starts 16-byte aligned too
  const bool vec = aligned16({a.x, a.eps, a.x0}) && a.row_elems % 4 == 0 && a.x_row_stride % 4 == 0;
  return ew_launch(vec, x0_predict_body{a.x, a.x_row_stride, a.eps, a.t, a.t_stride, a.table, a.n_table, a.x0, a.row_elems},
                   (size_t)a.rows * a.row_elems, s);
}

int launch_steer_resample(const pf_steer_resample_args& a, hipStream_t s) {
  PF_REQUIRE(a.reward && a.base && a.ancestors && a.weights && a.stats, "steer_resample: null reward, base, ancestors, weights or stats");
  PF_REQUIRE(a.groups > 0, "steer_resample: %d groups", a.groups);
  PF_REQUIRE(a.n >= 1 && a.n <= PF_STEER_MAX_N, "steer_resample: %d particles per group outside [1, %d]", a.n, PF_STEER_MAX_N);
  PF_REQUIRE(std::isfinite(a.lambda) && a.lambda >= 0.0, "steer_resample: lambda %g is not finite and >= 0", a.lambda);
  PF_REQUIRE(a.ess_frac > 0.0 && a.ess_frac <= 1.0, "steer_resample: ess_frac %g outside (0, 1]", a.ess_frac);      // (a NaN fails both)
  PF_REQUIRE((((uintptr_t)a.reward | (uintptr_t)a.base | (uintptr_t)a.weights | (uintptr_t)a.stats) & 7) == 0 && ((uintptr_t)a.ancestors & 3) == 0,
             "steer_resample: reward, base, weights and stats must be 8-byte aligned, ancestors 4-byte aligned");
  const size_t cnt = (size_t)a.groups * a.n, db = cnt * sizeof(double);
  const struct { const void* p; size_t bytes; const char* name; } t[5] = {{a.reward, db, "reward"}, {a.base, db, "base"},
      {a.ancestors, cnt * sizeof(int32_t), "ancestors"}, {a.weights, db, "weights"}, {a.stats, (size_t)a.groups * 4 * sizeof(double), "stats"}};
  for (int p = 0; p < 5; ++p)
    for (int q = p + 1; q < 5; ++q)
      PF_REQUIRE(!ranges_overlap(t[p].p, t[p].bytes, t[q].p, t[q].bytes), "steer_resample: %s overlaps %s", t[p].name, t[q].name);
  steer_params p{a.reward, a.base, a.lambda, a.ess_frac, a.seed, a.group_offset, a.event, a.ancestors, a.weights, a.stats, a.n};
  hipLaunchKernelGGL(steer_resample_kernel, dim3((unsigned)a.groups), dim3(PF_STEER_MAX_N), 0, s, p);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

int launch_rows_gather(const pf_rows_gather_args& a, hipStream_t s) {
  PF_REQUIRE(a.ancestors, "rows_gather: null ancestors");
  PF_REQUIRE(a.n_tensors >= 1 && a.n_tensors <= PF_GATHER_MAX_TENSORS, "rows_gather: %d tensors outside [1, %d]", a.n_tensors, PF_GATHER_MAX_TENSORS);
  PF_REQUIRE(a.groups > 0 && a.n >= 1 && a.per >= 1, "rows_gather: %d groups of %d particles of %d images", a.groups, a.n, a.per);
  const size_t rows = (size_t)a.groups * a.n * a.per;
  PF_REQUIRE(rows < (1ull << 31), "rows_gather: %zu rows", rows);
  PF_REQUIRE(((uintptr_t)a.ancestors & 3) == 0, "rows_gather: ancestors must be 4-byte aligned");
  gather_params p{};
  size_t longest = 0;
  for (int k = 0; k < a.n_tensors; ++k) {
    PF_REQUIRE(a.src[k] && a.dst[k], "rows_gather: null src or dst of tensor %d", k);
    PF_REQUIRE(a.row_elems[k] > 0 && a.row_elems[k] < (1ull << 32), "rows_gather: rows of %zu elements in tensor %d", a.row_elems[k], k);
    PF_REQUIRE((((uintptr_t)a.src[k] | (uintptr_t)a.dst[k]) & 3) == 0, "rows_gather: src and dst of tensor %d must be 4-byte aligned", k);
    p.src[k] = a.src[k]; p.dst[k] = a.dst[k]; p.row_elems[k] = a.row_elems[k];
    if (aligned16({a.src[k], a.dst[k]}) && a.row_elems[k] % 4 == 0) p.vec_mask |= 1u << k;
    longest = a.row_elems[k] > longest ? a.row_elems[k] : longest;
  }
  const size_t anc_bytes = (size_t)a.groups * a.n * sizeof(int32_t);
  for (int k = 0; k < a.n_tensors; ++k) {
    const size_t bk = rows * a.row_elems[k] * sizeof(float);
    PF_REQUIRE(!ranges_overlap(a.dst[k], bk, a.ancestors, anc_bytes), "rows_gather: dst of tensor %d overlaps ancestors", k);
    for (int q = 0; q < a.n_tensors; ++q) {
      const size_t bq = rows * a.row_elems[q] * sizeof(float);
      PF_REQUIRE(!ranges_overlap(a.dst[k], bk, a.src[q], bq), "rows_gather: dst of tensor %d overlaps src of tensor %d (dst is disjoint from src: ping-pong)", k, q);
      PF_REQUIRE(q == k || !ranges_overlap(a.dst[k], bk, a.dst[q], bq), "rows_gather: dst of tensor %d overlaps dst of tensor %d", k, q);
    }
  }
  const size_t chunks = chunks_of(longest, PF_MSE_CHUNK);
  PF_REQUIRE(rows * chunks < (1ull << 31), "rows_gather: %zu rows of %zu elements are more workgroups than one launch holds", rows, longest);
  p.ancestors = a.ancestors; p.n = a.n; p.per = a.per; p.chunks = (unsigned)chunks;
  hipLaunchKernelGGL(rows_gather_kernel, dim3((unsigned)(rows * chunks), (unsigned)a.n_tensors), dim3(kRowThreads), 0, s, p);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

}  // namespace pf
