// sampler_steps.hip - the sampler's elementwise family (gfx950), written against elementwise.h:
//   guidance combines (pf_cfg_combine, pf_cfg_combine3), the combine rescaled to the conditional prediction's per-row standard deviation as a
//   reduce and a combine launch (pf_cfg_rescale), and the canvas <-> window-batch gathers of joint overlapping-window sampling
//   (pf_window_split, pf_window_merge),
//   fused sampler updates (sampler_sdf.py:80-171,307-341; sampler_ddim.py:220-272,355-359), and the update of the sampler the reference
//   does not have, DPM-Solver++(2M) (pf_dpm_step) and its stochastic form (pf_dpm_sde_step), the RePaint re-noise (pf_axpby),
//   the device-resident step state (pf_step_state_set / begin / end / advance) and counter-based Gaussian noise (pf_randn, pf_randn_dev),
//   one fixed-point iterate of exact DDIM inversion with its fused residual (pf_invert_step),
//   the frames of a path between two noises, per-row slerp as a reduce and a combine launch (pf_slerp_rows).
// Every map is a body struct run by ew_kernel at one or both widths; every row sum goes through row_reduce_store / row_partials_sum
// or their double-double forms.
#include "elementwise.h"

namespace pf {

// ------------------------------------------------------------------ guidance
// e_u + s * (e_c - e_u) as three rounded operations, like the reference's tensor ops (shared with window_merge_body below)
__device__ __forceinline__ float cfg_combine_v(float u, float c, float s) { return add_rn(u, mul_rn(s, sub_rn(c, u))); }
struct cfg_combine_body {
  const float* __restrict__ e2; float s; float* __restrict__ e; size_t n;
  __device__ __forceinline__ void begin() {}
  template <int V>
  __device__ __forceinline__ void at(size_t i) const { e[i] = cfg_combine_v(e2[i], e2[n + i], s); }
};
int launch_cfg_combine(const float* eps2, float scale, float* eps, size_t n, hipStream_t s) {
  PF_REQUIRE(eps2 && eps && n > 0, "cfg_combine: bad arguments");
  return ew_launch_v<1>(cfg_combine_body{eps2, scale, eps, n}, n, s);
}

// Dual guidance (DualScale in sampler.py): e3 = [e0 | e1 | e2], the evaluations with both parts of the condition dropped, one kept, both kept.
//   e = e0 + s1 * (e1 - e0) + s2 * (e2 - e1)   as five rounded operations in this order (e1 == e2: cfg_combine_body's bits on [e0 | e1])
__device__ __forceinline__ float cfg_combine3_v(float e0, float e1, float e2, float s1, float s2) {
  return add_rn(add_rn(e0, mul_rn(s1, sub_rn(e1, e0))), mul_rn(s2, sub_rn(e2, e1)));
}
// 16-byte groups need e3 and e aligned and n % 4 == 0 - so e3 + n and e3 + 2n are aligned too and a group never straddles two thirds
struct cfg_combine3_body {
  const float* __restrict__ e3; float s1, s2; float* __restrict__ e; size_t n;
  __device__ __forceinline__ void begin() {}
  template <int V>
  __device__ __forceinline__ void at(size_t g) const {
    const size_t i = g * V;
    float a[V], b[V], c[V], o[V];
    ew_ld<V>(e3 + i, a); ew_ld<V>(e3 + n + i, b); ew_ld<V>(e3 + 2 * n + i, c);
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = cfg_combine3_v(a[j], b[j], c[j], s1, s2);
    ew_st<V>(e + i, o);
  }
};
int launch_cfg_combine3(const float* eps3, float s1, float s2, float* eps, size_t n, hipStream_t s) {
  PF_REQUIRE(eps3 && eps && n > 0, "cfg_combine3: bad arguments");
  return ew_launch(aligned16({eps3, eps}) && n % 4 == 0, cfg_combine3_body{eps3, s1, s2, eps, n}, n, s);
}

// ---- guidance rescale (include/pfhip.h: pf_cfg_rescale; DESIGN.md 3, "Guidance rescale and interval"; Lin et al. 2024, section 3.4): the
// combine above, scaled per row towards the standard deviation of the fully conditional group, out = e_cfg * w with
// w = phi * sqrt(var_pos / var_cfg) + (1 - phi).  Two launches, a workgroup = (row, chunk of PF_MSE_CHUNK), as pf_slerp_rows:
//   reduce   the row reduction of elementwise.h with four sums - e_pos, e_pos^2, e_cfg, e_cfg^2, every term widened to float64 first (the
//            squares are then exact) - in its double-double form (row_reduce_store_dd: the same order, every addition keeps its rounding
//            error), because the sums are held to an ulp: a plain float64 sum in this order was measured up to two ulps off.  One partial
//            4-tuple of (hi, lo) pairs per workgroup, no atomics
//   combine  EVERY workgroup of a row adds the row's 4-tuples in chunk order (the same four doubles in each of them), lane 0 forms w in
//            float64 and rounds it to float once; then the groups are read once more, e_cfg recomputed and e_cfg * w written.
// VEC and the element-by-element form do the same operations: the same bits.
// the four elements at e of one row: e_pos (the last group) and e_cfg (cfg_combine_v / cfg_combine3_v of the groups); gs = one group's elements
template <bool VEC>
__device__ __forceinline__ void cfg_rescale_load(const float* __restrict__ epsg, int groups, size_t gs, size_t base, size_t e, size_t row_elems,
                                                 float s1, float s2, f32x4& pos, f32x4& cfg) {
  const f32x4 a = load4<VEC>(epsg + base, e, row_elems), b = load4<VEC>(epsg + gs + base, e, row_elems);
  if (groups == 2) {
    pos = b;
#pragma unroll
    for (int j = 0; j < 4; ++j) cfg[j] = cfg_combine_v(a[j], b[j], s1);
  } else {
    pos = load4<VEC>(epsg + 2 * gs + base, e, row_elems);
#pragma unroll
    for (int j = 0; j < 4; ++j) cfg[j] = cfg_combine3_v(a[j], b[j], pos[j], s1, s2);
  }
}
template <bool VEC>
__global__ __launch_bounds__(kRowThreads) void cfg_rescale_reduce_kernel(const float* __restrict__ epsg, int groups, size_t gs, float s1, float s2,
                                                                        double* __restrict__ partial, size_t row_elems, unsigned chunks) {
  const unsigned row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks;
  const size_t base = (size_t)row * row_elems;
  dd acc[4] = {};
#pragma unroll
  for (int k = 0; k < kRowGroups; ++k) {
    const size_t e = row_group_elem(chunk, k);
    if (e < row_elems) {
      f32x4 pv, cv;
      cfg_rescale_load<VEC>(epsg, groups, gs, base, e, row_elems, s1, s2, pv, cv);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (VEC || e + j < row_elems) {
          const double p = (double)pv[j], c = (double)cv[j];
          acc[0] = dd_add(acc[0], p);
          acc[1] = dd_add(acc[1], p * p);        // (the square of a widened float is exact)
          acc[2] = dd_add(acc[2], c);
          acc[3] = dd_add(acc[3], c * c);
        }
    }
  }
  row_reduce_store_dd(acc, partial, row, chunks, chunk);
}
// var = sum x^2 / n - (sum x / n)^2 and f = sqrt(var_pos / var_cfg), in float64.  f = 1 - the row then comes out as e_cfg, bit for bit -
// when var_cfg is not > 0 (a constant row, or NaN) or the root is not finite (a quotient that overflowed, is NaN, or is negative because
// var_pos cancelled below zero): there is no scale to restore.
template <bool VEC>
__global__ __launch_bounds__(kRowThreads) void cfg_rescale_combine_kernel(const float* __restrict__ epsg, int groups, size_t gs, float s1, float s2,
                                                                         double phi, const double* __restrict__ partial, float* __restrict__ out,
                                                                         double* __restrict__ stats, float* __restrict__ weights,
                                                                         size_t row_elems, unsigned chunks) {
  __shared__ float w_sh;
  const unsigned row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks;
  if (threadIdx.x == 0) {
#pragma clang fp contract(off)             // every float64 operation below individually rounded: the formula as written
    double sum[4];                         // e_pos, e_pos^2, e_cfg, e_cfg^2
    row_partials_sum_dd(partial, row, chunks, sum);
    const double n = (double)row_elems, mp = sum[0] / n, mc = sum[2] / n;
    const double var_pos = sum[1] / n - mp * mp, var_cfg = sum[3] / n - mc * mc;
    double f = sqrt(var_pos / var_cfg);
    if (!(var_cfg > 0.0) || !isfinite(f)) f = 1.0;
    const float w = (float)(phi * f + (1.0 - phi));
    w_sh = w;
    if (chunk == 0) {
      if (stats) {
        stats[(size_t)row * 3 + 0] = var_pos;
        stats[(size_t)row * 3 + 1] = var_cfg;
        stats[(size_t)row * 3 + 2] = f;
      }
      if (weights) weights[row] = w;
    }
  }
  __syncthreads();
  const float w = w_sh;
  const size_t base = (size_t)row * row_elems;
#pragma unroll
  for (int k = 0; k < kRowGroups; ++k) {
    const size_t e = row_group_elem(chunk, k);
    if (e < row_elems) {
      f32x4 pv, cv, o;
      cfg_rescale_load<VEC>(epsg, groups, gs, base, e, row_elems, s1, s2, pv, cv);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = mul_rn(cv[j], w);
      store4<VEC>(out + base, e, row_elems, o);
    }
  }
}
size_t cfg_rescale_workspace_bytes(int rows, size_t row_elems) {
  if (rows <= 0 || row_elems == 0) return 0;
  return (size_t)rows * chunks_of(row_elems, PF_MSE_CHUNK) * 4 * 2 * sizeof(double);
}
int launch_cfg_rescale(const pf_cfg_rescale_args& a, hipStream_t s) {
  PF_REQUIRE(a.epsg && a.eps, "cfg_rescale: null epsg or eps");
  PF_REQUIRE(a.groups == 2 || a.groups == 3, "cfg_rescale: groups %d, expected 2 or 3 (one group has nothing to rescale)", a.groups);
  PF_REQUIRE(a.rows > 0 && a.row_elems > 0, "cfg_rescale: %d rows of %zu elements", a.rows, a.row_elems);
  PF_REQUIRE(a.phi >= 0.0 && a.phi <= 1.0, "cfg_rescale: phi %g outside [0, 1]", a.phi);       // (a NaN fails both)
  const size_t chunks = chunks_of(a.row_elems, PF_MSE_CHUNK), need = cfg_rescale_workspace_bytes(a.rows, a.row_elems);
  PF_REQUIRE(chunks * (size_t)a.rows < (1ull << 31), "cfg_rescale: %d rows of %zu elements are more workgroups than one launch holds", a.rows, a.row_elems);
  const size_t gs = (size_t)a.rows * a.row_elems, bytes = gs * sizeof(float);
  PF_REQUIRE(!ranges_overlap(a.eps, bytes, a.epsg, bytes * a.groups), "cfg_rescale: eps overlaps epsg (the combine launch reads the groups again)");
  PF_REQUIRE(((uintptr_t)a.stats & 7) == 0, "cfg_rescale: stats must be 8-byte aligned");
  PF_REQUIRE(a.workspace, "cfg_rescale: no workspace (pf_cfg_rescale_workspace_bytes)");
  PF_REQUIRE(a.workspace_bytes >= need, "cfg_rescale: workspace of %zu bytes required, got %zu", need, a.workspace_bytes);
  PF_REQUIRE(((uintptr_t)a.workspace & 7) == 0, "cfg_rescale: workspace must be 8-byte aligned");
  const bool vec = aligned16({a.epsg, a.eps}) && a.row_elems % 4 == 0;      // then every group and every row starts 16-byte aligned too
  const dim3 grid((unsigned)(chunks * a.rows)), block(kRowThreads);
  double* partial = reinterpret_cast<double*>(a.workspace);
  if (vec)
    hipLaunchKernelGGL(cfg_rescale_reduce_kernel<true>, grid, block, 0, s, a.epsg, a.groups, gs, a.s1, a.s2, partial, a.row_elems, (unsigned)chunks);
  else
    hipLaunchKernelGGL(cfg_rescale_reduce_kernel<false>, grid, block, 0, s, a.epsg, a.groups, gs, a.s1, a.s2, partial, a.row_elems, (unsigned)chunks);
  PF_CHECK_HIP(hipGetLastError());
  if (vec)
    hipLaunchKernelGGL(cfg_rescale_combine_kernel<true>, grid, block, 0, s, a.epsg, a.groups, gs, a.s1, a.s2, a.phi, partial, a.eps, a.stats, a.weights,
                       a.row_elems, (unsigned)chunks);
  else
    hipLaunchKernelGGL(cfg_rescale_combine_kernel<false>, grid, block, 0, s, a.epsg, a.groups, gs, a.s1, a.s2, a.phi, partial, a.eps, a.stats, a.weights,
                       a.row_elems, (unsigned)chunks);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// ---- overlapping windows along the time axis (include/pfhip.h: pf_window_split / pf_window_merge; WindowPlan in sampler.py).  A song is a
// canvas [S][C][Hc][W], Hc = stride * (Wn - 1) + Hw; window j of song s - batch row s * Wn + j - is canvas rows [j * stride, j * stride + Hw).
// Both bodies are gathers over their OUTPUT (split: a window element reads one canvas element; merge: a canvas element reads the <= 8
// windows that cover its row, in ascending j): no atomics, no LDS, nothing order-dependent.  V = 4: 16-byte vectors along W (W % 4 == 0 and
// aligned pointers, the launchers decide), V = 1: 4-byte elements; the same individually rounded operations, so the same bits.
struct window_geom { int S, C, Hw, W, Wn, stride, Hc; };
struct window_split_body {
  const float* __restrict__ canvas; float* __restrict__ win; window_geom g;
  __device__ __forceinline__ void begin() {}
  template <int V>
  __device__ __forceinline__ void at(size_t i) const {
    const size_t Wv = (size_t)(g.W / V), wv = i % Wv;
    size_t r = i / Wv;
    const size_t row = r % g.Hw; r /= g.Hw;
    const size_t c = r % g.C; r /= g.C;
    const size_t j = r % g.Wn, s = r / g.Wn;
    float v[V];
    ew_ld<V>(canvas + ((s * g.C + c) * g.Hc + j * g.stride + row) * g.W + wv * V, v);
    ew_st<V>(win + i * V, v);
  }
};
// eps = [groups][S * Wn][C][Hw][W]; per covering window e_j = the guidance combine of its groups (the device functions of pf_cfg_combine /
// pf_cfg_combine3), then: one window - out = e_j (a select); several - num = w_0*e_0, num += w_j*e_j, den likewise from the weights, out = num / den
struct window_merge_body {
  const float* __restrict__ eps; const float* __restrict__ rw; int groups; float s1, s2; window_geom g; float* __restrict__ out;
  __device__ __forceinline__ void begin() {}
  template <int V>
  __device__ __forceinline__ void at(size_t i) const {
    const size_t Wv = (size_t)(g.W / V), wv = i % Wv;
    const size_t gs = (size_t)g.S * g.Wn * g.C * g.Hw * g.W;       // elements of one group
    size_t r = i / Wv;
    const int y = (int)(r % g.Hc); r /= g.Hc;
    const size_t c = r % g.C, s = r / g.C;
    const int j0 = y < g.Hw ? 0 : (y - g.Hw) / g.stride + 1, j1 = min(g.Wn - 1, y / g.stride);    // 0 <= y - j * stride < Hw for j0 <= j <= j1
    float num[V], den = 0.f;
    for (int j = j0; j <= j1; ++j) {
      const int row = y - j * g.stride;
      const size_t src = (((s * g.Wn + j) * g.C + c) * g.Hw + row) * g.W + wv * V;
      float e[V];
      ew_ld<V>(eps + src, e);
      if (groups == 2) {
        float b[V];
        ew_ld<V>(eps + gs + src, b);
#pragma unroll
        for (int q = 0; q < V; ++q) e[q] = cfg_combine_v(e[q], b[q], s1);
      } else if (groups == 3) {
        float b[V], d[V];
        ew_ld<V>(eps + gs + src, b);
        ew_ld<V>(eps + 2 * gs + src, d);
#pragma unroll
        for (int q = 0; q < V; ++q) e[q] = cfg_combine3_v(e[q], b[q], d[q], s1, s2);
      }
      if (j0 == j1) {
#pragma unroll
        for (int q = 0; q < V; ++q) num[q] = e[q];
      } else {
        const float w = rw[row];
#pragma unroll
        for (int q = 0; q < V; ++q) num[q] = j == j0 ? mul_rn(w, e[q]) : add_rn(num[q], mul_rn(w, e[q]));
        den = j == j0 ? w : add_rn(den, w);
      }
    }
    if (j0 != j1) {
#pragma unroll
      for (int q = 0; q < V; ++q) num[q] = __fdiv_rn(num[q], den);
    }
    ew_st<V>(out + i * V, num);
  }
};
// the geometry both entries share; refused before any HIP call
static int window_geom_of(const char* who, int songs, int channels, int win_h, int width, int n_windows, int stride, window_geom* g) {
  PF_REQUIRE(songs > 0 && channels > 0 && win_h > 0 && width > 0 && n_windows > 0,
             "%s: non-positive extent (songs %d, channels %d, win_h %d, width %d, n_windows %d)", who, songs, channels, win_h, width, n_windows);
  PF_REQUIRE(stride >= 1, "%s: stride %d < 1", who, stride);
  PF_REQUIRE(stride <= win_h, "%s: stride %d > win_h %d (rows between two windows would belong to none)", who, stride, win_h);
  PF_REQUIRE((win_h + stride - 1) / stride <= 8, "%s: ceil(win_h / stride) = %d windows over one row, at most 8", who, (win_h + stride - 1) / stride);
  const int64_t hc = (int64_t)stride * (n_windows - 1) + win_h;
  PF_REQUIRE(hc <= INT32_MAX, "%s: canvas height %lld does not fit 32 bits", who, (long long)hc);
  *g = window_geom{songs, channels, win_h, width, n_windows, stride, (int)hc};
  return PF_OK;
}
int launch_window_split(const float* canvas, float* windows, int songs, int channels, int win_h, int width, int n_windows, int stride,
                        hipStream_t s) {
  window_geom g;
  if (int rc = window_geom_of("window_split", songs, channels, win_h, width, n_windows, stride, &g)) return rc;
  PF_REQUIRE(canvas && windows, "window_split: null pointer");
  const size_t n = (size_t)g.S * g.Wn * g.C * g.Hw * g.W, nc = (size_t)g.S * g.C * g.Hc * g.W;
  PF_REQUIRE(!ranges_overlap(windows, n * sizeof(float), canvas, nc * sizeof(float)), "window_split: windows aliases canvas");
  return ew_launch(g.W % 4 == 0 && aligned16({canvas, windows}), window_split_body{canvas, windows, g}, n, s);
}
int launch_window_merge(const pf_window_merge_args& a, hipStream_t s) {
  window_geom g;
  if (int rc = window_geom_of("window_merge", a.songs, a.channels, a.win_h, a.width, a.n_windows, a.stride, &g)) return rc;
  PF_REQUIRE(a.groups >= 1 && a.groups <= 3, "window_merge: groups %d, expected 1, 2 or 3", a.groups);
  PF_REQUIRE(a.eps && a.row_weight && a.out, "window_merge: null pointer (eps, row_weight and out must be set)");
  const size_t ne = (size_t)a.groups * g.S * g.Wn * g.C * g.Hw * g.W, n = (size_t)g.S * g.C * g.Hc * g.W;
  PF_REQUIRE(!ranges_overlap(a.out, n * sizeof(float), a.eps, ne * sizeof(float)) &&
                 !ranges_overlap(a.out, n * sizeof(float), a.row_weight, (size_t)g.Hw * sizeof(float)),
             "window_merge: out aliases an input");
  return ew_launch(g.W % 4 == 0 && aligned16({a.eps, a.row_weight, a.out}), window_merge_body{a.eps, a.row_weight, a.groups, a.s1, a.s2, g, a.out}, n, s);
}

// ------------------------------------------------------------------ the reverse-step updates
// coefficients passed by value, or - table != nullptr - the row of a device table named by the device-resident step state (graph replay)
template <class Coef>
__device__ __forceinline__ Coef coef_of(Coef c, const Coef* table, const pf_step_state* st) {
  if (table) c = table[st->index];
  return c;
}
// exactly one of the two sources
template <class Args>
static int check_coef_source(const Args& a, const char* name) {
  PF_REQUIRE(!(a.coef && (a.table || a.state)), "%s: coefficients both by value (coef) and from the device (table / state)", name);
  PF_REQUIRE(a.coef || (a.table && a.state), "%s: null coefficients (set coef, or table and state)", name);
  return PF_OK;
}

// one element of the DDPM / RePaint update on VALUES (has_*: which optional operands take part)
__device__ __forceinline__ float ddpm_update_v(float xv, float ev, bool has_p, float np, bool has_orig, bool has_q, float nq, float ov, float m,
                                               const pf_ddpm_coef& c) {
  // same operation order as the reference (each product rounded, then the sum)
  const float x0 = sub_rn(mul_rn(c.c_recip, xv), mul_rn(c.c_recipm1, ev));
  const float mean = add_rn(mul_rn(c.c_x0, x0), mul_rn(c.c_xt, xv));
  float xu = mean;
  if (has_p) xu = add_rn(mean, mul_rn(c.sigma, np));
  if (has_orig) {
    float xk = mul_rn(c.sqrt_ab, ov);
    if (has_q) xk = add_rn(xk, mul_rn(c.sqrt_1mab, nq));
    xu = add_rn(mul_rn(xk, m), mul_rn(xu, sub_rn(1.0f, m)));
  }
  return xu;
}
__device__ __forceinline__ float ddim_update_v(float xv, float e, bool has_noise, float nz, bool has_orig, float ov, float onv, float m,
                                               const pf_ddim_coef& c) {
  const float p0 = __fdiv_rn(sub_rn(xv, mul_rn(c.s1m, e)), c.sqrt_a);   // (a correctly rounded division has nothing to be merged with)
  float xp = add_rn(mul_rn(c.sqrt_aprev, p0), mul_rn(c.dir_coef, e));
  if (has_noise) xp = add_rn(xp, mul_rn(c.sigma, nz));
  if (has_orig) {
    const float ot = add_rn(mul_rn(c.q_sqrt_a, ov), mul_rn(c.q_s1m, onv));
    xp = add_rn(mul_rn(ot, m), mul_rn(xp, sub_rn(1.0f, m)));
  }
  return xp;
}
// The two bodies, each in two forms.  RNG = false: the noise comes from tensors (a null one: no such term), one element per lane.
// RNG = true: a lane owns the four elements of one Philox group and draws philox_normal4 of (group, draw index, seed) - exactly what
// randn_kernel stores for that draw - so the result is bit-identical to randn + the tensor form, without the noise tensors' round trip
// through HBM.  x and out carry no __restrict__: x_out may alias x (the captured step updates x where it stands).
template <bool RNG>
struct ddpm_step_body {
  const float* x; const float* __restrict__ eps; const float* __restrict__ np; const float* __restrict__ nq;
  const float* __restrict__ orig; const float* __restrict__ mask;
  pf_ddpm_coef c; const pf_ddpm_coef* __restrict__ table; const pf_step_state* __restrict__ st;
  uint64_t seed, draw_q, draw_p, off; float* out;
  __device__ __forceinline__ void begin() {
    c = coef_of(c, table, st);
    if (RNG && st) { draw_q = st->draws; draw_p = st->draws + (orig ? 1u : 0u); }
  }
  template <int V>
  __device__ __forceinline__ void at(size_t g) const {
    static_assert(!RNG || V == 4, "one Philox call yields the four normals of a 16-byte group");
    const size_t i = g * V;
    float xv[V], ev[V], zp[V] = {}, zq[V] = {}, ov[V] = {}, mv[V] = {}, o[V];
    if constexpr (RNG) {
      philox_normal4((off >> 2) + g, draw_p, seed, zp);
      if (orig) philox_normal4((off >> 2) + g, draw_q, seed, zq);
    } else {
      if (np) ew_ld<V>(np + i, zp);
      if (nq) ew_ld<V>(nq + i, zq);
    }
    ew_ld<V>(x + i, xv); ew_ld<V>(eps + i, ev);
    if (orig) { ew_ld<V>(orig + i, ov); ew_ld<V>(mask + i, mv); }
    const bool has_p = RNG || np != nullptr, has_q = RNG ? orig != nullptr : nq != nullptr;
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = ddpm_update_v(xv[j], ev[j], has_p, zp[j], orig != nullptr, has_q, zq[j], ov[j], mv[j], c);
    ew_st<V>(out + i, o);
  }
};
template <bool RNG>
struct ddim_step_body {
  const float* x; const float* __restrict__ eps; const float* __restrict__ noise; const float* __restrict__ orig;
  const float* __restrict__ on; const float* __restrict__ mask;
  pf_ddim_coef c; const pf_ddim_coef* __restrict__ table; const pf_step_state* __restrict__ st;
  uint64_t seed, draw, off; float* out;
  __device__ __forceinline__ void begin() {
    c = coef_of(c, table, st);
    if (RNG && st) draw = st->draws;
  }
  template <int V>
  __device__ __forceinline__ void at(size_t g) const {
    static_assert(!RNG || V == 4, "one Philox call yields the four normals of a 16-byte group");
    const size_t i = g * V;
    float xv[V], ev[V], z[V] = {}, ov[V] = {}, nv[V] = {}, mv[V] = {}, o[V];
    if constexpr (RNG) {
      philox_normal4((off >> 2) + g, draw, seed, z);
    } else {
      if (noise) ew_ld<V>(noise + i, z);
    }
    ew_ld<V>(x + i, xv); ew_ld<V>(eps + i, ev);
    if (orig) { ew_ld<V>(orig + i, ov); ew_ld<V>(on + i, nv); ew_ld<V>(mask + i, mv); }
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = ddim_update_v(xv[j], ev[j], RNG || noise != nullptr, z[j], orig != nullptr, ov[j], nv[j], mv[j], c);
    ew_st<V>(out + i, o);
  }
};
// one launcher per family: validate, then the tensor-noise or the in-kernel-noise form
template <class Args>
static int check_step_args(const Args& a, bool known_ok, bool any_noise, const char* name) {
  PF_REQUIRE(a.x && a.eps && a.x_out && a.n > 0 && known_ok, "%s: bad arguments", name);
  if (int rc = check_coef_source(a, name)) return rc;
  if (!a.rng) return PF_OK;
  PF_REQUIRE(!any_noise, "%s_rng: the noise is drawn in the kernel, noise tensors must be NULL", name);
  PF_REQUIRE(a.n % 4 == 0 && a.elem_offset % 4 == 0, "%s_rng: n and elem_offset must be multiples of 4 (one Philox call yields four normals)", name);
  return PF_OK;
}
int launch_ddpm_step(const pf_ddpm_step_args& a, hipStream_t s) {
  if (int rc = check_step_args(a, !a.orig || a.mask, a.noise_p || a.noise_q, "ddpm_step")) return rc;
  const pf_ddpm_coef cv = a.coef ? *a.coef : pf_ddpm_coef{};
  if (!a.rng) return ew_launch_v<1>(ddpm_step_body<false>{a.x, a.eps, a.noise_p, a.noise_q, a.orig, a.mask, cv, a.table, a.state, 0, 0, 0, 0, a.x_out}, a.n, s);
  PF_REQUIRE(aligned16({a.x, a.eps, a.x_out, a.orig, a.mask}), "ddpm_step_rng: tensors must be 16-byte aligned");
  return ew_launch_v<4>(ddpm_step_body<true>{a.x, a.eps, nullptr, nullptr, a.orig, a.mask, cv, a.table, a.state, a.seed, a.draw_q, a.draw_p, a.elem_offset, a.x_out},
                        a.n, s);
}
int launch_ddim_step(const pf_ddim_step_args& a, hipStream_t s) {
  if (int rc = check_step_args(a, !a.orig || (a.mask && a.orig_noise), a.noise != nullptr, "ddim_step")) return rc;
  const pf_ddim_coef cv = a.coef ? *a.coef : pf_ddim_coef{};
  if (!a.rng) return ew_launch_v<1>(ddim_step_body<false>{a.x, a.eps, a.noise, a.orig, a.orig_noise, a.mask, cv, a.table, a.state, 0, 0, 0, a.x_out}, a.n, s);
  PF_REQUIRE(aligned16({a.x, a.eps, a.x_out, a.orig, a.orig_noise, a.mask}), "ddim_step_rng: tensors must be 16-byte aligned");
  return ew_launch_v<4>(ddim_step_body<true>{a.x, a.eps, nullptr, a.orig, a.orig_noise, a.mask, cv, a.table, a.state, a.seed, a.draw, a.elem_offset, a.x_out}, a.n, s);
}

// RePaint re-noise between inner repeats: out = a*x + b*y, each product rounded, then the sum
struct axpby_body {
  const float* __restrict__ x; const float* __restrict__ y; float a, b; float* __restrict__ out;
  __device__ __forceinline__ void begin() {}
  template <int V>
  __device__ __forceinline__ void at(size_t i) const { out[i] = add_rn(mul_rn(a, x[i]), mul_rn(b, y[i])); }
};
int launch_axpby(const float* x, const float* y, float a, float b, float* out, size_t n, hipStream_t s) {
  PF_REQUIRE(x && y && out && n > 0, "axpby: bad arguments");
  return ew_launch_v<1>(axpby_body{x, y, a, b, out}, n, s);
}

// ---- DPM-Solver++(2M) (include/pfhip.h): one element of the update on VALUES.  Every operation is individually rounded (noise.h), so both
// widths give the same bits.  Roundings on the way to the result, which the tests' error budget counts:
//   x0:           mul (s1m*e), sub, div                                  3   (what x0_out receives)
//   first order:  those 3 + mul (c_x*x), mul (c_0*x0), add               6
//   second order: those 6 + mul (c_1*x0_prev), add                       8
//   known region: + mul, mul, add (the noised original), sub (1 - m), mul, mul, add (the blend)      + 7
// `second` is uniform over the launch (c_1 != 0); x0p is a VALUE the caller loaded only when `second` holds.
__device__ __forceinline__ float dpm_x0(float xv, float e, const pf_dpm_coef& c) { return __fdiv_rn(sub_rn(xv, mul_rn(c.s1m, e)), c.sqrt_a); }
// (the update in its two halves, which the stochastic form below puts its noise term between)
__device__ __forceinline__ float dpm_solve_v(float xv, float x0, bool second, float x0p, const pf_dpm_coef& c) {
  float xp = add_rn(mul_rn(c.c_x, xv), mul_rn(c.c_0, x0));
  if (second) xp = add_rn(xp, mul_rn(c.c_1, x0p));
  return xp;
}
__device__ __forceinline__ float dpm_blend_v(float xp, float ov, float onv, float m, const pf_dpm_coef& c) {
  const float ot = add_rn(mul_rn(c.q_sqrt_a, ov), mul_rn(c.q_s1m, onv));
  return add_rn(mul_rn(ot, m), mul_rn(xp, sub_rn(1.0f, m)));
}
__device__ __forceinline__ float dpm_update_v(float xv, float x0, bool second, float x0p, bool has_orig, float ov, float onv, float m,
                                              const pf_dpm_coef& c) {
  const float xp = dpm_solve_v(xv, x0, second, x0p, c);
  return has_orig ? dpm_blend_v(xp, ov, onv, m, c) : xp;
}
// x / out and x0p / x0o carry no __restrict__: x_out may alias x and x0_out may alias x0_prev (a lane reads group g of both before it
// writes group g of either, and no other lane touches group g)
struct dpm_step_body {
  const float* x; const float* __restrict__ eps; const float* x0p; float* x0o; const float* __restrict__ orig; const float* __restrict__ on;
  const float* __restrict__ mask; pf_dpm_coef c; const pf_dpm_coef* __restrict__ table; const pf_step_state* __restrict__ st; float* out;
  bool second;
  __device__ __forceinline__ void begin() {
    c = coef_of(c, table, st);
    second = c.c_1 != 0.f && x0p != nullptr;      // c_1 == 0: the history is not read at all (it may be uninitialised)
  }
  template <int V>
  __device__ __forceinline__ void at(size_t g) const {
    const size_t i = g * V;
    float xv[V], ev[V], pv[V] = {}, ov[V] = {}, nv[V] = {}, mv[V] = {}, o[V], z[V];
    ew_ld<V>(x + i, xv); ew_ld<V>(eps + i, ev);
    if (second) ew_ld<V>(x0p + i, pv);
    if (orig) { ew_ld<V>(orig + i, ov); ew_ld<V>(on + i, nv); ew_ld<V>(mask + i, mv); }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      z[j] = dpm_x0(xv[j], ev[j], c);
      o[j] = dpm_update_v(xv[j], z[j], second, pv[j], orig != nullptr, ov[j], nv[j], mv[j], c);
    }
    if (x0o) ew_st<V>(x0o + i, z);
    ew_st<V>(out + i, o);
  }
};
int launch_dpm_step(const pf_dpm_step_args& a, hipStream_t s) {
  PF_REQUIRE(a.x && a.eps && a.x_out && a.n > 0, "dpm_step: bad arguments (x, eps and x_out must be set, n > 0)");
  PF_REQUIRE((a.orig && a.orig_noise && a.mask) || (!a.orig && !a.orig_noise && !a.mask),
             "dpm_step: the known region needs orig, orig_noise and mask - all three or none");
  if (int rc = check_coef_source(a, "dpm_step")) return rc;
  PF_REQUIRE(!a.coef || a.coef->c_1 == 0.f || a.x0_prev, "dpm_step: a second-order step (c_1 != 0) needs x0_prev");
  const pf_dpm_coef cv = a.coef ? *a.coef : pf_dpm_coef{};
  const bool vec = aligned16({a.x, a.eps, a.x_out, a.x0_prev, a.x0_out, a.orig, a.orig_noise, a.mask}) && a.n % 4 == 0;
  return ew_launch(vec, dpm_step_body{a.x, a.eps, a.x0_prev, a.x0_out, a.orig, a.orig_noise, a.mask, cv, a.table, a.state, a.x_out, false}, a.n, s);
}

// ---- the stochastic form, SDE-DPM-Solver++(2M) (include/pfhip.h: pf_dpm_sde_step): the update above with sigma_n*z added BEFORE the
// known-region blend, on dpm_x0 / dpm_solve_v / dpm_blend_v - the same individually rounded operations in the same order, so a row with
// sigma_n == 0 gives the bits of pf_dpm_step.  Roundings on the way to the result:
//   x0:           mul (s1m*e), sub, div                                  3   (what x0_out receives)
//   first order:  those 3 + mul (c_x*x), mul (c_0*x0), add               6
//   second order: those 6 + mul (c_1*x0_prev), add                       8
//   noise term:   + mul (sigma_n*z), add                                 + 2
//   known region: + mul, mul, add (the noised original), sub (1 - m), mul, mul, add (the blend)      + 7
// `second` (c_1 != 0) and `noisy` (sigma_n != 0) are uniform over the launch and are selects: without them the history / the noise tensor
// is not read and no Philox call is made.  RNG as in ddim_step_body: a lane owns the four elements of one Philox group.
template <bool RNG>
struct dpm_sde_step_body {
  const float* x; const float* __restrict__ eps; const float* x0p; float* x0o; const float* __restrict__ noise;
  const float* __restrict__ orig; const float* __restrict__ on; const float* __restrict__ mask;
  pf_dpm_sde_coef c; const pf_dpm_sde_coef* __restrict__ table; const pf_step_state* __restrict__ st;
  uint64_t seed, draw, off; float* out;
  pf_dpm_coef b; bool second, noisy;
  __device__ __forceinline__ void begin() {
    c = coef_of(c, table, st);
    b = pf_dpm_coef{c.s1m, c.sqrt_a, c.c_x, c.c_0, c.c_1, c.q_sqrt_a, c.q_s1m};
    second = c.c_1 != 0.f && x0p != nullptr;
    noisy = c.sigma_n != 0.f && (RNG || noise != nullptr);
    if (RNG && st) draw = st->draws;
  }
  template <int V>
  __device__ __forceinline__ void at(size_t g) const {
    static_assert(!RNG || V == 4, "one Philox call yields the four normals of a 16-byte group");
    const size_t i = g * V;
    float xv[V], ev[V], pv[V] = {}, nz[V] = {}, ov[V] = {}, nv[V] = {}, mv[V] = {}, o[V], z[V];
    if (noisy) {
      if constexpr (RNG) philox_normal4((off >> 2) + g, draw, seed, nz);
      else ew_ld<V>(noise + i, nz);
    }
    ew_ld<V>(x + i, xv); ew_ld<V>(eps + i, ev);
    if (second) ew_ld<V>(x0p + i, pv);
    if (orig) { ew_ld<V>(orig + i, ov); ew_ld<V>(on + i, nv); ew_ld<V>(mask + i, mv); }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      z[j] = dpm_x0(xv[j], ev[j], b);
      float xp = dpm_solve_v(xv[j], z[j], second, pv[j], b);
      if (noisy) xp = add_rn(xp, mul_rn(c.sigma_n, nz[j]));
      o[j] = orig ? dpm_blend_v(xp, ov[j], nv[j], mv[j], b) : xp;
    }
    if (x0o) ew_st<V>(x0o + i, z);
    ew_st<V>(out + i, o);
  }
};
int launch_dpm_sde_step(const pf_dpm_sde_step_args& a, hipStream_t s) {
  PF_REQUIRE(a.x && a.eps && a.x_out && a.n > 0, "dpm_sde_step: bad arguments (x, eps and x_out must be set, n > 0)");
  PF_REQUIRE((a.orig && a.orig_noise && a.mask) || (!a.orig && !a.orig_noise && !a.mask),
             "dpm_sde_step: the known region needs orig, orig_noise and mask - all three or none");
  if (int rc = check_coef_source(a, "dpm_sde_step")) return rc;
  PF_REQUIRE(!(a.rng && a.noise), "dpm_sde_step_rng: the noise is drawn in the kernel, the noise tensor must be NULL");
  PF_REQUIRE(!a.coef || a.coef->c_1 == 0.f || a.x0_prev, "dpm_sde_step: a second-order step (c_1 != 0) needs x0_prev");
  PF_REQUIRE(!a.coef || a.coef->sigma_n == 0.f || a.noise || a.rng, "dpm_sde_step: a step with noise (sigma_n != 0) needs a noise tensor or rng");
  const pf_dpm_sde_coef cv = a.coef ? *a.coef : pf_dpm_sde_coef{};
  const bool al = aligned16({a.x, a.eps, a.x_out, a.x0_prev, a.x0_out, a.noise, a.orig, a.orig_noise, a.mask});
  if (!a.rng)
    return ew_launch(al && a.n % 4 == 0, dpm_sde_step_body<false>{a.x, a.eps, a.x0_prev, a.x0_out, a.noise, a.orig, a.orig_noise, a.mask, cv, a.table,
                                                                   a.state, 0, 0, 0, a.x_out, pf_dpm_coef{}, false, false}, a.n, s);
  PF_REQUIRE(a.n % 4 == 0 && a.elem_offset % 4 == 0, "dpm_sde_step_rng: n and elem_offset must be multiples of 4 (one Philox call yields four normals)");
  PF_REQUIRE(al, "dpm_sde_step_rng: tensors must be 16-byte aligned");
  return ew_launch_v<4>(dpm_sde_step_body<true>{a.x, a.eps, a.x0_prev, a.x0_out, nullptr, a.orig, a.orig_noise, a.mask, cv, a.table, a.state, a.seed,
                                                 a.draw, a.elem_offset, a.x_out, pf_dpm_coef{}, false, false}, a.n, s);
}

// ---- device-resident step state: what changes from one reverse step to the next lives in device memory, so a captured
// step (hipGraph) can be replayed unchanged
__global__ void step_state_set_kernel(pf_step_state* st, long long index, unsigned long long draws) { st->index = index; st->draws = draws; }
__global__ void step_begin_kernel(const pf_step_state* __restrict__ st, const int* __restrict__ time_steps, long long* __restrict__ t_out, int batch) {
  const long long t = time_steps ? (long long)time_steps[st->index] : (long long)st->index;
  for (int i = threadIdx.x; i < batch; i += blockDim.x) t_out[i] = t;
}
__global__ void step_end_kernel(pf_step_state* st, int draws_used) { st->index -= 1; st->draws += (unsigned long long)draws_used; }
// the upward walk's counterpart of step_end_kernel: index += delta; draws += draws_used
__global__ void step_advance_kernel(pf_step_state* st, long long delta, int draws_used) { st->index += delta; st->draws += (unsigned long long)draws_used; }
int launch_step_state_set(pf_step_state* st, int64_t index, uint64_t draws, hipStream_t s) {
  PF_REQUIRE(st, "step_state_set: null state");
  hipLaunchKernelGGL(step_state_set_kernel, dim3(1), dim3(1), 0, s, st, (long long)index, (unsigned long long)draws);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}
int launch_step_begin(const pf_step_state* st, const int* time_steps, int64_t* t_out, int batch, hipStream_t s) {
  PF_REQUIRE(st && t_out && batch > 0, "step_begin: bad arguments");
  hipLaunchKernelGGL(step_begin_kernel, dim3(1), dim3(64), 0, s, st, time_steps, reinterpret_cast<long long*>(t_out), batch);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}
int launch_step_end(pf_step_state* st, int draws_used, hipStream_t s) {
  PF_REQUIRE(st && draws_used >= 0, "step_end: bad arguments");
  hipLaunchKernelGGL(step_end_kernel, dim3(1), dim3(1), 0, s, st, draws_used);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}
int launch_step_advance(pf_step_state* st, int64_t delta, int draws_used, hipStream_t s) {
  PF_REQUIRE(st && draws_used >= 0, "step_advance: bad arguments");
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, s, st, (long long)delta, draws_used);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// ------------------------------------------------------------------ counter-based Gaussian noise (Philox4x32-10 + Box-Muller: noise.h)
// (its own loop: the groups are those of the GLOBAL tensor, so the first and the last one may lie partly outside [off, off + n))
__device__ __forceinline__ void randn_body(float* __restrict__ out, size_t n, uint64_t seed, uint64_t sid, uint64_t off) {
  const uint64_t g0 = off >> 2, g1 = (off + n + 3) >> 2;
  for (uint64_t g = g0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < g1; g += (uint64_t)gridDim.x * blockDim.x) {
    float z[4];
    philox_normal4(g, sid, seed, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t e = g * 4 + j;
      if (e >= off && e < off + n) out[e - off] = z[j];
    }
  }
}
__global__ void randn_kernel(float* __restrict__ out, size_t n, uint64_t seed, uint64_t sid, uint64_t off) { randn_body(out, n, seed, sid, off); }
// draw index = device-resident counter + slot (the position of this draw inside the step)
__global__ void randn_dev_kernel(float* __restrict__ out, size_t n, uint64_t seed, const pf_step_state* __restrict__ st, int slot, uint64_t off) {
  randn_body(out, n, seed, st->draws + (uint64_t)slot, off);
}
int launch_randn_dev(float* out, size_t n, uint64_t seed, const pf_step_state* st, int slot, uint64_t elem_offset, hipStream_t s) {
  PF_REQUIRE(out && st && n > 0 && slot >= 0, "randn_dev: bad arguments");
  hipLaunchKernelGGL(randn_dev_kernel, ew_grid(n / 4 + 1), dim3(256), 0, s, out, n, seed, st, slot, elem_offset);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}
int launch_randn(float* out, size_t n, uint64_t seed, uint64_t stream_id, uint64_t elem_offset, hipStream_t s) {
  PF_REQUIRE(out && n > 0, "randn: bad arguments");
  hipLaunchKernelGGL(randn_kernel, ew_grid(n / 4 + 1), dim3(256), 0, s, out, n, seed, stream_id, elem_offset);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// ---- exact DDIM inversion (include/pfhip.h: pf_invert_step; DESIGN.md 3, "Exact DDIM inversion"): one iterate of one UPWARD step,
//   x_out = c_y*y + c_e*eps          mul, mul, add - 3 roundings, which the tests' budget counts on |c_y*y| + |c_e*eps|
// Every operation is individually rounded (noise.h), so the map and the row kernel below give the same bits at either width.  y is never
// written and never aliases x_out (refused); eps, x_iter and out carry no __restrict__: x_out may alias x_iter (a lane reads its elements
// before it writes them, and no other lane touches them).
__device__ __forceinline__ float invert_update_v(float yv, float e, const pf_invert_coef& c) { return add_rn(mul_rn(c.c_y, yv), mul_rn(c.c_e, e)); }
struct invert_step_body {
  const float* __restrict__ y; const float* eps; pf_invert_coef c; const pf_invert_coef* __restrict__ table; const pf_step_state* __restrict__ st;
  float* out;
  __device__ __forceinline__ void begin() { c = coef_of(c, table, st); }
  template <int V>
  __device__ __forceinline__ void at(size_t g) const {
    const size_t i = g * V;
    float yv[V], ev[V], o[V];
    ew_ld<V>(y + i, yv); ew_ld<V>(eps + i, ev);
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = invert_update_v(yv[j], ev[j], c);
    ew_st<V>(out + i, o);
  }
};
// With the residual: the row reduction of elementwise.h with two sums.  A lane updates its groups and adds (x_out - x_iter)^2 and x_out^2
// in element order - the difference in float32, the squares (exact in float64) and the sums in float64.  A row's two sums do not depend on
// the rows around it.  One partial pair per workgroup; invert_resid_finish_kernel adds a row's pairs in index order.
template <bool VEC>
__global__ __launch_bounds__(kRowThreads) void invert_step_resid_kernel(const float* __restrict__ y, const float* eps, const float* xi,
                                                                       pf_invert_coef cv, const pf_invert_coef* __restrict__ table,
                                                                       const pf_step_state* __restrict__ st, float* out,
                                                                       double* __restrict__ partial, size_t row_elems, unsigned chunks) {
  const pf_invert_coef c = coef_of(cv, table, st);
  const unsigned row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks;
  const size_t base = (size_t)row * row_elems;
  double acc[2] = {0.0, 0.0};
#pragma unroll
  for (int k = 0; k < kRowGroups; ++k) {
    const size_t e = row_group_elem(chunk, k);
    if (e < row_elems) {
      const f32x4 yv = load4<VEC>(y + base, e, row_elems), ev = load4<VEC>(eps + base, e, row_elems);
      const f32x4 pv = xi ? load4<VEC>(xi + base, e, row_elems) : yv;     // no previous iterate: the iteration starts from y
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = invert_update_v(yv[j], ev[j], c);
        if (VEC || e + j < row_elems) {
          const double d = (double)sub_rn(o[j], pv[j]), q = (double)o[j];
          acc[0] += d * d;
          acc[1] += q * q;
        }
      }
      store4<VEC>(out + base, e, row_elems, o);
    }
  }
  row_reduce_store(acc, partial, row, chunks, chunk);
}
// one lane per row: the row's partial pairs in index order into slot `slot` of resid [n_slots][rows][2]; with a step state the slot is
// state->index * iters + k.  A slot outside the table is not written (memory safety only: the host refuses the ones it can see).
__global__ void invert_resid_finish_kernel(const double* __restrict__ partial, double* __restrict__ resid, int rows, unsigned chunks,
                                           const pf_step_state* __restrict__ st, int iters, int k, long long slot, long long n_slots) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  if (st) slot = (long long)st->index * iters + k;
  if (slot < 0 || slot >= n_slots) return;
  double sum[2];
  row_partials_sum(partial, row, chunks, sum);
  double* dst = resid + ((size_t)slot * rows + row) * 2;
  dst[0] = sum[0];
  dst[1] = sum[1];
}
size_t invert_step_workspace_bytes(int rows, size_t row_elems) {
  if (rows <= 0 || row_elems == 0) return 0;
  return (size_t)rows * chunks_of(row_elems, PF_MSE_CHUNK) * 2 * sizeof(double);
}
int launch_invert_step(const pf_invert_step_args& a, hipStream_t s) {
  PF_REQUIRE(a.y && a.eps && a.x_out && a.rows > 0 && a.row_elems > 0, "invert_step: bad arguments (y, eps and x_out must be set, rows and row_elems > 0)");
  if (int rc = check_coef_source(a, "invert_step")) return rc;
  const size_t n = (size_t)a.rows * a.row_elems, bytes = n * sizeof(float);
  PF_REQUIRE(!ranges_overlap(a.y, bytes, a.x_out, bytes), "invert_step: y aliases x_out (y is the fixed lower state of every iterate)");
  PF_REQUIRE(!ranges_overlap(a.eps, bytes, a.x_out, bytes), "invert_step: eps aliases x_out");
  PF_REQUIRE(!a.x_iter || a.x_iter == a.x_out || !ranges_overlap(a.x_iter, bytes, a.x_out, bytes), "invert_step: x_iter overlaps x_out without being it");
  const pf_invert_coef cv = a.coef ? *a.coef : pf_invert_coef{};
  const bool vec = aligned16({a.y, a.eps, a.x_out, a.x_iter}) && a.row_elems % 4 == 0;
  if (!a.resid) return ew_launch(vec, invert_step_body{a.y, a.eps, cv, a.table, a.state, a.x_out}, n, s);   // one launch, no workspace (one that is given is not touched)
  const size_t chunks = chunks_of(a.row_elems, PF_MSE_CHUNK), need = invert_step_workspace_bytes(a.rows, a.row_elems);
  PF_REQUIRE(chunks * (size_t)a.rows < (1ull << 31), "invert_step: %d rows of %zu elements are more workgroups than one launch holds", a.rows, a.row_elems);
  PF_REQUIRE(a.workspace, "invert_step: resid without a workspace (pf_invert_step_workspace_bytes)");
  PF_REQUIRE(a.workspace_bytes >= need, "invert_step: workspace of %zu bytes required, got %zu", need, a.workspace_bytes);
  PF_REQUIRE(((uintptr_t)a.workspace & 7) == 0 && ((uintptr_t)a.resid & 7) == 0, "invert_step: workspace and resid must be 8-byte aligned");
  PF_REQUIRE(a.n_slots > 0, "invert_step: resid needs n_slots > 0, the slots the table holds");
  if (a.state) {
    PF_REQUIRE(a.iters >= 1 && a.k >= 0 && a.k < a.iters, "invert_step: iterate k = %d outside [0, iters = %d)", a.k, a.iters);
  } else {
    PF_REQUIRE(a.slot >= 0 && a.slot < a.n_slots, "invert_step: slot %lld outside [0, n_slots = %lld)", (long long)a.slot, (long long)a.n_slots);
  }
  const dim3 grid((unsigned)(chunks * a.rows)), block(kRowThreads);
  double* partial = reinterpret_cast<double*>(a.workspace);
  if (vec)
    hipLaunchKernelGGL(invert_step_resid_kernel<true>, grid, block, 0, s, a.y, a.eps, a.x_iter, cv, a.table, a.state, a.x_out, partial, a.row_elems, (unsigned)chunks);
  else
    hipLaunchKernelGGL(invert_step_resid_kernel<false>, grid, block, 0, s, a.y, a.eps, a.x_iter, cv, a.table, a.state, a.x_out, partial, a.row_elems, (unsigned)chunks);
  PF_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(invert_resid_finish_kernel, dim3((unsigned)cdiv(a.rows, 64)), dim3(64), 0, s, partial, a.resid, a.rows, (unsigned)chunks, a.state, a.iters,
                     a.k, (long long)a.slot, (long long)a.n_slots);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// ---- a path between two noises (include/pfhip.h: pf_slerp_rows; DESIGN.md 3, "Morph"): per row, `frames` points on the great circle from
// a to b, out[k] = w0[k]*a + w1[k]*b.  Two launches, a workgroup = (row, chunk of PF_MSE_CHUNK):
//   reduce   the row reduction of elementwise.h with three sums, a*a, a*b, b*b - the products exact in float64; one partial triple per
//            workgroup, no atomics
//   combine  EVERY workgroup of a row adds the row's triples in chunk order (the same three doubles in each of them), lane k < frames forms
//            frame k's two weights in float64 and rounds each to float once; then a and b are read once and all frames written.
// Mode lerp runs the combine launch alone with (1 - t, t).  VEC and the element-by-element form do the same operations: the same bits.
struct slerp_fracs { double t[PF_SLERP_MAX_FRAMES]; };      // by value in the launch: the host array is copied at the call
template <bool VEC>
__global__ __launch_bounds__(kRowThreads) void slerp_reduce_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                  double* __restrict__ partial, size_t row_elems, unsigned chunks) {
  const unsigned row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks;
  const size_t base = (size_t)row * row_elems;
  double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < kRowGroups; ++k) {
    const size_t e = row_group_elem(chunk, k);
    if (e < row_elems) {
      const f32x4 av = load4<VEC>(a + base, e, row_elems), bv = load4<VEC>(b + base, e, row_elems);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (VEC || e + j < row_elems) {
          const double p = (double)av[j], q = (double)bv[j];
          acc[0] += p * p;
          acc[1] += p * q;
          acc[2] += q * q;
        }
    }
  }
  row_reduce_store(acc, partial, row, chunks, chunk);
}
// Lerp weights (1 - t, t) stand in for the slerp weights when aa == 0, bb == 0 or 1 - |c| < 2^-20: parallel rows, where the two agree to
// O(theta^2) and sin(theta) has lost its digits, and antiparallel rows, where the great circle is not defined (the path then goes
// through the origin).  A frame at t == 0 / t == 1 is a COPY of a / b, by a select: bit-identical, a negative zero included.
template <bool VEC>
__global__ __launch_bounds__(kRowThreads) void slerp_combine_kernel(const float* __restrict__ a, const float* __restrict__ b, slerp_fracs fr,
                                                                   int frames, int mode, const double* __restrict__ partial,
                                                                   float* __restrict__ out, double* __restrict__ stats,
                                                                   float* __restrict__ weights, int rows, size_t row_elems, unsigned chunks) {
  __shared__ float w_sh[PF_SLERP_MAX_FRAMES][2];
  __shared__ int sel_sh[PF_SLERP_MAX_FRAMES];
  const unsigned row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks;
  if ((int)threadIdx.x < frames) {
    const double t = fr.t[threadIdx.x];
    double w0 = 1.0 - t, w1 = t;
    if (mode == 0) {
      double sum[3];                       // aa, ab, bb
      row_partials_sum(partial, row, chunks, sum);
      const double c = sum[1] / sqrt(sum[0] * sum[2]);
      if (!(sum[0] == 0.0 || sum[2] == 0.0 || 1.0 - fabs(c) < 0x1p-20)) {
        const double theta = acos(c), sn = sin(theta);
        w0 = sin((1.0 - t) * theta) / sn;
        w1 = sin(t * theta) / sn;
      }
      if (chunk == 0 && threadIdx.x == 0 && stats) {
#pragma unroll
        for (int q = 0; q < 3; ++q) stats[(size_t)row * 3 + q] = sum[q];
      }
    }
    const float f0 = (float)w0, f1 = (float)w1;
    w_sh[threadIdx.x][0] = f0;
    w_sh[threadIdx.x][1] = f1;
    sel_sh[threadIdx.x] = t == 0.0 ? 1 : t == 1.0 ? 2 : 0;
    if (chunk == 0 && weights) {
      weights[((size_t)threadIdx.x * rows + row) * 2 + 0] = f0;
      weights[((size_t)threadIdx.x * rows + row) * 2 + 1] = f1;
    }
  }
  __syncthreads();
  const size_t base = (size_t)row * row_elems, frame_elems = (size_t)rows * row_elems;
#pragma unroll
  for (int g = 0; g < kRowGroups; ++g) {
    const size_t e = row_group_elem(chunk, g);
    if (e < row_elems) {
      const f32x4 av = load4<VEC>(a + base, e, row_elems), bv = load4<VEC>(b + base, e, row_elems);
      for (int k = 0; k < frames; ++k) {
        const float w0 = w_sh[k][0], w1 = w_sh[k][1];
        const int sel = sel_sh[k];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = add_rn(mul_rn(w0, av[j]), mul_rn(w1, bv[j]));
          o[j] = sel == 1 ? av[j] : sel == 2 ? bv[j] : v;
        }
        store4<VEC>(out + (size_t)k * frame_elems + base, e, row_elems, o);
      }
    }
  }
}
size_t slerp_rows_workspace_bytes(int rows, size_t row_elems) {
  if (rows <= 0 || row_elems == 0) return 0;
  return (size_t)rows * chunks_of(row_elems, PF_MSE_CHUNK) * 3 * sizeof(double);
}
int launch_slerp_rows(const pf_slerp_args& a, hipStream_t s) {
  PF_REQUIRE(a.a && a.b && a.out && a.t, "slerp_rows: null a, b, out or t");
  PF_REQUIRE(a.rows > 0 && a.row_elems > 0, "slerp_rows: %d rows of %zu elements", a.rows, a.row_elems);
  PF_REQUIRE(a.frames >= 1 && a.frames <= PF_SLERP_MAX_FRAMES, "slerp_rows: %d frames outside [1, %d]", a.frames, PF_SLERP_MAX_FRAMES);
  PF_REQUIRE(a.mode == 0 || a.mode == 1, "slerp_rows: mode %d, expected 0 (slerp) or 1 (lerp)", a.mode);
  slerp_fracs fr = {};
  for (int k = 0; k < a.frames; ++k) {
    PF_REQUIRE(a.t[k] >= 0.0 && a.t[k] <= 1.0, "slerp_rows: fraction t[%d] = %g outside [0, 1]", k, a.t[k]);     // (a NaN fails both)
    fr.t[k] = a.t[k];
  }
  const size_t n = (size_t)a.rows * a.row_elems, bytes = n * sizeof(float);
  PF_REQUIRE(!ranges_overlap(a.out, bytes * a.frames, a.a, bytes), "slerp_rows: out overlaps a");
  PF_REQUIRE(!ranges_overlap(a.out, bytes * a.frames, a.b, bytes), "slerp_rows: out overlaps b");
  PF_REQUIRE(((uintptr_t)a.stats & 7) == 0, "slerp_rows: stats must be 8-byte aligned");
  const size_t chunks = chunks_of(a.row_elems, PF_MSE_CHUNK), need = slerp_rows_workspace_bytes(a.rows, a.row_elems);
  PF_REQUIRE(chunks * (size_t)a.rows < (1ull << 31), "slerp_rows: %d rows of %zu elements are more workgroups than one launch holds", a.rows, a.row_elems);
  if (a.mode == 0) {
    PF_REQUIRE(a.workspace, "slerp_rows: mode slerp without a workspace (pf_slerp_rows_workspace_bytes)");
    PF_REQUIRE(a.workspace_bytes >= need, "slerp_rows: workspace of %zu bytes required, got %zu", need, a.workspace_bytes);
    PF_REQUIRE(((uintptr_t)a.workspace & 7) == 0, "slerp_rows: workspace must be 8-byte aligned");
  }
  const bool vec = aligned16({a.a, a.b, a.out}) && a.row_elems % 4 == 0;
  const dim3 grid((unsigned)(chunks * a.rows)), block(kRowThreads);
  double* partial = a.mode == 0 ? reinterpret_cast<double*>(a.workspace) : nullptr;
  if (a.mode == 0) {
    if (vec)
      hipLaunchKernelGGL(slerp_reduce_kernel<true>, grid, block, 0, s, a.a, a.b, partial, a.row_elems, (unsigned)chunks);
    else
      hipLaunchKernelGGL(slerp_reduce_kernel<false>, grid, block, 0, s, a.a, a.b, partial, a.row_elems, (unsigned)chunks);
    PF_CHECK_HIP(hipGetLastError());
  }
  if (vec)
    hipLaunchKernelGGL(slerp_combine_kernel<true>, grid, block, 0, s, a.a, a.b, fr, a.frames, a.mode, partial, a.out, a.stats, a.weights, a.rows,
                       a.row_elems, (unsigned)chunks);
  else
    hipLaunchKernelGGL(slerp_combine_kernel<false>, grid, block, 0, s, a.a, a.b, fr, a.frames, a.mode, partial, a.out, a.stats, a.weights, a.rows,
                       a.row_elems, (unsigned)chunks);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

}  // namespace pf
