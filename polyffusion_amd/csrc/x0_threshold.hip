// x0_threshold.hip - bound the predicted clean image inside a reverse step (gfx950; include/pfhip.h: pf_x0_threshold; DESIGN.md 3,
// "Clipping and dynamic thresholding").  Per row the kernel turns eps into the eps' whose predicted x0 is the clipped (Ho et al. 2020,
// clip_denoised) or dynamically thresholded (Saharia et al. 2022, section 2.3) one; untouched elements come through bit for bit.
// The dynamic mode needs an exact order statistic of |x0 - c| per row: a radix select over the uint32 bit patterns (|u| >= 0, so the order
// of the patterns is the order of the values; -0 counts as +0, NaN sorts above inf), most significant digit first, kDigits = 4 digits of
// kDigitBits = 8 bits, 256 bins.  Histograms are integer counts: order-free, so LDS atomics are exact.  Two forms, the same bits:
//   resident   row_elems <= PF_X0T_RESIDENT_MAX: ONE launch, one workgroup of 1024 lanes per row.  x and eps are read once into
//              registers (8 groups of 16 bytes per lane each), the keys staged in dynamic LDS (4 bytes per element, lane-linear: a lane
//              reads back its own 16-byte groups), the four histogram passes, the search for the next key above a_(k) and the count of
//              changed elements run on LDS, and eps' is written once from the registers.
//   streamed   any row_elems: workgroup = (row, chunk of PF_MSE_CHUNK), 256 lanes.  kDigits histogram launches - launch d first sums
//              the per-chunk histograms of digit d - 1 in chunk order, finds the bin that holds rank k, extends the prefix, and counts
//              digit d of its chunk's keys under that prefix into workspace; the last one also keeps the chunk's smallest key above the
//              24-bit prefix - then one apply launch, and with `stats` one launch that adds the per-chunk change counts in chunk order:
//              kDigits + 1 launches (+ 1 with stats) in mode dynamic, 1 (+ 1 with stats) in mode clip, whatever the data.  No global atomics.
// Both forms call the same device functions for the element arithmetic (individually rounded, noise.h) and for the float64 decision of a
// row (x0t_decide), and a 16-byte and an element-wise access do the same operations: the same bits everywhere.
#include <cmath>
#include "elementwise.h"
#include "x0_predict.h"

namespace pf {

namespace {

constexpr int kDigitBits = 8, kDigits = 32 / kDigitBits, kBins = 1 << kDigitBits;
constexpr int kResThreads = 1024;
constexpr int kResGroups = PF_X0T_RESIDENT_MAX / 4 / kResThreads;      // 16-byte groups of a row per lane in the resident form
static_assert(PF_X0T_RESIDENT_MAX == 4 * kResThreads * kResGroups, "PF_X0T_RESIDENT_MAX must be a whole number of 16-byte groups per lane");
static_assert(kBins == kRowThreads, "one lane of a streamed workgroup per bin");
constexpr uint32_t kNoKey = 0xffffffffu;                               // no key has its sign bit set: "no key above"
enum { X0T_CLIP = 0, X0T_DYNAMIC = 1 };
enum { ROW_COPY = 0, ROW_CLIP = 1, ROW_SCALE = 2 };

struct x0t_params {                 // what every kernel of a call gets, by value
  const float* x; size_t x_row_stride;
  const float* eps; float* eps_out;
  const int64_t* t; int32_t t_stride;
  const float* table; int32_t n_table;
  double* stats;
  double p, s_max;
  float lo, hi;
  int32_t mode;
  size_t row_elems;
  unsigned chunks;
  // streamed form: state [rows][kDigits][2] uint64 (prefix, remaining rank), hist [2][rows][chunks][kBins], min_above / changed [rows][chunks]
  unsigned long long* state; uint32_t* hist; uint32_t* min_above; uint32_t* changed;
  size_t hist_stride;               // elements of one of the two histogram buffers
};

struct x0t_coef { float cx, ce, kx, k0; };
struct x0t_row { float lo, hi, c, sf, w; int kind; };                  // how a row's x0 is bounded (x0t_decide)

__device__ __forceinline__ x0t_coef x0t_coef_of(const x0t_params& a, unsigned row) {
  const float* r = x0_table_row(a.t, a.t_stride, a.table, a.n_table, row);
  return x0t_coef{r[0], r[1], r[2], r[3]};
}
__device__ __forceinline__ float x0t_centre(float lo, float hi) { return (float)(((double)lo + (double)hi) / 2.0); }
__device__ __forceinline__ float x0t_x0(const x0t_coef& k, float x, float e) { return x0_of(k.cx, k.ce, x, e); }   // x0_predict.h: pf_x0_predict's too
__device__ __forceinline__ uint32_t x0t_key(const x0t_coef& k, float c, float x, float e) {
  return __float_as_uint(sub_rn(x0t_x0(k, x, e), c)) & 0x7fffffffu;
}
// one element: eps' and whether x0 changed.  Comparisons, not fminf / fmaxf: a NaN x0 stays NaN (and counts as changed: NaN != NaN)
__device__ __forceinline__ float x0t_apply(const x0t_coef& k, const x0t_row& R, float x, float e, unsigned& changed) {
  if (R.kind == ROW_COPY) return e;
  const float x0 = x0t_x0(k, x, e);
  float y;
  if (R.kind == ROW_CLIP) {
    y = x0 < R.lo ? R.lo : (x0 > R.hi ? R.hi : x0);
  } else {
    const float u = sub_rn(x0, R.c), v = u < -R.sf ? -R.sf : (u > R.sf ? R.sf : u);
    y = add_rn(R.c, mul_rn(v, R.w));
  }
  if (y == x0) return e;
  ++changed;
  return sub_rn(mul_rn(k.kx, x), mul_rn(k.k0, y));
}
// a float64 product that no later addition can be contracted with (noise.h: the pragma alone does not survive inlining)
__device__ __forceinline__ double dmul_rn(double a, double b) { double r; asm("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// rank of the quantile: pos = p * (n - 1), k = floor(pos), in float64
__device__ __forceinline__ unsigned long long x0t_rank(double p, size_t n, double& frac) {
  const double pos = dmul_rn(p, (double)(n - 1)), kf = floor(pos);
  frac = pos - kf;
  return (unsigned long long)kf;
}
// the float64 decision of a row from its two order statistics: q, s, w for stats and the row's rule.  Every operation individually rounded.
__device__ __forceinline__ x0t_row x0t_decide(const x0t_params& a, uint32_t key_k, uint32_t key_k1, double frac, double (&st)[3]) {
  x0t_row R{a.lo, a.hi, x0t_centre(a.lo, a.hi), 0.f, 1.f, ROW_CLIP};
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  st[0] = nan; st[1] = nan; st[2] = 1.0;
  if (a.mode == X0T_CLIP) return R;
  const double h = ((double)a.hi - (double)a.lo) / 2.0;
  const double ak = (double)__uint_as_float(key_k), ak1 = (double)__uint_as_float(key_k1);
  const double q = ak + dmul_rn(frac, ak1 - ak);
  st[0] = q;
  if (!isfinite(q)) { R.kind = ROW_COPY; return R; }       // a stated rule: no finite threshold, the row is left alone (s stays NaN in stats)
  const double cap = dmul_rn(a.s_max, h), s = fmin(fmax(q, h), cap);
  st[1] = s;
  if (s == h) return R;                                    // the clip mode's row, bit for bit
  R.w = (float)(h / s);
  R.sf = (float)s;
  R.kind = ROW_SCALE;
  st[2] = (double)R.w;
  return R;
}

// ---- the bin of rank k among kBins counts in LDS: wave 0, four bins per lane, an inclusive scan over the lanes.  res = {bin, count of the
// bin, count below it}; the caller puts a barrier before (the counts) and after (res).
template <class T>
__device__ __forceinline__ void x0t_select_bin(const T* tot, unsigned long long k, unsigned long long* res) {
  if (threadIdx.x >= 64) return;
  const int l = threadIdx.x;
  unsigned long long c[4], s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { c[j] = (unsigned long long)tot[4 * l + j]; s += c[j]; }
  unsigned long long incl = s;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned long long o = __shfl_up(incl, m, 64);
    if (l >= m) incl += o;
  }
  unsigned long long below = incl - s;
  if (below <= k && k < incl) {                            // exactly one lane, as k < the total
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (k < below + c[j]) { res[0] = 4 * l + j; res[1] = c[j]; res[2] = below; break; }
      below += c[j];
    }
  }
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m, 64));
  return v;
}
__device__ __forceinline__ int digit_shift(int d) { return 32 - kDigitBits * (d + 1); }
// whether `key` carries the digits 0 .. d - 1 of `prefix`
__device__ __forceinline__ bool under_prefix(uint32_t key, uint32_t prefix, int d) { return d == 0 || ((key ^ prefix) >> (32 - kDigitBits * d)) == 0; }

// ------------------------------------------------------------------------------------------------------------------- resident form
template <bool VEC>
__global__ __launch_bounds__(kResThreads) void x0t_resident_kernel(x0t_params a) {
  extern __shared__ uint32_t keys[];                       // [ceil(row_elems / 4) * 4], element order (dynamic mode only)
  __shared__ uint32_t hist[kBins];
  __shared__ unsigned long long sel[3];
  __shared__ uint32_t next_key, n_changed;
  __shared__ x0t_row row_sh;
  const unsigned row = blockIdx.x, tid = threadIdx.x;
  const size_t n = a.row_elems;
  const x0t_coef kf = x0t_coef_of(a, row);
  const float* xr = a.x + (size_t)row * a.x_row_stride;
  const float* er = a.eps + (size_t)row * n;
  f32x4 xv[kResGroups], ev[kResGroups];
#pragma unroll
  for (int g = 0; g < kResGroups; ++g) {
    const size_t e = 4 * ((size_t)g * kResThreads + tid);
    if (e < n) { xv[g] = load4<VEC>(xr, e, n); ev[g] = load4<VEC>(er, e, n); }
  }
  if (tid == 0) { next_key = kNoKey; n_changed = 0; }
  uint32_t key_k = 0, key_k1 = 0;
  double frac = 0.0;
  if (a.mode == X0T_DYNAMIC) {
    const float c = x0t_centre(a.lo, a.hi);
#pragma unroll
    for (int g = 0; g < kResGroups; ++g) {
      const size_t e = 4 * ((size_t)g * kResThreads + tid);
      if (e < n) {
        uint4 kk;
        kk.x = x0t_key(kf, c, xv[g][0], ev[g][0]); kk.y = x0t_key(kf, c, xv[g][1], ev[g][1]);
        kk.z = x0t_key(kf, c, xv[g][2], ev[g][2]); kk.w = x0t_key(kf, c, xv[g][3], ev[g][3]);
        *reinterpret_cast<uint4*>(keys + e) = kk;          // (elements at or past n hold the key of x = eps = 0 and are never counted)
      }
    }
    unsigned long long krem = x0t_rank(a.p, n, frac);
    const unsigned long long k_rank = krem;
    uint32_t prefix = 0;
    unsigned long long eq = 0;
    for (int d = 0; d < kDigits; ++d) {
      if (tid < kBins) hist[tid] = 0;
      __syncthreads();                                     // (the first one also orders the key stores before the reads)
      const int sh = digit_shift(d);
#pragma unroll 2                                           // (LDS reads, not the register arrays: a full unroll holds 32 more registers and spills)
      for (int g = 0; g < kResGroups; ++g) {
        const size_t e = 4 * ((size_t)g * kResThreads + tid);
        if (e < n) {
          const uint4 kk = *reinterpret_cast<const uint4*>(keys + e);
          const uint32_t kv[4] = {kk.x, kk.y, kk.z, kk.w};
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (e + j < n && under_prefix(kv[j], prefix, d)) atomicAdd(&hist[(kv[j] >> sh) & (kBins - 1)], 1u);
        }
      }
      __syncthreads();
      x0t_select_bin(hist, krem, sel);
      __syncthreads();
      prefix |= (uint32_t)sel[0] << sh;
      eq = sel[1];
      krem -= sel[2];
    }
    key_k = key_k1 = prefix;                               // krem: the rank inside the run of `eq` equal keys
    if (krem + 1 >= eq && k_rank + 1 < n) {                // the run ends at k: a_(k+1) is the smallest key above
      uint32_t mn = kNoKey;
#pragma unroll 2
      for (int g = 0; g < kResGroups; ++g) {
        const size_t e = 4 * ((size_t)g * kResThreads + tid);
        if (e < n) {
          const uint4 kk = *reinterpret_cast<const uint4*>(keys + e);
          const uint32_t kv[4] = {kk.x, kk.y, kk.z, kk.w};
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (e + j < n && kv[j] > key_k) mn = min(mn, kv[j]);
        }
      }
      mn = wave_min(mn);
      if ((tid & 63) == 0 && mn != kNoKey) atomicMin(&next_key, mn);
      __syncthreads();
      if (next_key != kNoKey) key_k1 = next_key;
    }
  }
  if (tid == 0) {
    double st[3];
    row_sh = x0t_decide(a, key_k, key_k1, frac, st);
    if (a.stats) { a.stats[(size_t)row * 4 + 0] = st[0]; a.stats[(size_t)row * 4 + 1] = st[1]; a.stats[(size_t)row * 4 + 2] = st[2]; }
  }
  __syncthreads();
  const x0t_row R = row_sh;
  float* outr = a.eps_out + (size_t)row * n;
  unsigned changed = 0;
#pragma unroll
  for (int g = 0; g < kResGroups; ++g) {
    const size_t e = 4 * ((size_t)g * kResThreads + tid);
    if (e < n) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned ch = 0;
        o[j] = x0t_apply(kf, R, xv[g][j], ev[g][j], ch);
        if (VEC || e + j < n) changed += ch;
      }
      store4<VEC>(outr, e, n, o);
    }
  }
  if (a.stats) {
    if (changed) atomicAdd(&n_changed, changed);
    __syncthreads();
    if (tid == 0) a.stats[(size_t)row * 4 + 3] = (double)n_changed;
  }
}

// ------------------------------------------------------------------------------------------------------------------- streamed form
// (prefix, remaining rank) before digit d of a row: from the state the launch of digit d - 1 left and that launch's histograms, summed in
// chunk order.  Every workgroup of the row computes the same pair; the caller's chunk-0 workgroup stores it for the next launch.
// Returns through `sel` the chosen bin's count as well (sel[1]) and leaves the summed histogram in tot[].
__device__ __forceinline__ void x0t_advance(const x0t_params& a, unsigned row, int d, unsigned long long* tot, unsigned long long* sel,
                                            uint32_t& prefix, unsigned long long& krem, double& frac) {
  krem = x0t_rank(a.p, a.row_elems, frac);
  prefix = 0;
  if (d == 0) return;
  if (d > 1) {
    const unsigned long long* st = a.state + ((size_t)row * kDigits + (d - 1)) * 2;
    prefix = (uint32_t)st[0];
    krem = st[1];
  }
  const uint32_t* h = a.hist + (size_t)((d - 1) & 1) * a.hist_stride + (size_t)row * a.chunks * kBins;
  unsigned long long s = 0;
  for (unsigned c = 0; c < a.chunks; ++c) s += h[(size_t)c * kBins + threadIdx.x];
  tot[threadIdx.x] = s;
  __syncthreads();
  x0t_select_bin(tot, krem, sel);
  __syncthreads();
  prefix |= (uint32_t)sel[0] << digit_shift(d - 1);
  krem -= sel[2];
}

template <bool VEC>
__global__ __launch_bounds__(kRowThreads) void x0t_hist_kernel(x0t_params a, int d) {
  __shared__ uint32_t hist[kBins];
  __shared__ unsigned long long tot[kBins], sel[3];
  __shared__ uint32_t mn_sh;
  const unsigned row = blockIdx.x / a.chunks, chunk = blockIdx.x - row * a.chunks, tid = threadIdx.x;
  const size_t n = a.row_elems;
  hist[tid] = 0;
  if (tid == 0) mn_sh = kNoKey;
  uint32_t prefix;
  unsigned long long krem;
  double frac;
  x0t_advance(a, row, d, tot, sel, prefix, krem, frac);
  if (d > 0 && chunk == 0 && tid == 0) {
    unsigned long long* st = a.state + ((size_t)row * kDigits + d) * 2;
    st[0] = prefix;
    st[1] = krem;
  }
  __syncthreads();
  const x0t_coef kf = x0t_coef_of(a, row);
  const float c = x0t_centre(a.lo, a.hi);
  const float* xr = a.x + (size_t)row * a.x_row_stride;
  const float* er = a.eps + (size_t)row * n;
  const int sh = digit_shift(d);
  uint32_t mn = kNoKey;
#pragma unroll
  for (int g = 0; g < kRowGroups; ++g) {
    const size_t e = row_group_elem(chunk, g);
    if (e < n) {
      const f32x4 xv = load4<VEC>(xr, e, n), ev = load4<VEC>(er, e, n);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (VEC || e + j < n) {
          const uint32_t key = x0t_key(kf, c, xv[j], ev[j]);
          if (under_prefix(key, prefix, d)) atomicAdd(&hist[(key >> sh) & (kBins - 1)], 1u);
          else if (d == kDigits - 1 && key > prefix) mn = min(mn, key);      // above the 24-bit prefix: a candidate for a_(k+1)
        }
    }
  }
  if (d == kDigits - 1) {
    mn = wave_min(mn);
    if ((tid & 63) == 0 && mn != kNoKey) atomicMin(&mn_sh, mn);
  }
  __syncthreads();
  a.hist[(size_t)(d & 1) * a.hist_stride + ((size_t)row * a.chunks + chunk) * kBins + tid] = hist[tid];
  if (d == kDigits - 1 && tid == 0) a.min_above[(size_t)row * a.chunks + chunk] = mn_sh;
}

template <bool VEC>
__global__ __launch_bounds__(kRowThreads) void x0t_apply_kernel(x0t_params a) {
  __shared__ unsigned long long tot[kBins], sel[3];
  __shared__ x0t_row row_sh;
  __shared__ uint32_t n_changed;
  const unsigned row = blockIdx.x / a.chunks, chunk = blockIdx.x - row * a.chunks, tid = threadIdx.x;
  const size_t n = a.row_elems;
  uint32_t key_k = 0, key_k1 = 0;
  double frac = 0.0;
  if (tid == 0) n_changed = 0;
  if (a.mode == X0T_DYNAMIC) {
    uint32_t prefix;
    unsigned long long krem;
    x0t_advance(a, row, kDigits, tot, sel, prefix, krem, frac);        // the last digit: prefix is a_(k), krem the rank inside its run
    key_k = key_k1 = prefix;
    if (tid == 0) {
      if (krem + 1 >= sel[1]) {                            // the run ends at k: the next occupied bin of the last digit, else the smallest key beyond
        uint32_t nk = kNoKey;
        for (int b = (int)sel[0] + 1; b < kBins && nk == kNoKey; ++b)
          if (tot[b]) nk = (prefix & ~(uint32_t)(kBins - 1)) | (uint32_t)b;
        if (nk == kNoKey)
          for (unsigned c = 0; c < a.chunks; ++c) nk = min(nk, a.min_above[(size_t)row * a.chunks + c]);
        if (nk != kNoKey) key_k1 = nk;                     // none: k is the last rank, a_(n) := a_(n-1)
      }
    }
  }
  if (tid == 0) {
    double st[3];
    row_sh = x0t_decide(a, key_k, key_k1, frac, st);
    if (a.stats && chunk == 0) { a.stats[(size_t)row * 4 + 0] = st[0]; a.stats[(size_t)row * 4 + 1] = st[1]; a.stats[(size_t)row * 4 + 2] = st[2]; }
  }
  __syncthreads();
  const x0t_row R = row_sh;
  const x0t_coef kf = x0t_coef_of(a, row);
  const float* xr = a.x + (size_t)row * a.x_row_stride;
  const float* er = a.eps + (size_t)row * n;
  float* outr = a.eps_out + (size_t)row * n;
  unsigned changed = 0;
#pragma unroll
  for (int g = 0; g < kRowGroups; ++g) {
    const size_t e = row_group_elem(chunk, g);
    if (e < n) {
      const f32x4 xv = load4<VEC>(xr, e, n), ev = load4<VEC>(er, e, n);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned ch = 0;
        o[j] = x0t_apply(kf, R, xv[j], ev[j], ch);
        if (VEC || e + j < n) changed += ch;
      }
      store4<VEC>(outr, e, n, o);
    }
  }
  if (a.stats) {
    if (changed) atomicAdd(&n_changed, changed);
    __syncthreads();
    if (tid == 0) a.changed[(size_t)row * a.chunks + chunk] = n_changed;
  }
}
// stats[row][3]: the per-chunk counts of changed elements, added in chunk order (integers: exact)
__global__ void x0t_count_kernel(x0t_params a, int rows) {
  const unsigned row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= (unsigned)rows) return;
  unsigned long long s = 0;
  for (unsigned c = 0; c < a.chunks; ++c) s += a.changed[(size_t)row * a.chunks + c];
  a.stats[(size_t)row * 4 + 3] = (double)s;
}

constexpr size_t kStateBytes = (size_t)kDigits * 2 * sizeof(unsigned long long);      // per row
constexpr size_t kChunkWords = 2 * kBins + 2;                                          // per (row, chunk): two histograms, min_above, changed

bool x0t_resident(int form, size_t row_elems) { return form == 1 || (form == 0 && row_elems <= PF_X0T_RESIDENT_MAX); }

}  // namespace

size_t x0_threshold_workspace_bytes(int rows, size_t row_elems, int form) {
  if (rows <= 0 || row_elems == 0 || form < 0 || form > 2 || x0t_resident(form, row_elems)) return 0;
  return (size_t)rows * (kStateBytes + chunks_of(row_elems, PF_MSE_CHUNK) * kChunkWords * sizeof(uint32_t));
}

int launch_x0_threshold(const pf_x0_threshold_args& a, hipStream_t s) {
  PF_REQUIRE(a.x && a.eps && a.eps_out && a.t && a.table, "x0_threshold: null x, eps, eps_out, t or table");
  PF_REQUIRE(a.rows > 0 && a.row_elems > 0, "x0_threshold: %d rows of %zu elements", a.rows, a.row_elems);
  PF_REQUIRE(a.x_row_stride >= a.row_elems, "x0_threshold: x_row_stride %zu below row_elems %zu", a.x_row_stride, a.row_elems);
  PF_REQUIRE(a.t_stride >= 0 && a.n_table > 0, "x0_threshold: t_stride %d, n_table %d", a.t_stride, a.n_table);
  PF_REQUIRE(std::isfinite(a.lo) && std::isfinite(a.hi) && a.lo < a.hi, "x0_threshold: range [%g, %g] is not lo < hi, both finite", (double)a.lo, (double)a.hi);
  PF_REQUIRE(a.p > 0.0 && a.p <= 1.0, "x0_threshold: p %g outside (0, 1]", a.p);             // (a NaN fails both)
  PF_REQUIRE(a.s_max >= 1.0, "x0_threshold: s_max %g below 1", a.s_max);                     // (a NaN fails; +inf passes)
  PF_REQUIRE(a.mode == X0T_CLIP || a.mode == X0T_DYNAMIC, "x0_threshold: unknown mode %d (0 clip, 1 dynamic)", a.mode);
  PF_REQUIRE(a.form >= 0 && a.form <= 2, "x0_threshold: unknown form %d (0 auto, 1 resident, 2 streamed)", a.form);
  PF_REQUIRE(a.form != 1 || a.row_elems <= PF_X0T_RESIDENT_MAX, "x0_threshold: the resident form holds rows of at most %d elements, got %zu",
             PF_X0T_RESIDENT_MAX, a.row_elems);
  PF_REQUIRE(a.row_elems < (1ull << 32), "x0_threshold: rows of %zu elements", a.row_elems);
  const size_t bytes = (size_t)a.rows * a.row_elems * sizeof(float);
  PF_REQUIRE(a.eps_out == a.eps || !ranges_overlap(a.eps_out, bytes, a.eps, bytes), "x0_threshold: eps_out overlaps eps partially (in place is eps_out == eps)");
  PF_REQUIRE(!ranges_overlap(a.eps_out, bytes, a.x, ((size_t)(a.rows - 1) * a.x_row_stride + a.row_elems) * sizeof(float)), "x0_threshold: eps_out overlaps x");
  PF_REQUIRE(!ranges_overlap(a.eps_out, bytes, a.table, (size_t)a.n_table * 4 * sizeof(float)), "x0_threshold: eps_out overlaps table");
  PF_REQUIRE(!ranges_overlap(a.eps_out, bytes, a.t, ((size_t)(a.rows - 1) * a.t_stride + 1) * sizeof(int64_t)), "x0_threshold: eps_out overlaps t");
  PF_REQUIRE(((uintptr_t)a.stats & 7) == 0, "x0_threshold: stats must be 8-byte aligned");
  const bool resident = x0t_resident(a.form, a.row_elems);
  const size_t chunks = chunks_of(a.row_elems, PF_MSE_CHUNK), need = x0_threshold_workspace_bytes(a.rows, a.row_elems, a.form);
  if (need) {
    PF_REQUIRE(a.workspace, "x0_threshold: no workspace (pf_x0_threshold_workspace_bytes)");
    PF_REQUIRE(a.workspace_bytes >= need, "x0_threshold: workspace of %zu bytes required, got %zu", need, a.workspace_bytes);
    PF_REQUIRE(((uintptr_t)a.workspace & 7) == 0, "x0_threshold: workspace must be 8-byte aligned");
    PF_REQUIRE(chunks * (size_t)a.rows < (1ull << 31), "x0_threshold: %d rows of %zu elements are more workgroups than one launch holds", a.rows, a.row_elems);
  }
  x0t_params p{};
  p.x = a.x; p.x_row_stride = a.x_row_stride; p.eps = a.eps; p.eps_out = a.eps_out; p.t = a.t; p.t_stride = a.t_stride;
  p.table = a.table; p.n_table = a.n_table; p.stats = a.stats; p.p = a.p; p.s_max = a.s_max; p.lo = a.lo; p.hi = a.hi; p.mode = a.mode;
  p.row_elems = a.row_elems; p.chunks = (unsigned)chunks;
  // 16-byte accesses: every row of x, eps and eps_out then starts 16-byte aligned too
  const bool vec = aligned16({a.x, a.eps, a.eps_out}) && a.row_elems % 4 == 0 && a.x_row_stride % 4 == 0;
  if (resident) {
    const size_t lds = a.mode == X0T_DYNAMIC ? align_up(a.row_elems, 4) * sizeof(uint32_t) : 0;
    static std::atomic<uint64_t> done_v{0}, done_e{0};
    constexpr int lds_max = PF_X0T_RESIDENT_MAX * (int)sizeof(uint32_t);
    if (int rc = set_max_lds_once(reinterpret_cast<const void*>(x0t_resident_kernel<true>), lds_max, done_v)) return rc;
    if (int rc = set_max_lds_once(reinterpret_cast<const void*>(x0t_resident_kernel<false>), lds_max, done_e)) return rc;
    if (vec) hipLaunchKernelGGL(x0t_resident_kernel<true>, dim3(a.rows), dim3(kResThreads), lds, s, p);
    else hipLaunchKernelGGL(x0t_resident_kernel<false>, dim3(a.rows), dim3(kResThreads), lds, s, p);
    PF_CHECK_HIP(hipGetLastError());
    return PF_OK;
  }
  const size_t rc_ = (size_t)a.rows * chunks;
  p.state = reinterpret_cast<unsigned long long*>(a.workspace);
  p.hist = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.workspace) + (size_t)a.rows * kStateBytes);
  p.hist_stride = rc_ * kBins;
  p.min_above = p.hist + 2 * p.hist_stride;
  p.changed = p.min_above + rc_;
  const dim3 grid((unsigned)rc_), block(kRowThreads);
  if (a.mode == X0T_DYNAMIC) {
    for (int d = 0; d < kDigits; ++d) {
      if (vec) hipLaunchKernelGGL(x0t_hist_kernel<true>, grid, block, 0, s, p, d);
      else hipLaunchKernelGGL(x0t_hist_kernel<false>, grid, block, 0, s, p, d);
      PF_CHECK_HIP(hipGetLastError());
    }
  }
  if (vec) hipLaunchKernelGGL(x0t_apply_kernel<true>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(x0t_apply_kernel<false>, grid, block, 0, s, p);
  PF_CHECK_HIP(hipGetLastError());
  if (a.stats) {
    hipLaunchKernelGGL(x0t_count_kernel, dim3((a.rows + 255) / 256), dim3(256), 0, s, p, (int)a.rows);
    PF_CHECK_HIP(hipGetLastError());
  }
  return PF_OK;
}

}  // namespace pf
