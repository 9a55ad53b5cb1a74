// loss.hip - the training objective, forward only (gfx950): the two memory-bound launches around the denoiser in
// LatentDiffusion.loss / DenoiseDiffusion.loss (stable_diffusion/latent_diffusion.py:149-177, 203-240; ddpm/__init__.py:36-64, 90-111):
//   qsample_rows - x_t = sqrt(alpha_bar_t) x0 + sqrt(1 - alpha_bar_t) noise with one t per sample,
//   mse_rows     - per-sample sum of (noise - eps_theta)^2 in float64, as per-chunk partials + an in-order second pass.
// Both read and write 16 bytes per lane and take one Philox call per four elements when the noise is drawn (or re-drawn) in the kernel.
// And the objective of the chord VAE (Chord_8Bar.chord_loss, models/model_chd_8bar.py:21-39):
//   chord_ce_rows - per-sample sums of the three cross-entropies (root, chroma, bass) in float64, one workgroup per row.
#include "elementwise.h"

namespace pf {

namespace {

constexpr int kThreads = kRowThreads;
constexpr int kQChunk = 4 * kThreads;            // elements of a row one qsample workgroup owns: one 16-byte group per lane

// workgroup = (row, chunk of kQChunk elements); lane = one 16-byte group.  x_t and x0 carry no __restrict__: x_t may alias x0.
template <bool VEC, bool RNG>
__global__ __launch_bounds__(kThreads) void qsample_rows_kernel(const float* x0, const float* __restrict__ noise, const long long* __restrict__ t,
                                                               const float* __restrict__ sqrt_ab, const float* __restrict__ sqrt_1mab, int n_steps,
                                                               uint64_t seed, uint64_t draw, uint64_t off, float* xt, float* __restrict__ noise_out,
                                                               size_t row_elems, unsigned chunks) {
  const unsigned row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks;
  const size_t e = (size_t)chunk * kQChunk + 4 * (size_t)threadIdx.x;
  if (e >= row_elems) return;
  long long tv = t[row];
  tv = tv < 0 ? 0 : (tv >= n_steps ? n_steps - 1 : tv);       // memory safety only: the host mirror rejects a bad t it can see
  const float a = sqrt_ab[tv], b = sqrt_1mab[tv];
  const size_t base = (size_t)row * row_elems;
  f32x4 nz;
  if (RNG) {
    nz = philox_normal4v((off + base + e) >> 2, draw, seed);
    if (noise_out) store4<true>(noise_out + base, e, row_elems, nz);
  } else {
    nz = load4<VEC>(noise + base, e, row_elems);
  }
  const f32x4 xv = load4<VEC>(x0 + base, e, row_elems);
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = add_rn(mul_rn(a, xv[j]), mul_rn(b, nz[j]));
  store4<VEC>(xt + base, e, row_elems, o);
}

// The row reduction of elementwise.h with one sum: a lane adds the squares of its groups in element order.  The order is fixed by
// (row_elems, element index) alone, so VEC and the element-by-element form give the same bits.
template <bool VEC, bool RNG>
__global__ __launch_bounds__(kThreads) void mse_partial_kernel(const float* __restrict__ eps, const float* __restrict__ noise, uint64_t seed,
                                                              uint64_t draw, uint64_t off, double* __restrict__ partial, size_t row_elems,
                                                              unsigned chunks) {
  const unsigned row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks;
  const size_t base = (size_t)row * row_elems;
  double acc[1] = {0.0};
#pragma unroll
  for (int k = 0; k < kRowGroups; ++k) {
    const size_t e = row_group_elem(chunk, k);
    if (e < row_elems) {
      const f32x4 nz = RNG ? philox_normal4v((off + base + e) >> 2, draw, seed) : load4<VEC>(noise + base, e, row_elems);
      const f32x4 ev = load4<VEC>(eps + base, e, row_elems);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double d = (double)sub_rn(nz[j], ev[j]);      // the difference in float32, as the reference forms it
        acc[0] += d * d;                                    // exact product (48 bits), float64 sum
      }
    }
  }
  row_reduce_store(acc, partial, row, chunks, chunk);
}
// one lane per row: the row's partials in index order
__global__ void mse_finish_kernel(const double* __restrict__ partial, double* __restrict__ row_sum, int rows, unsigned chunks) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  double s[1];
  row_partials_sum(partial, row, chunks, s);
  row_sum[row] = s[0];
}

// ---- chord cross-entropy.  A row has 14 * n_step items (per step: the root, 12 chroma bits, the bass); lane l owns items l, l + 256, ...
// in index order, then the butterfly and the four waves in wave order of row_reduce_store: an order fixed by n_step alone.
// -log_softmax(x)[target] = max + log(sum_j exp(x_j - max)) - x_target with x widened to float64 first.
template <int N>
__device__ __forceinline__ double ce_item(const float* __restrict__ x, int target, int& hit) {
  double v[N], vm = (double)x[0], vt = (double)x[0];
  int bi = 0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    v[j] = (double)x[j];
    if (v[j] > vm) { vm = v[j]; bi = j; }   // ties to the lowest index
    if (j == target) vt = v[j];
  }
  double se = 0.0;
#pragma unroll
  for (int j = 0; j < N; ++j) se += exp(v[j] - vm);
  hit = bi == target;
  return (vm + log(se)) - vt;
}
__device__ __forceinline__ int argmax12(const float* __restrict__ g) {
  int bi = 0;
#pragma unroll
  for (int j = 1; j < 12; ++j)
    if (g[j] > g[bi]) bi = j;
  return bi;
}
__global__ __launch_bounds__(kThreads) void chord_ce_rows_kernel(const float* __restrict__ root, const float* __restrict__ chroma,
                                                                const float* __restrict__ bass, const float* __restrict__ gt, int n_step,
                                                                double* __restrict__ ce_rows, int32_t* __restrict__ hit_rows) {
  const int row = blockIdx.x;
  double acc[3] = {0.0, 0.0, 0.0};
  int hits[3] = {0, 0, 0};
  for (int i = threadIdx.x; i < 14 * n_step; i += kThreads) {
    const int st = i / 14, k = i - st * 14;
    const size_t step = (size_t)row * n_step + st;
    const float* g = gt + step * 36;
    int hit = 0;
    if (k == 0) {
      acc[0] += ce_item<12>(root + step * 12, argmax12(g), hit);
      hits[0] += hit;
    } else if (k == 13) {
      acc[2] += ce_item<12>(bass + step * 12, argmax12(g + 24), hit);
      hits[2] += hit;
    } else {
      const long long c = (long long)g[12 + (k - 1)];        // .long(); the clamp is for memory safety only
      acc[1] += ce_item<2>(chroma + step * 24 + 2 * (k - 1), c < 0 ? 0 : (c > 1 ? 1 : (int)c), hit);
      hits[1] += hit;
    }
  }
  row_reduce_store(acc, ce_rows, row, 1, 0);                       // a row is one chunk: the sums land in ce_rows[row][3]
  if (hit_rows) row_reduce_store(hits, hit_rows, row, 1, 0);       // (uniform over the workgroup; integers: exact in any order)
}

}  // namespace

size_t mse_rows_workspace_bytes(int rows, size_t row_elems) {
  if (rows <= 0 || row_elems == 0) return 0;
  return (size_t)rows * chunks_of(row_elems, PF_MSE_CHUNK) * sizeof(double);
}

int launch_qsample_rows(const pf_qsample_rows_args& a, hipStream_t s) {
  PF_REQUIRE(a.x0 && a.t && a.sqrt_ab && a.sqrt_1mab && a.x_t && a.rows > 0 && a.row_elems > 0 && a.n_steps > 0, "qsample_rows: bad arguments");
  const size_t chunks = chunks_of(a.row_elems, kQChunk);
  PF_REQUIRE(chunks * (size_t)a.rows < (1ull << 31), "qsample_rows: %d rows of %zu elements are more workgroups than one launch holds", a.rows, a.row_elems);
  const bool vec = a.row_elems % 4 == 0 && aligned16({a.x0, a.x_t, a.noise, a.noise_out});
  const dim3 grid((unsigned)(chunks * a.rows)), block(kThreads);
  const long long* t = reinterpret_cast<const long long*>(a.t);
  if (a.rng) {
    PF_REQUIRE(!a.noise, "qsample_rows_rng: the noise is drawn in the kernel, the noise tensor must be NULL");
    PF_REQUIRE(a.row_elems % 4 == 0 && a.elem_offset % 4 == 0, "qsample_rows_rng: row_elems and elem_offset must be multiples of 4 (one Philox call yields four normals)");
    PF_REQUIRE(vec, "qsample_rows_rng: tensors must be 16-byte aligned");
    hipLaunchKernelGGL((qsample_rows_kernel<true, true>), grid, block, 0, s, a.x0, nullptr, t, a.sqrt_ab, a.sqrt_1mab, a.n_steps, a.seed, a.draw,
                       a.elem_offset, a.x_t, a.noise_out, a.row_elems, (unsigned)chunks);
  } else {
    PF_REQUIRE(a.noise && !a.noise_out, "qsample_rows: a noise tensor is required without rng (and noise_out belongs to rng)");
    if (vec)
      hipLaunchKernelGGL((qsample_rows_kernel<true, false>), grid, block, 0, s, a.x0, a.noise, t, a.sqrt_ab, a.sqrt_1mab, a.n_steps, 0, 0, 0, a.x_t,
                         nullptr, a.row_elems, (unsigned)chunks);
    else
      hipLaunchKernelGGL((qsample_rows_kernel<false, false>), grid, block, 0, s, a.x0, a.noise, t, a.sqrt_ab, a.sqrt_1mab, a.n_steps, 0, 0, 0, a.x_t,
                         nullptr, a.row_elems, (unsigned)chunks);
  }
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

int launch_mse_rows(const pf_mse_rows_args& a, hipStream_t s) {
  PF_REQUIRE(a.eps_theta && a.row_sum && a.rows > 0 && a.row_elems > 0, "mse_rows: bad arguments");
  const size_t chunks = chunks_of(a.row_elems, PF_MSE_CHUNK), need = mse_rows_workspace_bytes(a.rows, a.row_elems);
  PF_REQUIRE(chunks * (size_t)a.rows < (1ull << 31), "mse_rows: %d rows of %zu elements are more workgroups than one launch holds", a.rows, a.row_elems);
  PF_REQUIRE(a.workspace && a.workspace_bytes >= need && ((uintptr_t)a.workspace & 7) == 0 && ((uintptr_t)a.row_sum & 7) == 0,
             "mse_rows: workspace of %zu bytes (8-byte aligned) required, got %zu", need, a.workspace_bytes);
  const bool vec = a.row_elems % 4 == 0 && aligned16({a.eps_theta, a.noise});
  const dim3 grid((unsigned)(chunks * a.rows)), block(kThreads);
  double* partial = reinterpret_cast<double*>(a.workspace);
  if (a.rng) {
    PF_REQUIRE(!a.noise, "mse_rows_rng: the noise is re-drawn in the kernel, the noise tensor must be NULL");
    PF_REQUIRE(a.row_elems % 4 == 0 && a.elem_offset % 4 == 0, "mse_rows_rng: row_elems and elem_offset must be multiples of 4 (one Philox call yields four normals)");
    PF_REQUIRE(vec, "mse_rows_rng: tensors must be 16-byte aligned");
    hipLaunchKernelGGL((mse_partial_kernel<true, true>), grid, block, 0, s, a.eps_theta, nullptr, a.seed, a.draw, a.elem_offset, partial, a.row_elems,
                       (unsigned)chunks);
  } else {
    PF_REQUIRE(a.noise, "mse_rows: a noise tensor is required without rng");
    if (vec)
      hipLaunchKernelGGL((mse_partial_kernel<true, false>), grid, block, 0, s, a.eps_theta, a.noise, 0, 0, 0, partial, a.row_elems, (unsigned)chunks);
    else
      hipLaunchKernelGGL((mse_partial_kernel<false, false>), grid, block, 0, s, a.eps_theta, a.noise, 0, 0, 0, partial, a.row_elems, (unsigned)chunks);
  }
  PF_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(mse_finish_kernel, dim3((unsigned)cdiv(a.rows, 64)), dim3(64), 0, s, partial, a.row_sum, a.rows, (unsigned)chunks);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

int launch_chord_ce_rows(const float* root, const float* chroma, const float* bass, const float* gt, int rows, int n_step, double* ce_rows,
                         int32_t* hit_rows, hipStream_t s) {
  PF_REQUIRE(root && chroma && bass && gt && ce_rows && rows > 0 && n_step > 0, "chord_ce_rows: bad arguments");
  PF_REQUIRE(((uintptr_t)ce_rows & 7) == 0 && ((uintptr_t)hit_rows & 3) == 0, "chord_ce_rows: ce_rows must be 8-byte and hit_rows 4-byte aligned");
  hipLaunchKernelGGL(chord_ce_rows_kernel, dim3((unsigned)rows), dim3(kThreads), 0, s, root, chroma, bass, gt, n_step, ce_rows, hit_rows);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

}  // namespace pf

using namespace pf;

extern "C" {

int pf_qsample_rows(const pf_qsample_rows_args* a, void* stream) {
  PF_REQUIRE(a, "pf_qsample_rows: null arguments");
  return launch_qsample_rows(*a, (hipStream_t)stream);
}
size_t pf_mse_rows_workspace_bytes(int rows, size_t row_elems) { return mse_rows_workspace_bytes(rows, row_elems); }
int pf_mse_rows(const pf_mse_rows_args* a, void* stream) {
  PF_REQUIRE(a, "pf_mse_rows: null arguments");
  return launch_mse_rows(*a, (hipStream_t)stream);
}
int pf_chord_ce_rows(const float* root, const float* chroma, const float* bass, const float* gt, int rows, int n_step, double* ce_rows,
                     int32_t* hit_rows, void* stream) {
  return launch_chord_ce_rows(root, chroma, bass, gt, rows, n_step, ce_rows, hit_rows, (hipStream_t)stream);
}
int pf_normal_rsample(const float* mean, const float* std, const float* noise, uint64_t seed, uint64_t stream_id, uint64_t elem_offset,
                      float* z, size_t n, void* stream) {
  return launch_normal_rsample(mean, std, noise, seed, stream_id, elem_offset, z, n, (hipStream_t)stream);
}

}  // extern "C"
