// Internal declarations shared by the translation units of libpfhip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <string>
#include "../../include/pfhip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace pf {

int set_error(int code, const char* fmt, ...);

#define PF_CHECK_HIP(expr)                                                                   \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) return pf::set_error(PF_EHIP, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

#define PF_REQUIRE(cond, ...)                                   \
  do {                                                          \
    if (!(cond)) return pf::set_error(PF_EINVAL, __VA_ARGS__);  \
  } while (0)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: set it once per (kernel, device) - a process may
// drive several GPUs - with one bit per device in a mask owned by the launcher (two racing threads both set it: harmless)
static inline int set_max_lds_once(const void* kern, int bytes, std::atomic<uint64_t>& done_mask) {
  int dev = 0;
  PF_CHECK_HIP(hipGetDevice(&dev));
  const uint64_t bit = 1ull << (dev & 63);
  if (done_mask.load(std::memory_order_acquire) & bit) return PF_OK;
  PF_CHECK_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done_mask.fetch_or(bit, std::memory_order_release);
  return PF_OK;
}
// compute units of the current device (cached per device index; 256 on MI355X)
int num_cus();
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- launchers implemented in the .hip files (all enqueue on `stream`, never sync) ----
int launch_conv(const pf_conv_args& a, hipStream_t stream);      // validate, plan, parameter block, form launcher (conv_plan.h)
// both return false when a weight does not fit the split's element type (fp16 build: |w| * 2^8 > 65504; the packing then holds the clamped value)
bool pack_gemm_bf3(void* dst, const float* src, int n_src, int K, int taps, int Npad, int n_off, const int* colmap);
bool pack_upfold_bf3(void* dst, const float* src, int N, int K, int Npad);   // UpSample conv weight -> 4 parities x 4 taps
// fused Winograd F(2x2, 3x3) form of the stride-1 3x3 conv (conv_wino.hip): the weight transform + packing
bool pack_wino_bf3(void* dst, const float* src, int N, int K);            // [N][K][3][3] -> U = G g G^T, hi | lo, MFMA B-operand order

int launch_attention(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                     int batch, int n_heads, int d_head, int lq, int lk, hipStream_t stream);

// form: PF_OPT_AUTO | 0 = 128-query workgroups | 1 = 256-query workgroups (needs l % 256 == 0)
// scratch (optional): attention_bf3_split_floats(...) floats enable the key-split form for small batches (a second, merging launch)
int launch_attention_bf3(const void* planes, float* o, int ldo, void* o_planes, int batch, int n_heads, int l, int form, hipStream_t stream,
                         float* scratch = nullptr, size_t scratch_floats = 0);
size_t attention_bf3_split_floats(int batch, int n_heads, int l, int* nsplit_out);
// out = x + ff2(GeGLU(ff1(LayerNorm(x)))) for C = 256, hidden 1024, as one launch (mlp_fused_bf3.hip); w1 / w2 = bf16x3 packings
int launch_mlp_fused(const float* x, int batch, int l, const float* gamma, const float* beta, float eps, const void* w1, const float* b1,
                     const void* w2, const float* b2, float* out, void* out_planes, hipStream_t stream, const void* w3 = nullptr,
                     const float* b3 = nullptr, const float* res3 = nullptr, float* stats3 = nullptr);

size_t gn_scratch_bytes(int batch, int c, int hw);
int launch_gn_scale_shift(const float* x0, int c0, const float* x1, int c1, int batch, int hw, int groups, float eps,
                          const float* gamma, const float* beta, float* scale, float* shift, void* scratch,
                          size_t scratch_bytes, hipStream_t stream);
int launch_gn_finalize_tiles(const float* s0, int t0, int c0, const float* s1, int t1, int c1, int batch, int hw, int groups,
                             float eps, const float* gamma, const float* beta, float* scale, float* shift, hipStream_t stream, int bmod1 = 0);
// per-split (sum, sumsq) of an NHWC tensor in the tile-statistics layout [B][gn_nsplit(hw)][C][2] (for tensors whose producer emits none)
int gn_nsplit(int hw);
int launch_gn_partial(const float* x0, int c0, const float* x1, int c1, int batch, int hw, float* stats, hipStream_t stream);
int launch_ln_stats(const float* x, int rows, int c, float eps, float* mean, float* rstd, hipStream_t stream);
int launch_ln_planes(const float* x, int rows, int c, float eps, const float* gamma, const float* beta, void* planes,
                     hipStream_t stream);

// stem / head convolutions (NCHW <-> NHWC at the ABI edge)
int launch_conv_in(const float* x_nchw, const float* w /*[Cout][Cin][3][3]*/, const float* bias, float* out_nhwc,
                   int batch, int cin, int cout, int h, int w_, hipStream_t stream, float* stats = nullptr);
int launch_conv_in_stats_tiles(int cin, int cout, int h, int w_);   // per-sample statistics tiles launch_conv_in can emit (0: none)
int launch_conv_out(const float* x_nhwc, const float* sc, const float* sh, const float* w /*[9][Cin][Cout]*/,
                    const float* bias, float* out_nchw, int batch, int cin, int cout, int h, int w_, hipStream_t stream);

// time embedding: t[B] -> silu(time_embed(sinusoid(t))) [B][d_t]
// t == nullptr: row b is the embedding of time-step value b (the hoisted table of pf_unet_prepare_time)
int launch_time_embed(const int64_t* t, const float* w0, const float* b0, const float* w2, const float* b2,
                      float* out_silu, int batch, int channels, int d_t, hipStream_t stream);
// y[b][n] = sum_k W[n][k] * x[b][k] + bias[n]   (row-major W [N][K]; one wave per output)
// grouped form: output n reads x + (n / n_per_group) * x_group_stride (block-diagonal W); n_per_group <= 0 disables
int launch_prmat2c_durations(const float* x, int n, int steps, int custom_round, int32_t* dur, hipStream_t stream);
// roll statistics (include/pfhip.h, pf_roll_stats): integer counters, per-beat pitch-class counts and per-step onset counts of n images
int launch_roll_stats(const pf_roll_stats_args& a, hipStream_t stream);
// chord recognition (include/pfhip.h, pf_chord_recognize; chordrec.hip): labels, condition rows and comparison counters of whole songs
int launch_chord_recognize(const pf_chord_recognize_args& a, hipStream_t stream);
// packed rolls and nearest neighbours under transposition (include/pfhip.h, pf_roll_pack / pf_roll_match; rollmatch.hip)
int launch_roll_pack(const float* x, int n, int steps, int custom_round, uint32_t* bits, hipStream_t stream);
size_t roll_match_workspace_bytes(int na, int nb, int topk);
int launch_roll_match(const pf_roll_match_args& a, hipStream_t stream);
int launch_matvec(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int batch, int n, int k,
                  hipStream_t stream, int n_per_group = 0, int x_group_stride = 0);
// y[b][n] = expf(sum_k W[n][k] * x[b][k] + bias[n]): the same kernel with the exponential in its epilogue
int launch_matvec_exp(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int batch, int n, int k,
                      hipStream_t stream);

// sampler elementwise kernels (sampler_steps.hip, written against elementwise.h)
int launch_cfg_combine(const float* eps2, float scale, float* eps, size_t n, hipStream_t s);
int launch_cfg_combine3(const float* eps3, float s1, float s2, float* eps, size_t n, hipStream_t s);
// guidance rescale: the combine of 2 or 3 groups scaled per row towards the conditional group's standard deviation (a reduce launch + a combine launch)
size_t cfg_rescale_workspace_bytes(int rows, size_t row_elems);
int launch_cfg_rescale(const pf_cfg_rescale_args& a, hipStream_t s);
// clipping / dynamic thresholding of the predicted x0, as a rewrite of eps (x0_threshold.hip): an exact per-row quantile by radix select
size_t x0_threshold_workspace_bytes(int rows, size_t row_elems, int form);
int launch_x0_threshold(const pf_x0_threshold_args& a, hipStream_t s);
// steering by resampling (steer.hip): the predicted x0 written out, the particle filter's resampling step, the move of the state rows
int launch_x0_predict(const pf_x0_predict_args& a, hipStream_t s);
int launch_steer_resample(const pf_steer_resample_args& a, hipStream_t s);
int launch_rows_gather(const pf_rows_gather_args& a, hipStream_t s);
// overlapping windows along the time axis: canvas -> window batch, and window eps -> canvas eps with the guidance combine folded in
int launch_window_split(const float* canvas, float* windows, int songs, int channels, int win_h, int width, int n_windows, int stride, hipStream_t s);
int launch_window_merge(const pf_window_merge_args& a, hipStream_t s);
// one reverse step per family: validates the arguments, then the tensor-noise or the in-kernel Philox kernel (include/pfhip.h)
int launch_ddpm_step(const pf_ddpm_step_args& a, hipStream_t s);
int launch_ddim_step(const pf_ddim_step_args& a, hipStream_t s);
// DPM-Solver++(2M): no noise, an optional history operand (x0_prev) and an optional second output (x0_out); scalar or 16-byte vector kernel
int launch_dpm_step(const pf_dpm_step_args& a, hipStream_t s);
// its stochastic form: the same update with sigma_n*z before the blend, the noise from a tensor or drawn in the kernel
int launch_dpm_sde_step(const pf_dpm_sde_step_args& a, hipStream_t s);
int launch_axpby(const float* x, const float* y, float a, float b, float* out, size_t n, hipStream_t s);
int launch_randn(float* out, size_t n, uint64_t seed, uint64_t stream_id, uint64_t elem_offset, hipStream_t s);
int launch_randn_dev(float* out, size_t n, uint64_t seed, const pf_step_state* st, int slot, uint64_t elem_offset, hipStream_t s);
int launch_clock_probe(unsigned long long* out2, hipStream_t s);
int launch_mfma_probe(float* sink, int iters, double* flops, hipStream_t s);
int launch_step_state_set(pf_step_state* st, int64_t index, uint64_t draws, hipStream_t s);
int launch_step_begin(const pf_step_state* st, const int* time_steps, int64_t* t_out, int batch, hipStream_t s);
int launch_step_end(pf_step_state* st, int draws_used, hipStream_t s);
int launch_step_advance(pf_step_state* st, int64_t delta, int draws_used, hipStream_t s);
// exact DDIM inversion: one fixed-point iterate of one upward step, optionally with the per-row residual sums (a second, in-order launch)
size_t invert_step_workspace_bytes(int rows, size_t row_elems);
int launch_invert_step(const pf_invert_step_args& a, hipStream_t s);
// a path between two noises: per-row slerp (a reduce launch + a combine launch) or lerp (the combine launch alone) of `frames` points
size_t slerp_rows_workspace_bytes(int rows, size_t row_elems);
int launch_slerp_rows(const pf_slerp_args& a, hipStream_t s);
// the training objective, forward only (loss.hip): forward noising with one t per sample, and the per-sample squared error in float64
int launch_qsample_rows(const pf_qsample_rows_args& a, hipStream_t s);
size_t mse_rows_workspace_bytes(int rows, size_t row_elems);
int launch_mse_rows(const pf_mse_rows_args& a, hipStream_t s);
// the chord VAE's objective (loss.hip): per-row sums of the root / chroma / bass cross-entropies in float64, and arg-max hits
int launch_chord_ce_rows(const float* root, const float* chroma, const float* bass, const float* gt, int rows, int n_step, double* ce_rows,
                         int32_t* hit_rows, hipStream_t s);

// vanilla DDPM network (attention_wide.hip): single-head attention with a wide head (exact fp32; scratch = batch * l * l floats), the
// ConvTranspose2d(4, 2, 1) parity fold (fold: [Cout][Cin][16], the pack_upfold_bf3 tap order; fp32 packing [4][4][Cin][Cout]) and its fp32
// launch, the labml time embedding (sin | cos, lin1, Swish, lin2)
size_t attention_wide_scratch_floats(int batch, int l);
int launch_attention_wide(const float* q, const float* k, const float* v, int ld, float* o, int ldo, int batch, int l, int d,
                          float* scratch, size_t scratch_floats, hipStream_t stream);
void convT_fold(const float* w, int cin, int cout, float* fold);
void pack_convT_f32(const float* w, int cin, int cout, float* dst);
int launch_convT_f32(const float* x, int batch, int h, int w, int cin, const float* wpk, int cout, const float* bias, float* out,
                     hipStream_t stream);
int launch_ddpm_time_embed(const int64_t* t, const float* w1, const float* b1, const float* w2, const float* b2, float* out, int batch,
                           int d_t, hipStream_t stream);

// first-stage autoencoder (small_kernels.hip; the two samplers as bodies of elementwise.h's ew_kernel): GaussianDistribution.sample on computed moments; the encoder tail - GroupNorm + SiLU +
// conv_out (3x3, cin -> z2) + quant_conv (1x1, z2 -> e2) + clamp + sample, x NHWC -> z / mean / log_var NCHW [B][e2 / 2][h][w], each
// optional; the decoder front - z / scale + post_quant_conv (1x1, emb -> zc) + conv_in (3x3, zc -> cout), z NCHW -> out NHWC.
// noise == nullptr: element i draws what launch_randn(seed, sid, off) writes at i
int launch_gaussian_sample(const float* mean, const float* log_var, const float* noise, uint64_t seed, uint64_t sid, uint64_t off, float scale,
                           float* z, size_t n, hipStream_t s);
// Normal(mean, sd).rsample(): z = mean + sd * noise, the product rounded, then the sum; noise as for launch_gaussian_sample
int launch_normal_rsample(const float* mean, const float* sd, const float* noise, uint64_t seed, uint64_t sid, uint64_t off, float* z, size_t n,
                          hipStream_t s);
int launch_ae_tail(const float* x, const float* sc, const float* sh, const float* w /*[9][cin][z2]*/, const float* bias, const float* qw /*[e2][z2]*/,
                   const float* qb, int z2, int e2, const float* noise, uint64_t seed, uint64_t sid, uint64_t off, float scale, float* z, float* mean,
                   float* log_var, int batch, int cin, int h, int w_, hipStream_t stream);
int launch_ae_front(const float* z, float scale, const float* pw /*[zc][emb]*/, const float* pb, const float* w /*[cout][zc][3][3]*/, const float* bias,
                    float* out, int batch, int emb, int zc, int cout, int h, int w_, hipStream_t stream);

// encoder kernels
int launch_gru_gates(const float* gi, int ld_gi, const float* gh, float* h, int ld_h, int batch, int hidden, hipStream_t s);
int launch_pnotree_embed(const float* grid, const float* w, const float* bias, float* out, int rows, int emb, int pitch_range, hipStream_t s);
int launch_pnotree_lengths(const float* grid, int* lens, int nseq, int max_simu_note, int pad, hipStream_t s);
int launch_gru_gates_masked(const float* gi, const float* gh, float* h, int ld_h, int nseq, int hidden, int seq_len, const int* lens,
                            int step, int reverse, hipStream_t s);
int launch_txt_frontend(const float* pr, const float* w, const float* bias, float* out, int batch, int num_channel,
                        hipStream_t s);
// decoder kernel: one fused GRU step from the flat arguments of pf_gru_step (decoders.hip)
int launch_gru_step_flat(const pf_gru_step_args& a, hipStream_t s);

}  // namespace pf

// ---- element type of the split-precision ("x3") kernels ---------------------------------------------------------------------------------
// The default build splits every operand into two bf16 pieces (8 + 8 mantissa bits, fp32's exponent range).  -DPF_X3_F16 compiles the very
// same kernels with fp16 pieces (11 + 11 bits, three v_mfma_f32_32x32x16_f16 per product at the same rate): ~16x less rounding error per
// product, paid for with fp16's range - |activation| must stay below 65504 and pieces below 6e-5 lose bits (fp16 subnormals ARE honoured by
// the matrix pipe, tools/micro/f16x3_probe.hip).  Weights are small numbers (|w| ~ 0.03 puts the lo piece deep in the subnormals), so that
// build packs them times PF_X3_WS = 2^8 and every epilogue takes its accumulators times 2^-8 - exact, and folded into the bias add as an fma.
// The kernels spell the element type x3_t, its vectors x3x2 / x3x4 / x3x8 (typedef'd where they are used) and the MFMA x3_mfma_32x32x16.
#ifdef PF_X3_F16
typedef _Float16 x3_t;
#define x3_mfma_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_f16
#define PF_X3_WS 256.0f
#define PF_X3_WS_INV 0.00390625f
#define PF_X3_UNSCALE(a) ((a) * PF_X3_WS_INV)
#else
typedef __bf16 x3_t;
#define x3_mfma_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_bf16
#define PF_X3_WS 1.0f
#define PF_X3_WS_INV 1.0f
#define PF_X3_UNSCALE(a) (a)
#endif
// accumulator tile -> true units (a no-op in the bf16 build)
template <int FM, int FN>
__device__ __forceinline__ void x3_unscale(f32x16 (&acc)[FM][FN]) {
#ifdef PF_X3_F16
#pragma unroll
  for (int fm = 0; fm < FM; ++fm)
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) acc[fm][fn] = acc[fm][fn] * PF_X3_WS_INV;
#endif
}
