// abi_ops.hip - the part of the C ABI that belongs to no model handle: the library's error state, its version and build queries, and the
// entry points that launch a single kernel or pack a single weight (sampler steps, RNG, attention, convs, norms, packers, probes, step state).
#include <stdarg.h>
#include <vector>
#include "plan.h"
#include "conv_plan.h"

namespace pf {

static thread_local std::string g_err;
int set_error(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

}  // namespace pf

using namespace pf;

extern "C" {

int pf_version(void) { return 102; }
const char* pf_last_error(void) { return g_err.c_str(); }
int pf_x3_element(void) {
#ifdef PF_X3_F16
  return 1;
#else
  return 0;
#endif
}

size_t pf_packed_gemm_weight_floats(int n, int k, int taps) { return gemm_floats(taps, k, n); }
int pf_pack_gemm_weight(const float* w, int n, int k, int taps, float* dst) {
  PF_REQUIRE(w && dst && n > 0 && k > 0 && k % 4 == 0 && (taps == 1 || taps == 9), "pf_pack_gemm_weight: bad arguments");
  memset(dst, 0, gemm_floats(taps, k, n) * sizeof(float));
  pack_gemm(dst, w, n, k, taps, (n + 63) / 64 * 64, 0);
  return PF_OK;
}

int pf_pack_gemm_weight_bf16x3(const float* w, int n, int k, int taps, void* dst) {
  PF_REQUIRE(w && dst && n > 0 && k > 0 && k % 8 == 0 && (taps == 1 || taps == 9), "pf_pack_gemm_weight_bf16x3: bad arguments");
  memset(dst, 0, gemm_floats(taps, k, n) * sizeof(float));
  PF_REQUIRE(pack_gemm_bf3(dst, w, n, k, taps, (n + 63) / 64 * 64, 0, nullptr), X3_RANGE_MSG, "pf_pack_gemm_weight_bf16x3");
  return PF_OK;
}

int pf_gn_scale_shift(const float* x0, int c0, const float* x1, int c1, int batch, int hw, int groups, float eps,
                      const float* gamma, const float* beta, float* scale, float* shift, void* scratch, size_t scratch_bytes,
                      void* stream) {
  return launch_gn_scale_shift(x0, c0, x1, c1, batch, hw, groups, eps, gamma, beta, scale, shift, scratch, scratch_bytes, (hipStream_t)stream);
}
int pf_pack_upfold_weight_bf16x3(const float* w, int n, int k, void* dst) {
  PF_REQUIRE(w && dst && n > 0 && k > 0 && k % 8 == 0, "pack_upfold: bad arguments");
  PF_REQUIRE(pack_upfold_bf3(dst, w, n, k, (n + 63) / 64 * 64), X3_RANGE_MSG, "pf_pack_upfold_weight_bf16x3");
  return PF_OK;
}
size_t pf_wino_weight_bytes(int n, int k) { return (n > 0 && k > 0) ? (size_t)16 * k * n * 4 : 0; }
int pf_pack_wino_weight_bf16x3(const float* w, int n, int k, void* dst) {
  PF_REQUIRE(w && dst && n > 0 && k > 0 && n % 64 == 0 && k % 16 == 0, "pack_wino: n must be a multiple of 64 and k of 16 (n=%d k=%d)", n, k);
  PF_REQUIRE(pack_wino_bf3(dst, w, n, k), X3_RANGE_MSG, "pf_pack_wino_weight_bf16x3");
  return PF_OK;
}
int pf_prmat2c_durations(const float* prmat2c, int n, int steps, int custom_round, int32_t* dur, void* stream) {
  return launch_prmat2c_durations(prmat2c, n, steps, custom_round, dur, (hipStream_t)stream);
}
int pf_roll_stats(const pf_roll_stats_args* a, void* stream) {
  PF_REQUIRE(a, "pf_roll_stats: null arguments");
  return launch_roll_stats(*a, (hipStream_t)stream);
}
int pf_chord_recognize(const pf_chord_recognize_args* a, void* stream) {
  PF_REQUIRE(a, "pf_chord_recognize: null arguments");
  return launch_chord_recognize(*a, (hipStream_t)stream);
}
int pf_roll_pack(const float* prmat2c, int n, int steps, int custom_round, uint32_t* bits, void* stream) {
  return launch_roll_pack(prmat2c, n, steps, custom_round, bits, (hipStream_t)stream);
}
size_t pf_roll_match_workspace_bytes(int na, int nb, int topk) { return roll_match_workspace_bytes(na, nb, topk); }
int pf_roll_match(const pf_roll_match_args* a, void* stream) {
  PF_REQUIRE(a, "pf_roll_match: null arguments");
  return launch_roll_match(*a, (hipStream_t)stream);
}
int pf_mlp_geglu_fused(const float* x, int batch, int l, const float* ln_gamma, const float* ln_beta, float ln_eps,
                       const void* w1_bf16x3, const float* b1, const void* w2_bf16x3, const float* b2,
                       float* out, void* out_planes, void* stream) {
  return launch_mlp_fused(x, batch, l, ln_gamma, ln_beta, ln_eps, w1_bf16x3, b1, w2_bf16x3, b2, out, out_planes, (hipStream_t)stream);
}
int pf_mlp_geglu_proj_fused(const float* x, int batch, int l, const float* ln_gamma, const float* ln_beta, float ln_eps,
                            const void* w1_bf16x3, const float* b1, const void* w2_bf16x3, const float* b2,
                            const void* w3_bf16x3, const float* b3, const float* res3, float* out, float* stats3, void* stream) {
  if (!w3_bf16x3) return set_error(PF_EINVAL, "pf_mlp_geglu_proj_fused: null projection weight");
  return launch_mlp_fused(x, batch, l, ln_gamma, ln_beta, ln_eps, w1_bf16x3, b1, w2_bf16x3, b2, out, nullptr, (hipStream_t)stream, w3_bf16x3, b3,
                          res3, stats3);
}
int pf_ln_planes(const float* x, int rows, int c, float eps, const float* gamma, const float* beta, void* planes, void* stream) {
  return launch_ln_planes(x, rows, c, eps, gamma, beta, planes, (hipStream_t)stream);
}
int pf_ln_stats(const float* x, int rows, int c, float eps, float* mean, float* rstd, void* stream) {
  return launch_ln_stats(x, rows, c, eps, mean, rstd, (hipStream_t)stream);
}
int pf_conv_in(const float* x_nchw, const float* w, const float* bias, float* out_nhwc, int batch, int cin, int cout, int h, int w_,
               float* stats, void* stream) {
  PF_REQUIRE(x_nchw && w && bias && out_nhwc && batch > 0 && cin > 0 && cout > 0 && h > 0 && w_ > 0, "pf_conv_in: bad arguments");
  return launch_conv_in(x_nchw, w, bias, out_nhwc, batch, cin, cout, h, w_, (hipStream_t)stream, stats);
}
int pf_conv_in_stats_tiles(int cin, int cout, int h, int w_) { return (cin > 0 && h > 0 && w_ > 0) ? launch_conv_in_stats_tiles(cin, cout, h, w_) : 0; }
int pf_conv_out(const float* x_nhwc, const float* sc, const float* sh, const float* w, const float* bias, float* out_nchw, int batch, int cin,
                int cout, int h, int w_, void* stream) {
  PF_REQUIRE(x_nhwc && sc && sh && w && bias && out_nchw && batch > 0 && cin > 0 && h > 0 && w_ > 0, "pf_conv_out: bad arguments");
  return launch_conv_out(x_nhwc, sc, sh, w, bias, out_nchw, batch, cin, cout, h, w_, (hipStream_t)stream);
}
int pf_time_embed(const int64_t* t, const float* w0, const float* b0, const float* w2, const float* b2, float* out_silu, int batch,
                  int channels, int d_t, void* stream) {
  PF_REQUIRE(w0 && b0 && w2 && b2 && out_silu && batch > 0 && channels > 0 && d_t > 0, "pf_time_embed: bad arguments");
  return launch_time_embed(t, w0, b0, w2, b2, out_silu, batch, channels, d_t, (hipStream_t)stream);
}
int pf_matvec(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int batch, int n, int k, int n_per_group,
              int x_group_stride, int exp_flag, void* stream) {
  PF_REQUIRE(!exp_flag || n_per_group <= 0, "pf_matvec: the exp variant has no grouped form");
  return exp_flag ? launch_matvec_exp(x, ldx, w, bias, y, ldy, batch, n, k, (hipStream_t)stream)
                  : launch_matvec(x, ldx, w, bias, y, ldy, batch, n, k, (hipStream_t)stream, n_per_group, x_group_stride);
}
int pf_gru_gates(const float* gi, int ld_gi, const float* gh, float* h, int ld_h, int rows, int hidden, const int* lens, int seq_len,
                 int step, int reverse, void* stream) {
  PF_REQUIRE(gi && gh && h && rows > 0 && hidden > 0, "pf_gru_gates: bad arguments");
  PF_REQUIRE(ld_h >= hidden, "pf_gru_gates: ld_h=%d below hidden=%d", ld_h, hidden);
  PF_REQUIRE((int64_t)rows * hidden < ((int64_t)1 << 31), "pf_gru_gates: rows * hidden must stay below 2^31");
  if (lens) {
    PF_REQUIRE(seq_len > 0 && step >= 0, "pf_gru_gates: seq_len must be positive and step non-negative");
    return launch_gru_gates_masked(gi, gh, h, ld_h, rows, hidden, seq_len, lens, step, reverse != 0, (hipStream_t)stream);
  }
  PF_REQUIRE(ld_gi >= 3 * hidden, "pf_gru_gates: ld_gi=%d below 3 * hidden", ld_gi);
  return launch_gru_gates(gi, ld_gi, gh, h, ld_h, rows, hidden, (hipStream_t)stream);
}
int pf_gru_step(const pf_gru_step_args* a, void* stream) {
  PF_REQUIRE(a, "pf_gru_step: null arguments");
  return launch_gru_step_flat(*a, (hipStream_t)stream);
}
int pf_conv_stats_tiles(const pf_conv_args* a) { return a ? conv_plan(*a).stats_tiles : 0; }
size_t pf_conv_splitk_ws_bytes(const pf_conv_args* a) { return a ? conv_plan(*a).splitk_ws_bytes : 0; }
int pf_conv_describe(const pf_conv_args* a, pf_conv_plan_info* out) {
  PF_REQUIRE(a && out, "pf_conv_describe: null argument");
  memset(out, 0, sizeof *out);
  if (int rc = conv_validate(*a)) return rc;
  const ConvPlan pl = conv_plan(*a);
  out->form = pl.form; out->tile_h = pl.th; out->tile_w = pl.tw; out->tile_n = pl.bn; out->wave_groups = pl.wave_groups;
  out->ksplit_wanted = pl.ksplit_wanted; out->ksplit = pl.ksplit; out->stats_tiles = pl.stats_tiles;
  out->splitk_ws_bytes = pl.splitk_ws_bytes; out->flops = pl.flops;
  return PF_OK;
}
int pf_gn_finalize_tiles(const float* stats0, int tiles0, int c0, const float* stats1, int tiles1, int c1, int batch, int hw,
                         int groups, float eps, const float* gamma, const float* beta, float* scale, float* shift, void* stream) {
  return launch_gn_finalize_tiles(stats0, tiles0, c0, stats1, tiles1, c1, batch, hw, groups, eps, gamma, beta, scale, shift,
                                  (hipStream_t)stream);
}
int pf_conv2d(const pf_conv_args* a, void* stream) {
  PF_REQUIRE(a, "pf_conv2d: null argument");
  return launch_conv(*a, (hipStream_t)stream);
}
size_t pf_attention_split_scratch_bytes(int batch, int n_heads, int l) {
  return (batch > 0 && n_heads > 0 && l > 0) ? attention_bf3_split_floats(batch, n_heads, l, nullptr) * sizeof(float) : 0;
}
int pf_attention_bf16x3_split(const void* qkv_planes, float* o, int ldo, void* o_planes, int batch, int n_heads, int l, void* scratch, size_t scratch_bytes,
                              void* stream) {
  return launch_attention_bf3(qkv_planes, o, ldo, o_planes, batch, n_heads, l, 0, (hipStream_t)stream, static_cast<float*>(scratch), scratch_bytes / sizeof(float));
}
int pf_attention_bf16x3(const void* qkv_planes, float* o, int ldo, void* o_planes, int batch, int n_heads, int l, int form, void* stream) {
  return launch_attention_bf3(qkv_planes, o, ldo, o_planes, batch, n_heads, l, form, (hipStream_t)stream);
}
int pf_attention(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo, int batch,
                 int n_heads, int d_head, int lq, int lk, void* stream) {
  PF_REQUIRE(q && k && v && o, "pf_attention: null argument");
  return launch_attention(q, ldq, k, ldk, v, ldv, o, ldo, batch, n_heads, d_head, lq, lk, (hipStream_t)stream);
}

int pf_cfg_combine(const float* eps2, float scale, float* eps, size_t n, void* stream) { return launch_cfg_combine(eps2, scale, eps, n, (hipStream_t)stream); }
int pf_cfg_combine3(const float* eps3, float s1, float s2, float* eps, size_t n, void* stream) { return launch_cfg_combine3(eps3, s1, s2, eps, n, (hipStream_t)stream); }
size_t pf_cfg_rescale_workspace_bytes(int rows, size_t row_elems) { return cfg_rescale_workspace_bytes(rows, row_elems); }
int pf_cfg_rescale(const pf_cfg_rescale_args* a, void* stream) {
  PF_REQUIRE(a, "cfg_rescale: null arguments");
  return launch_cfg_rescale(*a, (hipStream_t)stream);
}
size_t pf_x0_threshold_workspace_bytes(int rows, size_t row_elems, int form) { return x0_threshold_workspace_bytes(rows, row_elems, form); }
int pf_x0_threshold(const pf_x0_threshold_args* a, void* stream) {
  PF_REQUIRE(a, "x0_threshold: null arguments");
  return launch_x0_threshold(*a, (hipStream_t)stream);
}
int pf_x0_predict(const pf_x0_predict_args* a, void* stream) {
  PF_REQUIRE(a, "x0_predict: null arguments");
  return launch_x0_predict(*a, (hipStream_t)stream);
}
int pf_steer_resample(const pf_steer_resample_args* a, void* stream) {
  PF_REQUIRE(a, "steer_resample: null arguments");
  return launch_steer_resample(*a, (hipStream_t)stream);
}
int pf_rows_gather(const pf_rows_gather_args* a, void* stream) {
  PF_REQUIRE(a, "rows_gather: null arguments");
  return launch_rows_gather(*a, (hipStream_t)stream);
}
int pf_window_split(const float* canvas,float* windows, int songs, int channels, int win_h, int width, int n_windows, int stride, void* stream) {
  return launch_window_split(canvas, windows, songs, channels, win_h, width, n_windows, stride, (hipStream_t)stream);
}
int pf_window_merge(const pf_window_merge_args* a, void* stream) {
  PF_REQUIRE(a, "window_merge: null arguments");
  return launch_window_merge(*a, (hipStream_t)stream);
}
int pf_ddpm_step(const pf_ddpm_step_args* a, void* stream) {
  PF_REQUIRE(a, "pf_ddpm_step: null arguments");
  return launch_ddpm_step(*a, (hipStream_t)stream);
}
int pf_ddim_step(const pf_ddim_step_args* a, void* stream) {
  PF_REQUIRE(a, "pf_ddim_step: null arguments");
  return launch_ddim_step(*a, (hipStream_t)stream);
}
int pf_dpm_step(const pf_dpm_step_args* a, void* stream) {
  PF_REQUIRE(a, "pf_dpm_step: null arguments");
  return launch_dpm_step(*a, (hipStream_t)stream);
}
int pf_dpm_sde_step(const pf_dpm_sde_step_args* a, void* stream) {
  PF_REQUIRE(a, "pf_dpm_sde_step: null arguments");
  return launch_dpm_sde_step(*a, (hipStream_t)stream);
}
size_t pf_invert_step_workspace_bytes(int rows, size_t row_elems) { return invert_step_workspace_bytes(rows, row_elems); }
int pf_invert_step(const pf_invert_step_args* a, void* stream) {
  PF_REQUIRE(a, "pf_invert_step: null arguments");
  return launch_invert_step(*a, (hipStream_t)stream);
}
size_t pf_slerp_rows_workspace_bytes(int rows, size_t row_elems) { return slerp_rows_workspace_bytes(rows, row_elems); }
int pf_slerp_rows(const pf_slerp_args* a, void* stream) {
  PF_REQUIRE(a, "slerp_rows: null arguments");
  return launch_slerp_rows(*a, (hipStream_t)stream);
}
int pf_step_advance(pf_step_state* st, int64_t delta, int draws_used, void* stream) { return launch_step_advance(st, delta, draws_used, (hipStream_t)stream); }
int pf_axpby(const float* x, const float* noise, float a, float b, float* out, size_t n, void* stream) { return launch_axpby(x, noise, a, b, out, n, (hipStream_t)stream); }
int pf_randn(float* out, size_t n, uint64_t seed, uint64_t stream_id, uint64_t elem_offset, void* stream) {
  return launch_randn(out, n, seed, stream_id, elem_offset, (hipStream_t)stream);
}
int pf_mfma_probe(float* sink, int iters, double* flops_out, void* stream) { return launch_mfma_probe(sink, iters, flops_out, (hipStream_t)stream); }
int pf_clock_probe(uint64_t* out2, void* stream) { return launch_clock_probe(reinterpret_cast<unsigned long long*>(out2), (hipStream_t)stream); }
int pf_step_state_set(pf_step_state* st, int64_t index, uint64_t draws, void* stream) { return launch_step_state_set(st, index, draws, (hipStream_t)stream); }
int pf_step_begin(const pf_step_state* st, const int32_t* time_steps, int64_t* t_out, int batch, void* stream) {
  return launch_step_begin(st, time_steps, t_out, batch, (hipStream_t)stream);
}
int pf_step_end(pf_step_state* st, int draws_used, void* stream) { return launch_step_end(st, draws_used, (hipStream_t)stream); }
int pf_randn_dev(float* out, size_t n, uint64_t seed, const pf_step_state* st, int slot, uint64_t elem_offset, void* stream) {
  return launch_randn_dev(out, n, seed, st, slot, elem_offset, (hipStream_t)stream);
}

size_t pf_attention_wide_scratch_bytes(int batch, int l) { return (batch > 0 && l > 0) ? attention_wide_scratch_floats(batch, l) * sizeof(float) : 0; }
int pf_attention_wide(const float* q, const float* k, const float* v, int ld, float* o, int ldo, int batch, int l, int d, void* scratch,
                      size_t scratch_bytes, void* stream) {
  return launch_attention_wide(q, k, v, ld, o, ldo, batch, l, d, static_cast<float*>(scratch), scratch_bytes / sizeof(float), (hipStream_t)stream);
}
size_t pf_convt_weight_floats(int cin, int cout) { return (cin > 0 && cout > 0) ? (size_t)16 * cin * cout : 0; }
int pf_pack_convt_weight_f32(const float* w, int cin, int cout, float* dst) {
  PF_REQUIRE(w && dst && cin > 0 && cout > 0 && cin % 4 == 0, "pf_pack_convt_weight_f32: bad arguments");
  pack_convT_f32(w, cin, cout, dst);
  return PF_OK;
}
int pf_pack_convt_weight_bf16x3(const float* w, int cin, int cout, void* dst) {
  PF_REQUIRE(w && dst && cin > 0 && cout > 0 && cin % 8 == 0, "pf_pack_convt_weight_bf16x3: bad arguments");
  std::vector<float> fold((size_t)16 * cin * cout);
  convT_fold(w, cin, cout, fold.data());
  memset(dst, 0, gemm_floats(16, cin, cout) * sizeof(float));
  PF_REQUIRE(pack_gemm_bf3(dst, fold.data(), cout, cin, 16, (cout + 63) / 64 * 64, 0, nullptr),
             "pf_pack_convt_weight_bf16x3: a weight exceeds what this library's fp16 split packing holds");
  return PF_OK;
}
int pf_conv_transpose_f32(const float* x, int batch, int h, int w, int cin, const float* w_packed, int cout, const float* bias, float* out,
                          void* stream) {
  return launch_convT_f32(x, batch, h, w, cin, w_packed, cout, bias, out, (hipStream_t)stream);
}

}  // extern "C"
