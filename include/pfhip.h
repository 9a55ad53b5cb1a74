/* pfhip.h - C ABI of libpfhip.so: the MI355X (gfx950) denoising hot path of Polyffusion.
 *
 * The reference is pure Python/PyTorch and has no FFI for this path; its interface is the
 * call signature of the denoiser and of the sampler step.  Each entry point
 * below cites the reference callable it replaces (paths relative to
 * /root/reference/polyffusion).  INTEGRATION.md shows the ctypes stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative PF_E* code on failure; the message
 *     is available from pf_last_error() (thread-local).  No exceptions cross the ABI.
 *   - all device buffers are owned by the caller (allocated e.g. through torch); the
 *     library never allocates or frees device memory and never synchronises the device.
 *   - kernels are enqueued on the caller's hipStream_t (passed as void*), so they order with
 *     the caller's other work and can be captured into a hipGraph.
 *   - activations at the ABI are fp32.  x / eps are NCHW [B,C,H,W] exactly as the reference
 *     passes them; internal activations are NHWC and never leave the workspace.
 */
#ifndef PFHIP_H
#define PFHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_OK 0
#define PF_EINVAL (-1)   /* bad argument / unsupported shape */
#define PF_ENOTFOUND (-2) /* unknown parameter key */
#define PF_ESTATE (-3)   /* call order violated (e.g. forward before bind) */
#define PF_EHIP (-4)     /* HIP runtime error */

int pf_version(void);
const char* pf_last_error(void);

/* ---- denoiser (replaces UNetModel.__init__/forward, stable_diffusion/model/unet.py:30-196,
 *      incl. SpatialTransformer, unet_attention.py:26-333) ---------------------------------- */
typedef struct pf_unet pf_unet;

typedef struct pf_unet_cfg {
  int32_t in_channels, out_channels, channels, n_res_blocks;
  int32_t n_attention_levels;
  int32_t attention_levels[8];
  int32_t n_levels;
  int32_t channel_multipliers[8];
  int32_t n_heads, tf_layers, d_cond;
  int32_t img_h, img_w; /* spatial size of x (params.img_h/img_w) */
} pf_unet_cfg;

int pf_unet_create(const pf_unet_cfg* cfg, pf_unet** out);
void pf_unet_destroy(pf_unet* u);

/* Weight ingestion in the reference state_dict namespace (keys relative to ldm.eps_model.,
 * SURVEY.md Appendix D; replaces nn.Module.load_state_dict for unet.py).  The caller owns a
 * host staging blob of pf_unet_weight_bytes(); pf_unet_pack_param repacks ONE named tensor
 * (fp32, contiguous, torch layout) into its kernel-friendly place inside that blob.
 * pf_unet_pack_missing returns the number of keys not yet packed (0 = complete) and writes
 * the first missing key into buf.  The packed blob is then copied to the device by the
 * caller (or received by RCCL broadcast) and attached with pf_unet_bind_weights. */
size_t pf_unet_weight_bytes(const pf_unet* u);
int pf_unet_n_params(const pf_unet* u);
int pf_unet_param_info(const pf_unet* u, int i, char* key_buf, size_t key_buf_len, int64_t shape[4], int* ndim);
int pf_unet_pack_param(pf_unet* u, const char* key, const float* src, const int64_t* shape, int ndim, void* host_blob);
int pf_unet_pack_missing(const pf_unet* u, char* buf, size_t buf_len);
int pf_unet_bind_weights(pf_unet* u, const void* dev_blob);

/* Workspace (activations, skips, statistics) for a given batch / number of context tokens. */
size_t pf_unet_workspace_bytes(const pf_unet* u, int batch, int n_cond);

/* eps = UNet(x, t, cond): x [B,Cin,H,W] f32, t [B] i64, cond [B,n_cond,d_cond] f32,
 * eps [B,Cout,H,W] f32 (unet.py:171-196; LatentDiffusion.forward latent_diffusion.py:138-147). */
int pf_unet_forward(pf_unet* u, const float* x, const int64_t* t, const float* cond, int batch, int n_cond,
                    float* eps, void* workspace, size_t workspace_bytes, void* stream);

/* ---- step-invariant prefix, hoisted out of the reverse loop -----------------------------------------------------------
 * Two parts of UNetModel.forward do not depend on x: the time MLP + every ResBlock's emb_layers (unet.py:181-182, 286-289:
 * a function of t only) and, with ONE context token, the whole cross-attention (unet_attention.py:186-212, 261-293: softmax over
 * one key is 1, so attn2(x, c) = to_out(to_v(c)) for every position: a function of cond only).  A sampler knows every t of its
 * loop in advance and holds cond fixed, so it computes both ONCE and hands them to every forward of the loop:
 *   pf_unet_prepare_time - rows r = 0 .. n_rows-1 of `table` [n_rows][pf_unet_time_bias_width] = the additive time biases of all
 *                          ResBlocks for time-step VALUE r (what forward computes from t == r); scratch: n_rows * 4 * channels floats
 *   pf_unet_prepare_cond - `cross` [batch][pf_unet_cross_bias_width] = to_out(to_v(cond[b])) + bias of every transformer block
 *                          (n_cond == 1 only); scratch: batch * width floats
 * Both buffers are caller-owned device memory; nothing is cached inside the library.  pf_unet_forward_prepared with prep == NULL
 * (or with NULL members) computes the missing part itself, exactly like pf_unet_forward; results are bit-identical either way.
 * With a time table every t[b] must lie in [0, n_time_rows) (values outside are clamped for memory safety). */
typedef struct pf_unet_prepared {
  const float* time_table; int32_t n_time_rows;   /* from pf_unet_prepare_time, or NULL */
  const float* cross_bias;                         /* from pf_unet_prepare_cond for THIS cond / batch, or NULL */
} pf_unet_prepared;
int pf_unet_time_bias_width(const pf_unet* u);
int pf_unet_cross_bias_width(const pf_unet* u);
int pf_unet_prepare_time(pf_unet* u, int n_rows, float* table, void* scratch, size_t scratch_bytes, void* stream);
int pf_unet_prepare_cond(pf_unet* u, const float* cond, int batch, float* cross, void* scratch, size_t scratch_bytes, void* stream);
int pf_unet_forward_prepared(pf_unet* u, const float* x, const int64_t* t, const float* cond, int batch, int n_cond,
                             const pf_unet_prepared* prep, float* eps, void* workspace, size_t workspace_bytes, void* stream);
/* Classifier-free guidance (stable_diffusion/sampler/__init__.py:63-77 `get_eps`: the model is evaluated on cat([x, x]), cat([t, t]),
 * cat([uncond_cond, cond])).  The condition enters the UNet only through the cross-attention of its transformer blocks (unet.py:181-196,
 * unet_attention.py:240-246), so everything in front of the first SpatialTransformer - the stem, the ResBlocks and DownSamples of the levels
 * without attention, the first ResBlock of the first attention level - is IDENTICAL for the two halves.  This entry computes that prefix once on
 * the `batch2 / 2` samples of `x`, shares the skip tensors it produced between the halves (a sample index taken modulo batch2 / 2 inside the
 * consuming kernels: no copies) and runs the rest on all batch2 samples: the same eps2 [batch2, ...] as pf_unet_forward_prepared on the
 * concatenated inputs up to tile-choice rounding, for 13 % fewer FLOPs at sdf_chd8bar.  x: [batch2 / 2, ...]; t, cond (and prep->cross_bias): batch2
 * rows, second half = first half for t.  Workspace: pf_unet_workspace_bytes_cfg(u, batch2, n_cond) bytes. */
size_t pf_unet_workspace_bytes_cfg(const pf_unet* u, int batch2, int n_cond);
int pf_unet_forward_cfg(pf_unet* u, const float* x, const int64_t* t, const float* cond, int batch2, int n_cond,
                        const pf_unet_prepared* prep, float* eps2, void* workspace, size_t workspace_bytes, void* stream);
int pf_unet_n_launches_cfg(const pf_unet* u, int batch2, int n_cond, int has_time, int has_cross);
/* The same plan over `groups` stacked evaluations of one x (groups = 2: exactly the three entries above; groups = 3: dual guidance, the rows
 * of cat([uncond, partial, cond]) - pf_cfg_combine3).  The shared prefix runs on batch_total / groups samples, the hand-over copies the running
 * tensor (and its statistics) `groups` times, shared skips are read modulo batch_total / groups.  x: [batch_total / groups, ...]; t, cond (and
 * prep->cross_bias): batch_total rows, every group carrying the same t.  groups outside {2, 3} or batch_total % groups != 0: PF_EINVAL from the
 * forward (nothing is launched), 0 from the two queries. */
size_t pf_unet_workspace_bytes_cfgn(const pf_unet* u, int batch_total, int groups, int n_cond);
int pf_unet_forward_cfgn(pf_unet* u, const float* x, const int64_t* t, const float* cond, int batch_total, int groups, int n_cond,
                         const pf_unet_prepared* prep, float* eps, void* workspace, size_t workspace_bytes, void* stream);
int pf_unet_n_launches_cfgn(const pf_unet* u, int batch_total, int groups, int n_cond, int has_time, int has_cross);
/* kernel launches of one forward; has_time / has_cross: with that member of pf_unet_prepared supplied */
int pf_unet_n_launches_prepared(const pf_unet* u, int batch, int n_cond, int has_time, int has_cross);

/* Plan options, per handle (default PF_OPT_AUTO for all): which of two equivalent kernel forms the plan launches.
 *   PF_OPT_MLP_FUSED  - transformer feed-forward (+ proj_out) as ONE launch per 64-token tile vs LayerNorm planes + GeGLU GEMM + FF-out
 *                       GEMM + proj_out (bit-identical results); auto: fused when its last round of workgroups is >= 85 % full
 *   PF_OPT_ATTN_WIDE  - self-attention with 256-query vs 128-query workgroups (equal up to summation order); auto: 256 when L % 256 == 0
 *                       and that still gives 3/4 of the CUs a workgroup
 *   PF_OPT_CONV_T16   - 16x16-pixel tile for the 64-output-channel 3x3 convs with >= 128 input channels vs the 8x16 tile
 *   PF_OPT_CONV_PP    - 3x3 convs whose 128-wide tiles give every CU at most one workgroup (B = 16: the 32x32 level) as 8-wave workgroups:
 *                       two wave groups split K and run half a tap apart, one loading while the other computes (equal up to summation order)
 *   PF_OPT_CONV_WINO  - ResBlock 3x3 convs in the fused Winograd F(2x2, 3x3) form (pf_conv_args.wino; bf16x3 / f16x3 modes; equal to the direct
 *                       form up to rounding, 2.25x fewer matrix operations) vs the direct implicit GEMM; auto: where it measured faster
 *                       (profiles/r06_ab_winograd.md: input channels >= 192, or >= 128 at 32x32 and below); on: every conv that qualifies */
enum { PF_OPT_MLP_FUSED = 0, PF_OPT_ATTN_WIDE = 1, PF_OPT_CONV_T16 = 2, PF_OPT_CONV_PP = 3, PF_OPT_CONV_WINO = 4, PF_OPT_COUNT = 5 };
enum { PF_OPT_AUTO = -1, PF_OPT_OFF = 0, PF_OPT_ON = 1 };
int pf_unet_set_option(pf_unet* u, int option, int value);
/* Range telemetry.  `device_word` (4 bytes of caller-owned device memory, zeroed by the caller; NULL switches it off): while bound, every forward
 * max-combines into it - as an fp32 bit pattern, NaN / inf kept - the largest |value| of every tensor its layers store: block outputs, the residual
 * stream, q | k | v, GeGLU products (the fused feed-forward / pre-attention launches are replaced by their bit-identical chains while it is bound).
 * Each of those is, after at most a normalisation, the split A operand of a following layer; the fp16-piece build (f16x3) overflows beyond 65504,
 * so 65504 / *device_word is the run's headroom - measured in ANY arithmetic mode (in f32 nothing overflows while measuring).  inference_sdf's
 * `--precision auto` reads it from its f32 probe before it considers f16x3; bench.py prints it (f16x3_mode.max_abs_activation). */
int pf_unet_track_absmax(pf_unet* u, void* device_word);
int pf_unet_get_option(const pf_unet* u, int option);

/* Per-launch profiling: when enabled, forward brackets every kernel launch with hipEvents
 * on the launch stream.  pf_unet_profile_read synchronises those events and returns, per
 * launch: a kernel-family id (PF_K_*), elapsed ms and the algorithmic FLOPs of the launch. */
enum { PF_K_CONV3 = 0, PF_K_GEMM = 1, PF_K_ATTN = 2, PF_K_GNSTAT = 3, PF_K_LNSTAT = 4, PF_K_SMALL = 5, PF_K_COUNT = 6 };
int pf_unet_set_profiling(pf_unet* u, int enabled);
int pf_unet_profile_read(pf_unet* u, int* kind, float* ms, double* flops, int capacity);
/* the same launches' operation counts in the DIRECT form of each layer: equal to `flops` except for Winograd launches (PF_OPT_CONV_WINO), whose
 * `flops` are the 16 / 36 actually executed - keeps achieved rates comparable between plans (bench.py: direct_equivalent_tflops) */
int pf_unet_profile_read_direct(pf_unet* u, double* direct_flops, int capacity);
int pf_unet_n_launches(const pf_unet* u, int batch, int n_cond);

/* ---- sampler steps (elementwise, NCHW fp32, n = B*C*H*W elements) -------------------------
 * Classifier-free guidance combine (DiffusionSampler.get_eps, stable_diffusion/sampler/__init__.py:69-77):
 *   eps = e_uncond + scale * (e_cond - e_uncond), where eps2 = [e_uncond ; e_cond] (2n elements). */
int pf_cfg_combine(const float* eps2, float scale, float* eps, size_t n, void* stream);
/* Dual guidance combine (not in the reference): eps3 = [e0 ; e1 ; e2] (3n elements) - both parts of a two-part condition dropped, the first
 * part kept, both kept:
 *   eps = (e0 + s1 * (e1 - e0)) + s2 * (e2 - e1)     five individually rounded fp32 operations in this order
 * With e1 == e2 these are pf_cfg_combine's bits on [e0 ; e1] with scale s1 (finite values).  16-byte vectors when eps3 and eps are 16-byte
 * aligned and n % 4 == 0, 4-byte elements otherwise: the same bits. */
int pf_cfg_combine3(const float* eps3, float s1, float s2, float* eps, size_t n, void* stream);
/* Guidance rescale (not in the reference; Lin, Liu, Li & Yang 2024, "Common Diffusion Noise Schedules and Sample Steps Are Flawed", section 3.4;
 * its companion on the host, the guidance interval, is Kynkaanniemi et al. 2024, "Applying Guidance in a Limited Interval Improves Sample and
 * Distribution Quality" - DESIGN.md 0, row a42, and 3, "Guidance rescale and interval").  At a high scale the combined prediction has a much
 * larger per-sample standard deviation than the conditional one; this scales it back and mixes the result with the plain combine by phi.
 * epsg is [groups][rows][row_elems], group-major as pf_cfg_combine / pf_cfg_combine3 read it; per row r:
 *     e_cfg[i] = pf_cfg_combine's expression (s1)        groups == 2      the same device functions, so the same individually
 *              = pf_cfg_combine3's expression (s1, s2)   groups == 3      rounded fp32 operations as those launches
 *     e_pos[i] = the fully conditional group: the last one
 *     four sums over the row: e_pos, e_pos^2, e_cfg, e_cfg^2        every term widened to float64 first (squares exact); every addition in
 *                                                                   double-double (its rounding error kept), the total rounded to float64:
 *                                                                   within an ulp of the exact sum, i.e. within 2^-52 * sum |term|
 *     var = sum x^2 / n - (sum x / n)^2 ;  f = sqrt(var_pos / var_cfg)                                 float64, each operation rounded
 *     f = 1  when var_cfg is not > 0 or the root is not finite (a constant row; a quotient that is NaN, overflowed, or negative
 *            because var_pos cancelled below zero): a stated rule, like pf_slerp_rows' lerp weights - there is no scale to restore
 *     w = phi*f + (1 - phi)  in float64, rounded to float ONCE ;  eps[r][i] = fl(e_cfg[i] * w)         one rounded product
 *   which is the published phi*(e_cfg*f) + (1 - phi)*e_cfg, factored: a row with f == 1 has w == 1 and comes out as e_cfg bit for bit.
 *   Two launches without a host sync, workgroup = (row, PF_MSE_CHUNK of it), as pf_slerp_rows.  Reduce: the four sums in the lane / butterfly /
 *   wave order of pf_invert_step's residual, one partial 4-tuple of (hi, lo) pairs per workgroup into `workspace` (pf_cfg_rescale_workspace_bytes(rows,
 *   row_elems) bytes, 8-byte aligned: double [rows][chunks][4][2], which the call leaves behind); no atomics.  Combine: every workgroup of a row adds the row's 4-tuples in chunk order - the same four
 *   doubles in each -, forms w, recomputes e_cfg from one more read of the groups and writes its chunk: (2*groups + 1) * n * 4 bytes move.
 *   The chunk-0 workgroup of a row also writes stats[row] and weights[row].  A row's outputs depend on that row alone: bit-identical from
 *   call to call and however the rows are split into calls.  epsg and eps 16-byte aligned with row_elems % 4 == 0 are moved as 16-byte
 *   vectors, anything else element by element; the same operations, so the same bits.
 * Refused before any launch (message prefix "cfg_rescale: "): null epsg or eps; groups outside {2, 3}; rows <= 0 or row_elems == 0; phi NaN
 * or outside [0, 1]; eps overlapping epsg, partially too; no workspace, one too small or not 8-byte aligned; stats not 8-byte aligned; more
 * workgroups than one launch holds (rows * chunks >= 2^31). */
typedef struct pf_cfg_rescale_args {
  const float* epsg;                  /* [groups][rows][row_elems] */
  float* eps;                         /* [rows][row_elems]; may not overlap epsg */
  double* stats;                      /* [rows][3] device doubles: var_pos, var_cfg, f; may be NULL */
  float* weights;                     /* [rows] device floats: the w actually used; may be NULL */
  void* workspace; size_t workspace_bytes;
  double phi;                         /* the mix factor, in [0, 1]; 0 gives the plain combine's bits (at the cost of both launches) */
  float s1, s2;                       /* guidance scales: s1 always, s2 with groups == 3 */
  int32_t groups, rows; size_t row_elems;
} pf_cfg_rescale_args;
size_t pf_cfg_rescale_workspace_bytes(int rows, size_t row_elems);
int pf_cfg_rescale(const pf_cfg_rescale_args* a, void* stream);
/* Bounding the predicted clean image (not in the reference; static clipping is clip_denoised of Ho, Jain & Abbeel 2020, dynamic thresholding
 * is Saharia et al. 2022, "Photorealistic Text-to-Image Diffusion Models with Deep Language Understanding", section 2.3 - DESIGN.md 0, row
 * a43, and 3, "Clipping and dynamic thresholding").  Every sampler family consumes eps, so the operation rewrites eps: per row r (a batch
 * entry, or a song canvas under a window plan) eps becomes the eps' whose predicted x0 is the bounded one.  Per element, fp32, every
 * operation individually rounded, no contraction:
 *     (cx, ce, kx, k0) = table[clamp(t[r * t_stride], 0, n_table - 1)]    1/sqrt(ab), sqrt(1-ab)/sqrt(ab), 1/sqrt(1-ab), sqrt(ab)/sqrt(1-ab)
 *     x0  = fl(fl(cx*x) - fl(ce*eps))
 *     mode 0 (clip):     x0' = x0 < lo ? lo : x0 > hi ? hi : x0                           (a NaN x0 stays NaN)
 *     mode 1 (dynamic):  u = fl(x0 - c), c = float((lo + hi)/2), h = (hi - lo)/2 in float64
 *                        q = the p-quantile of |u| over the row, torch.quantile's linear rule in float64: pos = p*(row_elems - 1),
 *                            k = floor(pos), q = a_(k) + (pos - k)*(a_(k+1) - a_(k)), a_(n) := a_(n-1); the order statistics are exact
 *                            (a radix select over the uint32 patterns of |u|: -0 counts as +0, NaN sorts above inf), ties included
 *                        s = min(max(q, h), s_max*h) in float64
 *                        s == h        the row is mode 0's row, bit for bit
 *                        q not finite  eps' = eps for the whole row (a stated rule; stats then hold s = NaN, w = 1, count 0)
 *                        otherwise     w = float(h/s), rounded once; x0' = fl(c + fl(clamp(u, -float(s), float(s)) * w))
 *     eps' = (x0' == x0) ? eps : fl(fl(kx*x) - fl(k0*x0'))                                untouched elements come through bit for bit
 *   stats (optional) [rows][4] device doubles: q, s, w and the number of elements with x0' != x0 (an integer; exact); mode 0: NaN, NaN, 1, count.
 *   Two forms with the same bits, chosen by `form` (0: resident when row_elems <= PF_X0T_RESIDENT_MAX, else streamed; 1, 2: forced):
 *     resident  ONE launch, a workgroup of 1024 lanes per row: x and eps are read once into registers, the keys staged in LDS (4 bytes
 *               per element, up to 128 KiB), four 8-bit histogram passes with integer LDS atomics (order-free), eps' written once.
 *     streamed  workgroup = (row, PF_MSE_CHUNK of it): four histogram launches (one per 8-bit digit; per-chunk partials in `workspace`,
 *               added in chunk order, no global atomics), one apply launch, and with stats one launch adding the per-chunk counts:
 *               5 launches (6 with stats) in mode 1, 1 (2 with stats) in mode 0, whatever the data.
 *   No host sync, no allocation, capturable.  A row's result depends on that row alone.  x (with x_row_stride % 4 == 0), eps and eps_out
 *   16-byte aligned with row_elems % 4 == 0 are moved as 16-byte vectors, anything else element by element: the same bits.
 *   workspace: pf_x0_threshold_workspace_bytes(rows, row_elems, form) bytes, 8-byte aligned (0 for the resident form: none needed).
 * Refused before any launch (message prefix "x0_threshold: "): null x, eps, eps_out, t or table; rows <= 0 or row_elems == 0 (or >= 2^32);
 * x_row_stride < row_elems; t_stride < 0 or n_table <= 0; lo >= hi or either not finite; p NaN or outside (0, 1]; s_max < 1 or NaN; an
 * unknown mode or form; form 1 with row_elems > PF_X0T_RESIDENT_MAX; eps_out overlapping eps partially (eps_out == eps is in place), or x,
 * table or t at all; a needed workspace that is missing, too small or not 8-byte aligned; stats not 8-byte aligned; more workgroups than
 * one launch holds (rows * chunks >= 2^31). */
#define PF_X0T_RESIDENT_MAX 32768
typedef struct pf_x0_threshold_args {
  const float* x; size_t x_row_stride;      /* the state eps was predicted from; may carry cond_concat channels behind the first row_elems */
  const float* eps; float* eps_out;         /* [rows][row_elems]; eps_out == eps (in place) or disjoint */
  const int64_t* t; int32_t t_stride;       /* device; row r reads t[r * t_stride] */
  const float* table; int32_t n_table;      /* device, [n_table][4] */
  double* stats;                            /* may be NULL */
  void* workspace; size_t workspace_bytes;
  double p, s_max; float lo, hi;            /* p in (0, 1]; s_max >= 1 or +inf; lo < hi */
  int32_t mode, form, rows; size_t row_elems;
} pf_x0_threshold_args;
size_t pf_x0_threshold_workspace_bytes(int rows, size_t row_elems, int form);
int pf_x0_threshold(const pf_x0_threshold_args* a, void* stream);

/* Steering a population of candidates while it is sampled (not in the reference; Feynman-Kac / SMC steering of a diffusion sampler,
 * Singhal et al. 2025; the twisted diffusion sampler of Wu et al. 2023 - DESIGN.md 0, row a44, and 3, "Steering by resampling").  Every
 * few reverse steps the predicted clean image of every candidate is scored (pf_x0_predict, then pf_roll_stats and float64 on the device),
 * each group of n candidates is resampled in proportion to exp(lambda * reward gain) (pf_steer_resample) and the state rows are moved to
 * their survivors (pf_rows_gather).  None of the three has atomics, allocates or syncs with the host; all are capturable.
 *
 * pf_x0_predict: x0[r][i] = fl(fl(cx*x[r][i]) - fl(ce*eps[r][i])), (cx, ce) = table[clamp(t[r * t_stride], 0, n_table - 1)][0:2] - the table
 *   and the very device function of pf_x0_threshold (csrc/x0_predict.h), fp32, every operation individually rounded.  x (with
 *   x_row_stride % 4 == 0), eps and x0 16-byte aligned with row_elems % 4 == 0 are moved as 16-byte vectors, anything else element by
 *   element: the same bits.  Refused before any launch (message prefix "x0_predict: "): a null pointer; rows <= 0 or row_elems == 0;
 *   x_row_stride < row_elems; t_stride < 0 or n_table <= 0; x0 overlapping x, eps, t or table. */
typedef struct pf_x0_predict_args {
  const float* x; size_t x_row_stride;      /* the state eps was predicted from; may carry cond_concat channels behind the first row_elems */
  const float* eps;                         /* [rows][row_elems] */
  const int64_t* t; int32_t t_stride;       /* device; row r reads t[r * t_stride] */
  const float* table; int32_t n_table;      /* device, [n_table][4] */
  float* x0;                                /* [rows][row_elems], disjoint from every input */
  int32_t rows; size_t row_elems;
} pf_x0_predict_args;
int pf_x0_predict(const pf_x0_predict_args* a, void* stream);
/* pf_steer_resample: one workgroup per group of n particles, 1 <= n <= PF_STEER_MAX_N.  Every float64 operation below is rounded on its own,
 * never contracted; sums are added serially in index order.  Per group G (global index g = group_offset + G), particles i = 0 .. n - 1:
 *   1. lw_i = fl(lambda * fl(reward_i - base_i)); a particle whose reward_i or lw_i is not finite gets w_i = 0
 *   2. m = the maximum of the finite lw_i, w_i = exp(fl(lw_i - m))                         (weights[]; the exponential claims <= 1 ulp)
 *   3. S = sum w_i, Q = sum w_i^2 (c_i: the running sum of S after particle i), ESS = fl(fl(S*S) / Q)
 *   4. flag 2: no particle has a finite weight - ancestors are the identity, base is unchanged (ESS is 0/0 = NaN)
 *   5. flag 0: ESS <= fl(ess_frac * n) does not hold - ancestors are the identity, base is unchanged
 *   6. flag 1: systematic resampling - u = c0 * 2^-32, c0 the first output word of Philox4x32-10 with counter (g lo, g hi, event lo,
 *      event hi) and key (seed lo, seed hi ^ 0x53544552); step = fl(S / n); p_j = fl(fl(double(j) + u) * step); a_j = the first i with
 *      c_i > p_j, clamped to n - 1; then base_j <- reward_(a_j)
 *   stats [groups][4]: ESS, S, the flag, u (u is written whatever the flag).
 * What follows from the rule: the key is tagged, so the steering stream is disjoint from every noise stream of the same seed and consumes no
 * draw - an unsteered run keeps its bits.  u has 32 bits, so j + u is exact, and p_j <= (n - 2^-32) * (S/n) * (1 + 2^-53)^2 < S for
 * n <= 256 < 2^20: the clamp never acts and, c being non-decreasing, c_(a_j) > p_j >= c_(a_j - 1) - a zero-weight particle is never chosen.
 * Equal weights (w_i = 1, c_i = i + 1, step = 1) give the identity for every u.  ancestors are group-local.
 * Refused before any launch (message prefix "steer_resample: "): a null pointer; groups <= 0; n outside [1, PF_STEER_MAX_N]; lambda negative
 * or not finite; ess_frac NaN or outside (0, 1]; a misaligned pointer (8 bytes; ancestors 4); any two of the five arrays overlapping. */
#define PF_STEER_MAX_N 256
typedef struct pf_steer_resample_args {
  const double* reward;                     /* [groups * n], device */
  double* base;                             /* [groups * n], read and - on flag 1 - written */
  double lambda, ess_frac;
  uint64_t seed, group_offset, event;       /* group_offset: global index of the first group; event: steering events so far */
  int32_t* ancestors;                       /* [groups * n], group-local */
  double* weights;                          /* [groups * n] */
  double* stats;                            /* [groups][4]: ESS, sum of weights, flag, u */
  int32_t groups, n;
} pf_steer_resample_args;
int pf_steer_resample(const pf_steer_resample_args* a, void* stream);
/* pf_rows_gather: for up to PF_GATHER_MAX_TENSORS tensors k in one launch, rows of row_elems[k] floats, `per` images per particle:
 *   dst_k[(G*n + j)*per + s][:] = src_k[(G*n + clamp(ancestors[G*n + j], 0, n - 1))*per + s][:]
 * The clamp is inside the kernel: a corrupt table cannot make it read outside its inputs.  dst is disjoint from src (the host ping-pongs);
 * workgroup = (row, PF_MSE_CHUNK of the longest row); a tensor whose src and dst are 16-byte aligned with row_elems % 4 == 0 moves as
 * 16-byte vectors, any other element by element.  Refused before any launch (message prefix "rows_gather: "): null ancestors, src or dst; n_tensors
 * outside [1, PF_GATHER_MAX_TENSORS]; groups <= 0, n < 1 or per < 1; row_elems == 0 or >= 2^32; a misaligned pointer (4 bytes); a dst
 * overlapping any src, another dst or ancestors; more workgroups than one launch holds (rows * chunks >= 2^31). */
#define PF_GATHER_MAX_TENSORS 4
typedef struct pf_rows_gather_args {
  const float* src[PF_GATHER_MAX_TENSORS]; float* dst[PF_GATHER_MAX_TENSORS];
  size_t row_elems[PF_GATHER_MAX_TENSORS];
  int32_t n_tensors;
  const int32_t* ancestors;                 /* [groups * n], group-local */
  int32_t groups, n, per;
} pf_rows_gather_args;
int pf_rows_gather(const pf_rows_gather_args* a, void* stream);

/* Overlapping windows along the time axis (not in the reference; MultiDiffusion, Bar-Tal et al. 2023, on the rows of a piano roll): a song is
 * a canvas [songs][channels][canvas_h][width], canvas_h = stride * (n_windows - 1) + win_h, and the denoiser sees it as the batch of its
 * n_windows windows of win_h rows.  Window j of song s is batch row s * n_windows + j (song-major) and canvas rows [j * stride, j * stride + win_h).
 * Canvas row y is covered by the windows j with 0 <= y - j * stride < win_h, taken in ascending j; k(y) is their number.
 *   pf_window_split: windows[s * n_windows + j][c][r][w] = canvas[s][c][j * stride + r][w]      (a copy; `channels` is whatever the canvas carries)
 *   pf_window_merge: the windows' noise predictions back onto the canvas, with the guidance combine folded in.  eps is
 *     [groups][songs * n_windows][channels][win_h][width], group-major as the guided evaluation stacks it.  Per canvas element, in fp32, every
 *     operation individually rounded and in this order:
 *       e_j = eps                                     groups == 1
 *           = pf_cfg_combine's expression (scale s1)   groups == 2      the same device functions, so the same bits as the combine
 *           = pf_cfg_combine3's expression (s1, s2)    groups == 3      launch followed by a groups == 1 merge
 *       k(y) == 1:  out = e_j                          a select, not w*e/w: a row one window owns comes through bit for bit
 *       otherwise:  num = w_0*e_0, num += w_j*e_j ; den = w_0, den += w_j ; out = num / den        w_j = row_weight[y - j * stride]
 *     row_weight: win_h floats on the device, all > 0 (ones: the plain mean).
 * Both are gathers over their output - no atomics, no shared memory, nothing order-dependent - so a launch is bit-reproducible.  16-byte
 * vectors along width when width % 4 == 0 and every pointer is 16-byte aligned, 4-byte elements otherwise: the same bits.  Refused before
 * any launch (message prefix "window_split: " / "window_merge: "): a non-positive extent, stride < 1, stride > win_h (rows would belong to
 * no window), ceil(win_h / stride) > 8, null pointers, an output that overlaps an input, groups outside 1..3. */
int pf_window_split(const float* canvas, float* windows, int songs, int channels, int win_h, int width, int n_windows, int stride, void* stream);
typedef struct pf_window_merge_args {
  const float* eps;                   /* [groups][songs * n_windows][channels][win_h][width] */
  const float* row_weight;            /* [win_h], device memory, every weight > 0 */
  int groups;                         /* 1, 2 or 3 */
  float s1, s2;                       /* guidance scales: s1 with groups >= 2, s2 with groups == 3 */
  int songs, channels, win_h, width, n_windows, stride;
  float* out;                         /* [songs][channels][canvas_h][width]; must not overlap eps or row_weight */
} pf_window_merge_args;
int pf_window_merge(const pf_window_merge_args* a, void* stream);

/* One reverse step of a sampler family as ONE elementwise kernel (DDPM / RePaint and DDIM here; DPM-Solver++(2M) follows them below).  The caller zero-fills the struct and sets what it needs.
 *   DDPM / RePaint (SDFSampler.paint body + p_sample, sampler_sdf.py:80-171,307-336):
 *     x0    = c_recip*x - c_recipm1*eps ; mean = c_x0*x0 + c_xt*x ; x_unkn = mean + sigma*noise_p
 *     x_kn  = sqrt_ab*orig + sqrt_1mab*noise_q          (skipped when orig == NULL)
 *     x_out = x_kn*mask + x_unkn*(1-mask)
 *   DDIM (DDIMSampler.get_x_prev_and_pred_x0 + paint blend, sampler_ddim.py:220-272,355-359):
 *     pred_x0 = (x - s1m*eps)/sqrt_a ; x_prev = sqrt_aprev*pred_x0 + dir_coef*eps + sigma*noise
 *     if orig: x_prev = (q_sqrt_a*orig + q_s1m*orig_noise)*mask + x_prev*(1-mask)
 * Two independent choices:
 *   coefficients - `coef` (host memory, copied at the call) or `table` + `state` (device memory: row state->index of a table with one
 *     coefficient struct per step, what a captured step reads - see pf_step_state below).  Exactly one of the two.
 *   noise - tensors (rng == 0; a NULL tensor means the term is absent: step 0, eta = 0), or drawn INSIDE the kernel (rng == 1): element i
 *     of draw d is exactly what pf_randn(seed, d, elem_offset) writes at i, so the result is bit-identical to pf_randn + the tensor form,
 *     without the noise tensors' round trip through HBM.  rng always adds the sigma term.  DDPM draws noise_q (draw_q) only with a known
 *     region and noise_p (draw_p) always - the reference's order is q then p (sampler_sdf.py:317-321, 153-160); DDIM draws `draw`
 *     (orig_noise stays a tensor: the reference's DDIM paint re-uses one fixed tensor).  With `state` the draw indices come from the
 *     device: DDPM (q, p) = (state->draws, state->draws + 1), p = state->draws without a known region; DDIM draw = state->draws.
 *     rng needs n and elem_offset to be multiples of 4 (one Philox call = 4 normals) and 16-byte aligned tensors. */
typedef struct pf_ddpm_coef { float c_recip, c_recipm1, c_x0, c_xt, sigma, sqrt_ab, sqrt_1mab; } pf_ddpm_coef;
typedef struct pf_ddim_coef { float s1m, sqrt_a, sqrt_aprev, dir_coef, sigma, q_sqrt_a, q_s1m; } pf_ddim_coef;
typedef struct pf_step_state { int64_t index; uint64_t draws; } pf_step_state;
typedef struct pf_ddpm_step_args {
  const float *x, *eps;               /* [n] */
  const float *orig, *mask;           /* known region: both or neither */
  const float *noise_p, *noise_q;     /* noise tensors, NULL = no such term (rng == 0 only) */
  int rng;                            /* 1: both draws made in the kernel; noise_p / noise_q must be NULL */
  const pf_ddpm_coef* coef;           /* host coefficients, copied at the call ...            */
  const pf_ddpm_coef* table;          /* ... or a device table, row state->index              */
  const pf_step_state* state;         /* device step state: required with table; with rng it also supplies the draw indices */
  uint64_t seed, draw_q, draw_p, elem_offset;   /* rng only; draw_* ignored when state is set */
  float* x_out; size_t n;             /* x_out may alias x */
} pf_ddpm_step_args;
int pf_ddpm_step(const pf_ddpm_step_args* a, void* stream);
typedef struct pf_ddim_step_args {
  const float *x, *eps;               /* [n] */
  const float *orig, *orig_noise, *mask;   /* known region: all three or none */
  const float *noise;                 /* noise tensor, NULL = no sigma term (rng == 0 only) */
  int rng;                            /* 1: the draw is made in the kernel; noise must be NULL */
  const pf_ddim_coef* coef;           /* host coefficients, copied at the call ...            */
  const pf_ddim_coef* table;          /* ... or a device table, row state->index              */
  const pf_step_state* state;         /* device step state: required with table; with rng it also supplies the draw index */
  uint64_t seed, draw, elem_offset;   /* rng only; draw ignored when state is set */
  float* x_out; size_t n;             /* x_out may alias x */
} pf_ddim_step_args;
int pf_ddim_step(const pf_ddim_step_args* a, void* stream);

/* DPM-Solver++(2M), the third family: the second-order multistep solver of the probability-flow ODE in its data-prediction form (Lu et al.,
 * "DPM-Solver++", 2022, algorithm 2), one denoiser evaluation per step like DDIM.  With alpha = sqrt(ab), sigma = sqrt(1 - ab),
 * lambda = log(alpha / sigma) and h = lambda(target) - lambda(current), one step is
 *     x0    = (x - s1m*eps) / sqrt_a                      this step's data prediction (written to x0_out when that is set)
 *     x_out = c_x*x + c_0*x0 + c_1*x0_prev                the c_1 term only when c_1 != 0
 *     if orig: x_out = (q_sqrt_a*orig + q_s1m*orig_noise)*mask + x_out*(1-mask)         the known-region blend of the DDIM family
 * The host folds everything else into the three coefficients, in float64, rounded once:
 *     c_x = sigma_tgt / sigma_cur,  c_0 = -alpha_tgt*expm1(-h)*(1 + 1/(2r)),  c_1 = +alpha_tgt*expm1(-h)/(2r),  r = h_previous / h
 * and a first-order step (the first of a loop, order 1, a repeated time step with h == 0, the lower-order last step) has c_1 == 0 and
 * c_0 = -alpha_tgt*expm1(-h): it is the DDIM step with eta = 0.  c_1 == 0 means x0_prev is NOT READ (a select, not a product with zero:
 * the history of a first step is uninitialised memory), so it may be NULL then; c_1 != 0 with x0_prev == NULL is refused when the
 * coefficients come by value; with a device table the host cannot see the row, and the kernel leaves the term out (memory safety only).  The step draws no noise and uses
 * state->draws for nothing.  Tensors that are all 16-byte aligned with n % 4 == 0 are moved as 16-byte vectors, anything else element by
 * element; both evaluate the same individually rounded operations, so the bits do not depend on the path. */
typedef struct pf_dpm_coef {
  float s1m;                          /* sqrt(1 - ab) of the current time step */
  float sqrt_a;                       /* sqrt(ab) of the current time step */
  float c_x, c_0, c_1;                /* as above; c_1 == 0: first-order step */
  float q_sqrt_a, q_s1m;              /* known-region forward noising at this index: sqrt(ab), sqrt(1 - ab) of the current time step, as pf_ddim_coef */
} pf_dpm_coef;
typedef struct pf_dpm_step_args {
  const float *x, *eps;               /* [n] */
  const float *x0_prev;               /* [n] the previous step's x0; read only when c_1 != 0 */
  float* x0_out;                      /* [n] receives this step's x0; may alias x0_prev; NULL = not kept */
  const float *orig, *orig_noise, *mask;   /* known region: all three or none */
  const pf_dpm_coef* coef;            /* host coefficients, copied at the call ...            */
  const pf_dpm_coef* table;           /* ... or a device table, row state->index              */
  const pf_step_state* state;         /* device step state: required with table */
  float* x_out; size_t n;             /* x_out may alias x */
} pf_dpm_step_args;
int pf_dpm_step(const pf_dpm_step_args* a, void* stream);

/* The stochastic form of DPM-Solver++(2M) (SDE-DPM-Solver++(2M) of Lu et al., "DPM-Solver++", section 5 / appendix; the midpoint form other
 * toolkits call "DPM++ 2M SDE"; DESIGN.md 3, "Stochastic DPM-Solver++(2M)"), with one more parameter eta >= 0 that the host folds into the
 * coefficients.  In the notation above,
 *     x0    = (x - s1m*eps) / sqrt_a
 *     x_out = c_x*x + c_0*x0 + c_1*x0_prev + sigma_n*z          z ~ N(0, 1); the c_1 term only when c_1 != 0, the noise only when sigma_n != 0
 *     if orig: x_out = (q_sqrt_a*orig + q_s1m*orig_noise)*mask + x_out*(1-mask)
 *     c_x = (sigma_tgt / sigma_cur)*exp(-eta*h),  E = -alpha_tgt*expm1(-(1 + eta)*h),  c_0 = E*(1 + 1/(2r)),  c_1 = -E/(2r),
 *     sigma_n = sigma_tgt*sqrt(-expm1(-2*eta*h))
 * eta = 0 gives the coefficients of pf_dpm_step with sigma_n = 0; eta = 1 is the SDE solver; a first-order row has c_1 = 0 and c_0 = E.
 * For every eta: c_x*alpha_cur + c_0 + c_1 = alpha_tgt and c_x^2*sigma_cur^2 + sigma_n^2 = sigma_tgt^2 - a step fed the true x0 maps the
 * marginal at the current time step onto the marginal at the target.
 *   Both conditions are uniform over the launch and are selects, not products with zero: c_1 == 0 - x0_prev is NOT READ (it may be NULL or
 * uninitialised); sigma_n == 0 - the noise tensor is NOT READ and no Philox call is made, and the result has the bits of pf_dpm_step on
 * the same inputs.  By value, c_1 != 0 without x0_prev and sigma_n != 0 with neither `noise` nor `rng` are refused; with a device table
 * the host cannot see the row, and the kernel leaves the term out (memory safety only).
 *   Noise as in pf_ddim_step: a tensor (rng == 0), or drawn INSIDE the kernel (rng == 1) - a lane owns one Philox group of four, element i
 * of draw d is exactly what pf_randn(seed, d, elem_offset) stores at i, so the result is bit-identical to pf_randn + the tensor form.
 * With `state` the draw index is state->draws.  rng needs n and elem_offset to be multiples of 4 and 16-byte aligned tensors; orig_noise
 * stays a tensor.  Without rng, tensors that are all 16-byte aligned with n % 4 == 0 are moved as 16-byte vectors, anything else element
 * by element; every operation is individually rounded, so the bits do not depend on the path.  x_out may alias x and x0_out may alias
 * x0_prev.  No atomics, no allocation, no host sync: the launch can be captured. */
typedef struct pf_dpm_sde_coef {
  float s1m;                          /* sqrt(1 - ab) of the current time step */
  float sqrt_a;                       /* sqrt(ab) of the current time step */
  float c_x, c_0, c_1;                /* as above; c_1 == 0: first-order step */
  float q_sqrt_a, q_s1m;              /* known-region forward noising at this index, as pf_dpm_coef */
  float sigma_n;                      /* standard deviation of the step's fresh noise; 0: no noise term */
} pf_dpm_sde_coef;
typedef struct pf_dpm_sde_step_args {
  const float *x, *eps;               /* [n] */
  const float *x0_prev;               /* [n] the previous step's x0; read only when c_1 != 0 */
  float* x0_out;                      /* [n] receives this step's x0; may alias x0_prev; NULL = not kept */
  const float *orig, *orig_noise, *mask;   /* known region: all three or none */
  const float *noise;                 /* noise tensor, read only when sigma_n != 0 (rng == 0 only) */
  int rng;                            /* 1: the draw is made in the kernel; noise must be NULL */
  const pf_dpm_sde_coef* coef;        /* host coefficients, copied at the call ...            */
  const pf_dpm_sde_coef* table;       /* ... or a device table, row state->index              */
  const pf_step_state* state;         /* device step state: required with table; with rng it also supplies the draw index */
  uint64_t seed, draw, elem_offset;   /* rng only; draw ignored when state is set */
  float* x_out; size_t n;             /* x_out may alias x */
} pf_dpm_sde_step_args;
int pf_dpm_sde_step(const pf_dpm_sde_step_args* a, void* stream);

/* Exact DDIM inversion (DESIGN.md 0, row "edit by inversion", and 3, "Exact DDIM inversion"; not in the reference): one iterate of one
 * UPWARD step of the eta = 0 DDIM ODE.  The DDIM step from x at level a down to level ap is F(x) = (x - c_e*eps(x)) / c_y with
 *     c_y = sqrt(a / ap),   c_e = sqrt(1 - a) - sqrt(a * (1 - ap) / ap)
 * (the host forms both in float64 and rounds once).  The x whose step lands exactly on y solves x = c_y*y + c_e*eps(x), and
 *     x_out = c_y*y + c_e*eps                              two products and one sum, each individually rounded
 * is one iterate of that fixed-point iteration, elementwise on [rows][row_elems]; eps is the denoiser at the previous iterate (at y for
 * the first one).  y, the state at the lower level, is fixed over the iterates: it is never written and may not alias x_out.  Coefficients
 * by value or from a device table, row state->index - exactly one of the two, as pf_ddim_step.  Tensors that are all 16-byte aligned with
 * row_elems % 4 == 0 are moved as 16-byte vectors, anything else element by element; the same operations, so the same bits.
 *   Fused residual (resid != NULL): the same launch also forms, per row b,
 *     resid[(slot * rows + b) * 2 + 0] = sum_i (x_out[b][i] - x_iter[b][i])^2        x_iter == NULL: the iterate is y
 *     resid[(slot * rows + b) * 2 + 1] = sum_i x_out[b][i]^2
 *   the difference in float32, squares and sums in float64.  x_iter is the previous iterate (read for the residual only; x_out may alias
 *   it).  A workgroup owns one PF_MSE_CHUNK of one row, reduces in a fixed order and writes one partial pair into `workspace`
 *   (pf_invert_step_workspace_bytes(rows, row_elems) bytes, 8-byte aligned); a second small launch adds a row's pairs in index order.  No
 *   atomics: a row's two sums depend on that row alone, bit-identical from call to call and however the batch is split into calls.
 *   slot = state->index * iters + k with a table (k, the iterate number, is a constant of a captured node), else `slot` by value; resid
 *   holds n_slots slots of [rows][2] doubles and a slot outside [0, n_slots) is refused (by value) or not written (from the device).
 *   The forward step's round-trip defect is the next residual over c_y: F(x_K) - y = (x_K - x_{K+1}) / c_y.
 * Refused before any launch: two coefficient sources or none, resid without workspace or with one too small, y overlapping x_out. */
typedef struct pf_invert_coef { float c_y, c_e; } pf_invert_coef;
typedef struct pf_invert_step_args {
  const float *y, *eps;               /* [rows][row_elems]: the lower state, the denoiser's output at the previous iterate */
  const float *x_iter;                /* [rows][row_elems] the previous iterate, read for the residual only; NULL: it is y */
  const pf_invert_coef* coef;         /* host coefficients, copied at the call ...            */
  const pf_invert_coef* table;        /* ... or a device table, row state->index              */
  const pf_step_state* state;         /* device step state: required with table; it also names the residual's slot */
  float* x_out;                       /* [rows][row_elems]; may alias x_iter, not y */
  double* resid;                      /* [n_slots][rows][2] device doubles; NULL: no residual, one launch */
  void* workspace; size_t workspace_bytes;      /* resid only */
  int32_t iters, k;                   /* resid with state: slot = state->index * iters + k */
  int64_t slot, n_slots;              /* resid: the slot by value (without state), and how many slots resid holds */
  int32_t rows; size_t row_elems;
} pf_invert_step_args;
size_t pf_invert_step_workspace_bytes(int rows, size_t row_elems);
int pf_invert_step(const pf_invert_step_args* a, void* stream);

/* A path between two noises (DESIGN.md 0, row "morph", and 3, "Morph"; not in the reference): `frames` points between the rows of a and
 * the rows of b, on the great circle through them (mode 0, slerp) or on the chord (mode 1, lerp),
 *     out[k][r][i] = fl(fl(w0*a[r][i]) + fl(w1*b[r][i]))      two products and one sum, each individually rounded
 * with one weight pair (w0, w1) per (frame k, row r).  Mode slerp forms them from the row's three sums
 *     aa = sum a*a, ab = sum a*b, bb = sum b*b                products exact in float64, sums in float64
 *     c = ab / sqrt(aa*bb), theta = acos(c), w0 = sin((1 - t[k])*theta) / sin(theta), w1 = sin(t[k]*theta) / sin(theta)
 * in float64 on the device, each weight rounded to float once; mode lerp takes (1 - t[k], t[k]) rounded to float.  A slerp row with
 * aa == 0, bb == 0 or 1 - |c| < 2^-20 takes the lerp weights: parallel rows, where slerp and lerp agree to O(theta^2) and sin(theta) has
 * no digits left, and antiparallel rows, where no great circle is defined.  A frame with t[k] == 0 is a copy of a and one with
 * t[k] == 1 a copy of b (a select, not arithmetic: bit-identical, -0.0f included).
 *   Mode slerp is two launches without a host sync.  Reduce: a workgroup owns one PF_MSE_CHUNK of one row, adds its three sums in the
 *   lane / butterfly / wave order of pf_invert_step's residual and writes one partial triple into `workspace`
 *   (pf_slerp_rows_workspace_bytes(rows, row_elems) bytes, 8-byte aligned); no atomics.  Combine: a workgroup owns one (row, chunk), adds
 *   its row's triples in chunk order - every workgroup of a row forms the same three doubles -, forms the weights and writes its chunk
 *   of ALL frames: a and b are read once, (2 + frames) * n * 4 bytes move.  The chunk-0 workgroup of a row also writes stats[row] and
 *   weights[:, row].  Mode lerp is the combine launch alone: no workspace, stats is not written.
 *   A row's outputs depend on that row alone: bit-identical from call to call and however the rows are split into calls.  Tensors that
 *   are all 16-byte aligned with row_elems % 4 == 0 are moved as 16-byte vectors, anything else element by element; the same operations,
 *   so the same bits.
 * Refused before any launch: null a, b, out or t; rows <= 0 or row_elems == 0; frames outside [1, PF_SLERP_MAX_FRAMES]; a t[k] that is
 * NaN or outside [0, 1]; another mode; out overlapping a or b, partially too; mode slerp without workspace, with one too small or not
 * 8-byte aligned; stats not 8-byte aligned; more workgroups than one launch holds. */
#define PF_SLERP_MAX_FRAMES 64
typedef struct pf_slerp_args {
  const float *a, *b;                 /* [rows][row_elems] the two endpoints */
  const double* t;                    /* HOST array of `frames` fractions in [0, 1], copied at the call */
  float* out;                         /* [frames][rows][row_elems]; may not overlap a or b */
  double* stats;                      /* [rows][3] device doubles: sum a*a, sum a*b, sum b*b; may be NULL; not written in mode lerp */
  float* weights;                     /* [frames][rows][2] device floats: the (w0, w1) actually used; may be NULL */
  void* workspace; size_t workspace_bytes;      /* mode slerp only */
  int32_t mode;                       /* 0 slerp, 1 lerp */
  int32_t frames, rows; size_t row_elems;
} pf_slerp_args;
size_t pf_slerp_rows_workspace_bytes(int rows, size_t row_elems);
int pf_slerp_rows(const pf_slerp_args* a, void* stream);

/* RePaint re-noise between inner repeats (sampler_sdf.py:337-341; keeps the reference's beta-not-sqrt quirk):
 *   x_t = a*x + b*noise */
int pf_axpby(const float* x, const float* noise, float a, float b, float* out, size_t n, void* stream);

/* Standard-normal noise, counter-based (Philox4x32-10 + Box-Muller), keyed by (seed, stream_id,
 * global element index) so results do not depend on how a batch is sharded over GPUs.
 * elem_offset = index of out[0] in the global (unsharded) tensor.
 * Philox counter = (g lo, g hi, stream_id lo, stream_id hi) with g = global element index >> 2, key = (seed lo, seed hi); element 4 g + j
 * takes normal j of (r0 cos t0, r0 sin t0, r1 cos t1, r1 sin t1), r = sqrt(-2 ln u), t = 2 pi u, from the pairs (u0, u1) and (u2, u3) of
 * u_i = ((float)(c_i >> 8) + 0.5f) * 2^-24.  The real range of u is [2^-25, 1], not (0, 1): from c_i >> 8 = 2^23 on the sum rounds to
 * even in float, and 2^24 - 1 gives u = 1.0 exactly.  So |out[i]| <= 5.887 (never infinite or NaN), and a pair with u0 = 1.0 - 2^-24 of
 * all pairs - is exactly (+-)0.  The stream is part of the interface (goldens and seeds depend on it) and stays as it is. */
int pf_randn(float* out, size_t n, uint64_t seed, uint64_t stream_id, uint64_t elem_offset, void* stream);

/* Measurement aid (bench.py): writes {shader-cycle counter, constant-rate reference counter} of the moment the probe kernel runs into
 * row x of out[8][2] for every XCD x (XCDs have counters and clocks of their own; rows of XCDs the part does not have stay
 * untouched); two probes around a stretch of stream work give the average shader clock each XCD sustained over it. */
int pf_clock_probe(uint64_t* out8x2, void* stream);
/* Measurement aid (bench.py): one launch that keeps the bf16 matrix pipe of every CU 100 % busy (8 waves per CU, dependency-free
 * v_mfma_f32_32x32x16_bf16 streams on operands with random signs / mantissas) for `iters` x 24 MFMAs per wave; *flops_out = the launch's
 * flops.  Timed with events it gives the rate the pipe SUSTAINS on this box under its power management - the reference
 * `roofline.sustained` of the bench line; `sink` is one float of device memory (never written in practice). */
int pf_mfma_probe(float* sink, int iters, double* flops_out, void* stream);

/* ---- replayable reverse step: everything that changes from one step to the next - the table row, the
 * time-step value fed to the denoiser, the noise draw counter - lives in a small device-resident pf_step_state, so ONE captured
 * hipGraph of {begin, pf_unet_forward, step, end} is replayed for every step of the loop (pf_ddpm_step / pf_ddim_step / pf_dpm_step with
 * `table` and `state`).  `time_steps` is the DDIM tau table (int32 per row; NULL: the row index itself is the time step, as in the DDPM sampler). */
int pf_step_state_set(pf_step_state* dev_state, int64_t index, uint64_t draws, void* stream);
int pf_step_begin(const pf_step_state* dev_state, const int32_t* time_steps, int64_t* t_out, int batch, void* stream);
int pf_step_end(pf_step_state* dev_state, int draws_used, void* stream);          /* index -= 1; draws += draws_used */
/* the end of a captured UPWARD step (pf_invert_step walks its table from row 0 up): index += delta; draws += draws_used */
int pf_step_advance(pf_step_state* dev_state, int64_t delta, int draws_used, void* stream);
int pf_randn_dev(float* out, size_t n, uint64_t seed, const pf_step_state* dev_state, int slot, uint64_t elem_offset, void* stream);

/* ---- the training objective, forward only: what LightningLearner.validation_step logs as val/loss (lightning_learner.py:41-52) through
 * LatentDiffusion.loss / DenoiseDiffusion.loss (stable_diffusion/latent_diffusion.py:203-240, ddpm/__init__.py:90-111).  Two memory-bound
 * launches around the denoiser; the caller zero-fills the structs and sets what it needs.  All memory is caller-owned device memory;
 * nothing is allocated and nothing synchronises.
 *
 * pf_qsample_rows - q_xt_x0 + q_sample with one time step PER SAMPLE (latent_diffusion.py:149-177, ddpm/__init__.py:36-64):
 *     x_t[b][i] = sqrt_ab[t[b]] * x0[b][i] + sqrt_1mab[t[b]] * noise[b][i]       rows samples of row_elems floats
 *   each product rounded, then the sum, as the reference's tensor operations.  sqrt_ab / sqrt_1mab are device tables of n_steps floats
 *   that the host builds in float32 as the reference does (alpha_bar ** 0.5, (1 - alpha_bar) ** 0.5); t[b] outside [0, n_steps) is
 *   clamped for memory safety only.  Noise: a tensor (rng == 0), or drawn in the kernel (rng == 1): element i of the [rows][row_elems]
 *   tensor is exactly what pf_randn(seed, draw, elem_offset) writes at i; rng needs row_elems and elem_offset to be multiples of 4 and
 *   16-byte aligned tensors.  noise_out (optional, rng == 1) receives the drawn noise.  x_t may alias x0. */
typedef struct pf_qsample_rows_args {
  const float* x0;                    /* [rows][row_elems] */
  const float* noise;                 /* [rows][row_elems]; rng == 0 only */
  const int64_t* t;                   /* [rows] */
  const float *sqrt_ab, *sqrt_1mab;   /* [n_steps] */
  int32_t n_steps;
  int rng;                            /* 1: the noise is drawn in the kernel; noise must be NULL */
  uint64_t seed, draw, elem_offset;   /* rng only */
  float* x_t;                         /* [rows][row_elems] */
  float* noise_out;                   /* optional, rng only */
  int32_t rows; size_t row_elems;
} pf_qsample_rows_args;
int pf_qsample_rows(const pf_qsample_rows_args* a, void* stream);
/* pf_mse_rows - the reduction of F.mse_loss(noise, eps_theta) (latent_diffusion.py:239-240, ddpm/__init__.py:110-111), kept per sample:
 *     row_sum[b] = sum_i (noise[b][i] - eps_theta[b][i])^2        into a device double[rows]
 *   the difference formed in float32, squared and accumulated in float64.  Noise: a tensor, or (rng == 1) RE-DRAWN in the kernel from the
 *   (seed, draw, elem_offset) that pf_qsample_rows used - a loss evaluation with library noise never writes or reads a noise tensor.
 *   The result is a function of the row's values alone: workgroup j of a row owns elements [j * PF_MSE_CHUNK, (j + 1) * PF_MSE_CHUNK),
 *   reduces them in a fixed order and leaves one partial in `workspace` (pf_mse_rows_workspace_bytes(rows, row_elems) bytes, 8-byte
 *   aligned); a second launch adds each row's partials in index order.  No atomics: bit-identical from call to call, between the two
 *   noise forms and however the batch is split into calls (with elem_offset advanced by the rows in front). */
#define PF_MSE_CHUNK 2048
typedef struct pf_mse_rows_args {
  const float* eps_theta;             /* [rows][row_elems] */
  const float* noise;                 /* [rows][row_elems]; rng == 0 only */
  int rng;                            /* 1: the noise is re-drawn in the kernel; noise must be NULL */
  uint64_t seed, draw, elem_offset;   /* rng only */
  double* row_sum;                    /* [rows] */
  void* workspace; size_t workspace_bytes;
  int32_t rows; size_t row_elems;
} pf_mse_rows_args;
size_t pf_mse_rows_workspace_bytes(int rows, size_t row_elems);
int pf_mse_rows(const pf_mse_rows_args* a, void* stream);
/* pf_chord_ce_rows - the three cross-entropies of Chord_8Bar.chord_loss (models/model_chd_8bar.py:21-39; ChordDecoder.recon_loss,
 *   dl_modules/chord_dec.py:72-85), kept per sample and not yet divided: from the logits root [rows][n_step][12], chroma
 *   [rows][n_step][12][2], bass [rows][n_step][12] and the chord matrix gt [rows][n_step][36],
 *     ce_rows[b][0..2] = sum over the row's steps of -log_softmax(logits)[target]   for root (12-way), chroma (12 two-way items a step), bass
 *   into a device double[rows][3]; the reference's means are ce_rows summed over b / (rows n_step), / (rows n_step 12) for chroma.
 *   Targets are the reference's: root / bass = arg-max of gt[..., 0:12] / gt[..., 24:36] (ties to the lowest index: an all-zero row
 *   targets 0), chroma = (long) gt[..., 12:24], clamped to {0, 1} for memory safety only.  hit_rows (optional, int32 [rows][3]): how
 *   many arg-maxes of the logits equal their target.  Logits are widened to float64; log-sum-exp and the row sum are float64 in a fixed
 *   order, one workgroup per row, no atomics: a row's result is a function of that row alone, bit-identical however the batch is
 *   split into calls.  ce_rows 8-byte aligned. */
int pf_chord_ce_rows(const float* root, const float* chroma, const float* bass, const float* gt, int rows, int n_step, double* ce_rows,
                     int32_t* hit_rows, void* stream);
/* pf_normal_rsample - Normal(mean, std).rsample() of torch.distributions, what Chord_8Bar.get_loss_dict draws from the encoder
 *   (models/model_chd_8bar.py:44): z[i] = mean[i] + std[i] * noise[i], n elements, the product rounded, then the sum.  noise: a tensor,
 *   or NULL - then element i uses what pf_randn(seed, stream_id, elem_offset) writes at i, bit-equal to pf_randn + the tensor form.
 *   As for pf_gaussian_sample, any n, elem_offset and alignment are accepted. */
int pf_normal_rsample(const float* mean, const float* std, const float* noise, uint64_t seed, uint64_t stream_id, uint64_t elem_offset,
                      float* z, size_t n, void* stream);

/* ---- weight broadcast over RCCL / xGMI.  The path has ONE exchange: rank 0 ships the packed weight
 * blob at start-up; the step loop has no collective.  librccl.so is opened on first use (dlopen), so a single-GPU process
 * never loads it.  `unique_id` is the 128-byte ncclUniqueId: rank 0 obtains it with pf_comm_unique_id and hands it to the
 * other ranks out of band (file / TCP store), exactly like an ncclUniqueId. */
typedef struct pf_comm pf_comm;
int pf_comm_unique_id(void* unique_id_out128);
int pf_comm_init(const void* unique_id128, int rank, int nranks, pf_comm** out);
int pf_comm_bcast(pf_comm* comm, void* dev_buf, size_t bytes, int root, void* stream);
int pf_comm_destroy(pf_comm* comm);

/* ---- output step: generated onset/sustain image -> note durations ----
 * Replaces the triple Python loop of utils.py:240-269 (prmat2c_to_prmat) and the note extraction of
 * utils.py:433-476 (prmat2c_to_midi_file): dur[n][t][key] = length in steps of the note that starts at (t, key), 0 where no
 * onset.  prmat2c is [n][2][steps][128] fp32 on the device (channel 0 onset, 1 sustain), dur is [n][steps][128] int32.
 * Rounding is the reference's int(round(v)) > 0 (== v > 0.5); custom_round != 0 selects utils.py:395-399 for the onset. */
int pf_prmat2c_durations(const float* prmat2c, int n, int steps, int custom_round, int32_t* dur, void* stream);

/* ---- scoring a roll against its chords ("Roll statistics"; not in the reference) ----
 * One pass over n onset/sustain images and, optionally, the chords they were conditioned on: integer counters per image, the number of
 * sounding cells per pitch class per beat, the number of onset cells per step.  Everything is a comparison or an integer count, so the
 * result is exact and does not depend on any order.  It is a fixed statistic, not a chord extractor: no voicing, no key, no inversion.
 *   Cells.  r(v) = v > 0.5 (custom_round: 0.95 < v < 1.05); on = r(onset), sus = r(sustain), sounding = on | sus; a NaN is silent.  With
 *   `mask`, only cells whose mask (channel 0) == 0 - the generated ones - count: any other cell is silent for every counter and table,
 *   but its raw values still serve as predecessor.  Predecessor occupied: v > 0.5 || v < -0.5 on either channel of the same key one step
 *   earlier (custom_round: r(v) on either channel) - check_prmat2c_integrity's rule; step 0 has no predecessor.  Pitch class = key % 12,
 *   beat j = step / 4.
 *   Chords.  Row j of `chord` is root one-hot [0:12] | chroma bits [12:24] | bass one-hot [24:36].  C = {k : chord[12 + k] > 0.5}; a beat
 *   with empty C enters no chord counter.  Bass class = arg-max of chord[24:36] (ties to the lowest index; no entry > 0: the beat has no
 *   bass); with bass_relative it becomes (bass + arg-max of chord[0:12]) % 12.  chord == NULL: every chord counter is 0.
 *   Every word of the three outputs is written by the call (unused counter slots as 0): the caller does not pre-zero.  One launch, one
 *   workgroup per image, no atomics, nothing allocated, nothing synchronised: capturable.  Refused before any launch: null prmat2c or
 *   outputs, pointers not 4-byte aligned, n <= 0, steps <= 0, steps % 4 != 0. */
enum {
  PF_ROLL_N_ONSET = 0,         /* onset cells */
  PF_ROLL_N_SOUNDING = 1,      /* sounding cells */
  PF_ROLL_N_ORPHAN = 2,        /* sus cells whose predecessor is not occupied */
  PF_ROLL_CHORD_BEATS = 3,     /* beats with non-empty C */
  PF_ROLL_SOUND_ON_CHORD = 4,  /* sounding cells on those beats */
  PF_ROLL_SOUND_IN_CHORD = 5,  /* of those, class in C */
  PF_ROLL_ONSET_IN_CHORD = 6,  /* onset cells on those beats, class in C */
  PF_ROLL_ONSET_ON_CHORD = 7,  /* onset cells on those beats */
  PF_ROLL_CHORD_CLASSES = 8,   /* sum over those beats of |C| */
  PF_ROLL_CHORD_HEARD = 9,     /* sum over those beats of how many classes of C sound at all in the beat */
  PF_ROLL_BASS_BEATS = 10,     /* chord beats that have a bass and at least one sounding cell */
  PF_ROLL_BASS_HIT = 11,       /* of those, the lowest sounding key of the beat has the bass class */
  PF_ROLL_LOW_KEY = 12,        /* lowest sounding key of the image, -1 if silent */
  PF_ROLL_HIGH_KEY = 13        /* highest sounding key of the image, -1 if silent */
};
#define PF_ROLL_NCOUNT 16
typedef struct pf_roll_stats_args {
  const float* prmat2c;               /* [n][2][steps][128]: channel 0 onset, 1 sustain (as pf_prmat2c_durations) */
  const float* chord;                 /* [n][steps/4][36]; NULL: the chord counters stay 0 */
  const float* mask;                  /* optional, shape of prmat2c, channel 0 read: only cells with mask == 0 count */
  int32_t n, steps;                   /* steps > 0, steps % 4 == 0 (a beat is 4 steps) */
  int32_t custom_round, bass_relative;
  int32_t* counters;                  /* [n][PF_ROLL_NCOUNT] */
  int32_t* chroma;                    /* [n][steps/4][12]: sounding cells per pitch class per beat */
  int32_t* onsets;                    /* [n][steps]: onset cells per step */
} pf_roll_stats_args;
int pf_roll_stats(const pf_roll_stats_args* a, void* stream);

/* ---- recognising the chords of a roll ("Chord recognition"; restates chord_extractor/ of the reference) ----
 * The labels chord_extractor.recognize returns for the file prmat2c_to_midi_file would write from a song of `segments` consecutive images,
 * computed on the images, with two deviations: a song always has segments * steps / 4 beats, and a song without notes is all "N".
 *   Notes.  Onset v > 0.5 (custom_round: 0.95 < v < 1.05) on channel 0, lasting while channel 1 is > 0.5 on the following steps of the key
 *   (as pf_prmat2c_durations), clipped at the end of its image; a NaN is silent.  A note-off closes every open note of its key, as the MIDI
 *   reader does.  A beat is 4 steps, a bar 4 beats: position 1 + beat % 4.
 *   Features.  chroma_q[j][pc]: the longest stretch of beat j covered by a single note of class pc = key % 12, in quarter beats (steps).
 *   bass_q[j][pc]: eighth beats (two per step) of beat j whose lowest sounding key has class pc.
 *   Scores.  For every window of j + 1 <= 5 beats ending at beat i that decode() reaches (it stops one beat past a downbeat) and every class
 *   c: num = window sum of chroma_q over the template minus over its complement, bass = window sum of bass_q at the class's bass, then in
 *   float64, in this order, (((num / 4) / size + 0.5 * (bass / 8)) - cls_const[c][0]) - cls_const[c][1]; a class of size 0 ("N") scores
 *   consts[14].  obs = ((score + consts[j]) + (position of beat i - j == 3 ? consts[12] : 0)) + (position odd ? consts[13] : 0).  The best
 *   class of a window is the arg-max of obs, ties to the lowest index; dp[i] = max over windows of dp[i - j - 1] + best obs, updated on
 *   strict "<" with j ascending; the labels are read back from dp[n - 1].  The division is IEEE round-to-nearest and no other operation
 *   rounds differently under contraction, so every score is the bit pattern numpy gives.
 *   Tables (caller-owned, on the device, built once from the vocabulary):  cls_bits[c] = template bits 0..11 | bass class << 12 | template
 *   size << 16;  cls_const[c] = {size * 0.1, 0.05 if the label is an inversion else 0.0} as the host computes them;  cls_rows[c] = the
 *   condition row [36] of the label;  consts[16] = {j * 0.7 for j = 0..11, 0.15, 0.2, 0.2 (the score of "N"), 0}.
 *   Comparison with `chord` (optional), per beat, recognised row r against condition row c: ROOT_HIT - arg-max of [0:12] equal (lowest
 *   index on ties) and both or neither have an entry > 0.5;  CHROMA_HIT - the bit sets {k : [12 + k] > 0.5} equal;  BASS_HIT - as root on
 *   [24:36], with bass_relative the condition's bass read as (bass + root) % 12;  FULL_HIT - all three;  CHROMA_INTER / CHROMA_UNION - sizes
 *   of the intersection / union of the bit sets.  chord == NULL: those six are 0.
 *   Every word of the seven outputs is written by the call: the caller does not pre-zero.  One launch, one workgroup per song, no global
 *   atomics, nothing allocated, nothing synchronised: capturable.  Refused before any launch: null or misaligned pointers (8 bytes for the
 *   float64 tables and path_score, 4 otherwise), songs, segments or steps <= 0, steps % 16 != 0, more than PF_CHORDREC_MAX_BEATS beats per
 *   song (16 images of 128 steps), n_classes outside 1..PF_CHORDREC_MAX_CLASSES, max_template outside 1..12 (the caller states the largest
 *   template size of its table; a larger entry in cls_bits is read modulo 16). */
enum {
  PF_CHORDREC_BEATS = 0,         /* beats of the song */
  PF_CHORDREC_ROOT_HIT = 1,
  PF_CHORDREC_CHROMA_HIT = 2,
  PF_CHORDREC_BASS_HIT = 3,
  PF_CHORDREC_FULL_HIT = 4,
  PF_CHORDREC_CHROMA_INTER = 5,
  PF_CHORDREC_CHROMA_UNION = 6,
  PF_CHORDREC_SEGMENTS = 7       /* recognised segments of the song */
};
#define PF_CHORDREC_NCOUNT 8
#define PF_CHORDREC_MAX_BEATS 512
#define PF_CHORDREC_MAX_CLASSES 576
typedef struct pf_chord_recognize_args {
  const float* prmat2c;               /* [songs * segments][2][steps][128]: channel 0 onset, 1 sustain */
  const float* chord;                 /* [songs][beats][36], beats = segments * steps / 4; NULL: no comparison */
  const int32_t* cls_bits;            /* [n_classes] */
  const double* cls_const;            /* [n_classes][2] */
  const float* cls_rows;              /* [n_classes][36] */
  const double* consts;               /* [16] */
  int32_t songs, segments, steps;     /* steps % 16 == 0 (a bar is 16 steps) */
  int32_t n_classes, max_template;
  int32_t custom_round, bass_relative;
  int32_t reserved;                   /* 0 */
  int32_t* labels;                    /* [songs][beats]: index into the vocabulary */
  int32_t* bounds;                    /* [songs][beats]: 1 on the first beat of every recognised segment, else 0 */
  float* rows;                        /* [songs][beats][36]: cls_rows[label] */
  int32_t* counters;                  /* [songs][PF_CHORDREC_NCOUNT] */
  double* path_score;                 /* [songs]: dp[n - 1] */
  int32_t* chroma_q;                  /* [songs][beats][12] */
  int32_t* bass_q;                    /* [songs][beats][12] */
} pf_chord_recognize_args;
int pf_chord_recognize(const pf_chord_recognize_args* a, void* stream);

/* ---- packed rolls and their nearest neighbours under transposition ("Roll matching"; not in the reference) ----
 * pf_roll_pack: n images [n][2][steps][128] (channel 0 onset, 1 sustain) -> bits[2][n * steps][4]: plane-major, the images' rows
 * consecutive, so a song of several images is one run of rows.  Key k of a row is bit k % 32 of word k / 32.  Plane 0 is on = r(onset),
 * plane 1 is sounding = on | r(sustain), r exactly the rule of pf_roll_stats: v > 0.5 (custom_round: 0.95 < v < 1.05); a NaN is silent.
 * One launch, ballots only, every output word written.  Refused: null or misaligned (4 bytes) pointers, n or steps <= 0.
 *
 * pf_roll_match: both sides are windows into one packed plane.  Side A, the queries: a_bits [rows_a][4] and a_starts[na], the row index
 * of each window's first row; side B, the corpus: b_bits and b_starts[nb].  Every window is `steps` consecutive rows; windows may overlap,
 * so a corpus with a window at every bar of every song is stored once.  The starts are trusted, as the other kernels trust their shapes:
 * every start .. start + steps - 1 must lie inside its plane.  The row offset start * 4 is formed in 64 bits.
 *   Shifts: k = 0 .. 2 * shifts, s_k = 0, -1, +1, -2, +2, ...  A candidate (b, k) means "the query is corpus window b transposed up by s_k
 *   semitones".  Its shifted query is qs[t][j] = q[t][j + s] for 0 <= j + s < 128, else 0: query notes that leave the keyboard are dropped.
 *   inter = |qs AND c|, union = |qs| + |c| - inter.  Two candidates compare as the fractions inter / union, exactly: a / b > c / d is
 *   a * d > c * b in int64; a candidate with union == 0 counts as 0 / 1.  Per corpus window the kept candidate is the best k, ties to the
 *   lowest k (s = 0 wins a tie).  Per query the topk best corpus windows are kept in descending order, ties to the lowest b.
 *   Outputs: top_index / top_shift (the semitones s, not k) / top_inter / top_union [na][topk]; slots beyond nb are -1, 0, 0, 0.  With
 *   the three table pointers non-NULL, tab_inter / tab_union / tab_shift [na][nb] hold each corpus window's kept candidate.  Every word
 *   of every output is written: the caller does not pre-zero.
 *   Three launches (|qs| per query and shift; the scan, a workgroup per PF_ROLL_MATCH_CHUNK corpus windows and 4 queries, which leaves its
 *   top-k per query in the workspace; a merge of those lists in chunk order), no atomics, nothing allocated, nothing synchronised:
 *   capturable.  Results do not depend on how queries or corpus are grouped.  Refused before any launch: null arguments, null a_bits /
 *   a_starts / b_bits / b_starts / top_* / workspace, a_bits / b_bits / workspace not 16-byte or any other pointer not 4-byte aligned,
 *   na, nb or steps <= 0, shifts outside 0..PF_ROLL_MATCH_MAX_SHIFTS, topk outside 1..PF_ROLL_MATCH_MAX_TOPK, reserved != 0, exactly one
 *   or two of the three table pointers, workspace_bytes < pf_roll_match_workspace_bytes(na, nb, topk) (which is 0 for arguments the call
 *   would refuse). */
#define PF_ROLL_MATCH_CHUNK 256       /* corpus windows one workgroup scans; partial top-k lists are per chunk */
#define PF_ROLL_MATCH_MAX_SHIFTS 15
#define PF_ROLL_MATCH_MAX_TOPK 8
typedef struct pf_roll_match_args {
  const uint32_t* a_bits;             /* one plane of the queries' rows, [rows_a][4] */
  const int32_t* a_starts;            /* [na] */
  const uint32_t* b_bits;             /* one plane of the corpus' rows, [rows_b][4] */
  const int32_t* b_starts;            /* [nb] */
  int32_t na, nb, steps;
  int32_t shifts, topk;
  int32_t reserved;                   /* 0 */
  int32_t* top_index;                 /* [na][topk] */
  int32_t* top_shift;                 /* [na][topk] */
  int32_t* top_inter;                 /* [na][topk] */
  int32_t* top_union;                 /* [na][topk] */
  int32_t* tab_inter;                 /* [na][nb] or NULL (all three or none) */
  int32_t* tab_union;
  int32_t* tab_shift;
  void* workspace;
  size_t workspace_bytes;
} pf_roll_match_args;
int pf_roll_pack(const float* prmat2c, int n, int steps, int custom_round, uint32_t* bits, void* stream);
size_t pf_roll_match_workspace_bytes(int na, int nb, int topk);
int pf_roll_match(const pf_roll_match_args* a, void* stream);

/* ---- condition encoders (replace RnnEncoder.forward dl_modules/chord_enc.py:15-22, TextureEncoder.forward
 *      dl_modules/txt_enc.py:23-35 and PianoTreeEncoder.forward dl_modules/pianotree_enc.py:97-121; only the Normal's mean is produced)
 *      PF_ENC_PNOTREE: input_dim = pitch classes + 5 duration digits (135), emb_size = note embedding (128), num_channel = hidden size
 *      of the per-step note GRU (256), hidden_dim = hidden size of the GRU over the 32 steps (512), z_dim 512 */
typedef struct pf_encoder pf_encoder;
enum { PF_ENC_CHORD = 0, PF_ENC_TEXTURE = 1, PF_ENC_PNOTREE = 2 };
int pf_encoder_create(int kind, int input_dim, int emb_size, int hidden_dim, int z_dim, int num_channel, pf_encoder** out);
void pf_encoder_destroy(pf_encoder* e);
size_t pf_encoder_weight_bytes(const pf_encoder* e);
int pf_encoder_pack_param(pf_encoder* e, const char* key, const float* src, const int64_t* shape, int ndim, void* host_blob);
int pf_encoder_pack_missing(const pf_encoder* e, char* buf, size_t buf_len);
int pf_encoder_bind_weights(pf_encoder* e, const void* dev_blob);
size_t pf_encoder_workspace_bytes(const pf_encoder* e, int batch);
/* chord:   x [B,T,input_dim] -> mu [B,z_dim];   texture: x [B,32,128] -> mu [B,z_dim];
 * pnotree: x [B,32,n_step,6] - the index grid (pitch index, 5 duration digits) of B two-bar segments with n_step = max_simu_note
 *          entries per time step, stored as floats - -> mu [B,z_dim] */
int pf_encoder_forward(pf_encoder* e, const float* x, int batch, int n_step, float* mu,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The whole Normal of the Polydis encoders (polydis/ptvae.py RnnEncoder.forward :21-28 and TextureEncoder.forward :106-118):
 * mu = linear_mu(h) as above and scale = exp(linear_var(h)), which DisentangleVAE's samplers need (polydis/model.py:188-239).
 * pf_encoder_create_dist is pf_encoder_create with one more flag: with_scale != 0 (PF_ENC_CHORD and PF_ENC_TEXTURE only) gives
 * linear_var.* a place in the blob and makes both keys required; pf_encoder_create is its with_scale = 0 case, whose blob size,
 * layout and mu are unchanged (linear_var.* accepted and ignored).  pf_encoder_forward_dist runs the pipeline of pf_encoder_forward
 * and writes mu [B,z_dim] and scale [B,z_dim]; on an encoder created without scale, or on PF_ENC_PNOTREE, it is an error. */
int pf_encoder_create_dist(int kind, int input_dim, int emb_size, int hidden_dim, int z_dim, int num_channel, int with_scale,
                           pf_encoder** out);
int pf_encoder_forward_dist(pf_encoder* e, const float* x, int batch, int n_step, float* mu, float* scale,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- frozen decoders, inference mode (greedy: every arg-max is fed back as the next token; ties go to the lowest index); plain fp32.
 *      PF_DEC_PNOTREE replaces PianoTreeDecoder.decoder(z, True, None, None, 0, 0) (dl_modules/pianotree_dec.py:155-332) at the default
 *      sizes of PianoTreeDecoder.__init__ (:11-99); max_simu_note (2..32) is an argument, and hidden_dim is dec_dur_hid_size, the width
 *      of the duration GRU: 0 or 16 (the default of PianoTreeDecoder) or 64 (polydis/ptvae.py PtvaeDecoder as DisentangleVAE.init_model
 *      builds it, polydis/model.py:314-316; the class is PianoTreeDecoder statement for statement); any other value is an error.  The
 *      other create arguments are ignored.
 *      PF_DEC_CHORD replaces ChordDecoder.forward(z_chd, True, 0.) (dl_modules/chord_dec.py:27-70) for
 *      ChordDecoder(input_dim = 36, z_input_dim, hidden_dim, z_dim, n_step) (:8-25).
 *      Parameter keys and shapes are the state_dict of those modules, in its order (pf_decoder_param_info). */
typedef struct pf_decoder pf_decoder;
enum { PF_DEC_CHORD = 0, PF_DEC_PNOTREE = 1 };
int pf_decoder_create(int kind, int max_simu_note, int input_dim, int z_input_dim, int hidden_dim, int z_dim, int n_step,
                      pf_decoder** out);
void pf_decoder_destroy(pf_decoder* d);
size_t pf_decoder_weight_bytes(const pf_decoder* d);
int pf_decoder_n_params(const pf_decoder* d);
int pf_decoder_param_info(const pf_decoder* d, int i, char* key_buf, size_t key_buf_len, int64_t shape[4], int* ndim);
/* nn.Module.load_state_dict of the two decoders: one tensor into the host blob (same messages as the other handles) */
int pf_decoder_pack_param(pf_decoder* d, const char* key, const float* src, const int64_t* shape, int ndim, void* host_blob);
int pf_decoder_pack_missing(const pf_decoder* d, char* buf, size_t buf_len);
/* The blob must be writable and 16-byte aligned: for PF_DEC_PNOTREE its tail is filled here, on the device, with what the decode loop
 * reads instead of note_embedding + the token columns of the GRU input weights (pianotree_dec.py:147-153 folded into :214-216 and
 * :320-327).  Synchronises the device; not part of a decode. */
int pf_decoder_bind_weights(pf_decoder* d, void* dev_blob);
size_t pf_decoder_workspace_bytes(const pf_decoder* d, int rows);
/* Kernel launches one pf_decoder_forward enqueues, counted by a dry run of the very walk that forward enqueues (no GPU needed); it
 * does not depend on rows. */
int pf_decoder_launches(const pf_decoder* d, int rows);
/* pnotree: z [rows,512] -> out0 = recon_pitch [rows,32,S-1,130], out1 = recon_dur [rows,32,S-1,5,2] (the two tensors
 *          PianoTreeDecoder.forward returns, pianotree_dec.py:334-339), out2 unused, est [rows,32,S-1,6] = their max(-1)[1]
 *          (pitch index, 5 duration digits: output_to_numpy, :375-378), S = max_simu_note.
 * chord:   z [rows,z_dim] -> out0 = recon_root [rows,n_step,12], out1 = recon_chroma [rows,n_step,12,2], out2 = recon_bass
 *          [rows,n_step,12] (chord_dec.py:66-70), est unused.
 * Everything is caller-owned device memory (workspace 16-byte aligned); launches only, on `stream`: capturable as a graph.  A row's
 * result does not depend on the other rows of the call. */
int pf_decoder_forward(pf_decoder* d, const float* z, int rows, float* out0, float* out1, float* out2, int32_t* est,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The chord walk with teacher forcing: ChordDecoder.forward(z_chd, False, tfr, gt_chd) (dl_modules/chord_dec.py:27-70), PF_DEC_CHORD
 * only.  The reference's per-step coin `random.random() < tfr` (:55) is the caller's: bit t of force_mask (t < n_step - 1) set means the
 * token fed to step t + 1 is gt[:, t] (:56-57), otherwise the arg-max token of step t is fed back (:59-64).  feedback says which
 * arg-max token:
 *   PF_FEEDBACK_ROW   - each row's own one-hot root | chroma bits | one-hot bass, as pf_decoder_forward feeds it: a row's result does
 *                       not depend on the other rows of the call, and force_mask 0 gives pf_decoder_forward's bits;
 *   PF_FEEDBACK_BATCH - what the reference computes at batch > 1: t_root[arange(bs), 0, idx] with idx of shape (bs, 1) (:59-63) sets
 *                       the root and bass part of EVERY row's token to the union over the call's rows (one more small launch per
 *                       fed-back step); the number Lightning logged as val/loss comes from this form at the logged batch size.
 * Refused before anything is enqueued: n_step - 1 > 64, a null gt, an unknown feedback, a short workspace.  Everything is
 * caller-owned device memory (workspace 16-byte aligned, pf_decoder_forced_workspace_bytes(d, rows) bytes); launches only: capturable.
 * pf_decoder_forced_launches counts, by a dry run of the same walk with every step fed back (force_mask 0), the most launches a call
 * enqueues: pf_decoder_launches under PF_FEEDBACK_ROW, at most n_step - 1 more under PF_FEEDBACK_BATCH; it does not depend on rows. */
enum { PF_FEEDBACK_ROW = 0, PF_FEEDBACK_BATCH = 1 };
typedef struct pf_chord_forced_args {
  const float* z;                     /* [rows][z_dim] */
  const float* gt;                    /* [rows][n_step][36], the batch's chord matrix */
  int32_t rows;
  int feedback;                       /* PF_FEEDBACK_* */
  uint64_t force_mask;
  float *root, *chroma, *bass;        /* [rows][n_step][12], [rows][n_step][12][2], [rows][n_step][12] */
  void* workspace; size_t workspace_bytes;
} pf_chord_forced_args;
size_t pf_decoder_forced_workspace_bytes(const pf_decoder* d, int rows);
int pf_decoder_forced_launches(const pf_decoder* d, int rows, int feedback);
int pf_decoder_forward_forced(pf_decoder* d, const pf_chord_forced_args* a, void* stream);

/* Arithmetic of the dense contractions (convs / linears):
 *   PF_PREC_F32    - v_mfma_f32_32x32x2_f32, exact fp32 FMA chains (157 TFLOP/s pipe);
 *   PF_PREC_BF16X3 - error-compensated split on the bf16 pipe: a.w ~= a_hi.w_hi + a_hi.w_lo + a_lo.w_hi with fp32
 *                    accumulation (~1e-5 relative per product, three v_mfma_f32_32x32x16_bf16 instead of eight fp32 MFMAs).
 * Both packings of every weight live in the blob; the mode can be switched between calls. */
enum { PF_PREC_F32 = 0, PF_PREC_BF16X3 = 1 };
int pf_unet_set_precision(pf_unet* u, int precision);
int pf_unet_get_precision(const pf_unet* u);
/* Element type of the split: the library is built twice from the same sources.  libpfhip.so splits into bf16 pieces (8 + 8 mantissa
 * bits, fp32's exponent range: "bf16x3", unit roundoff ~2^-18).  libpfhip_f16.so (-DPF_X3_F16) splits into fp16 pieces (11 + 11 bits,
 * three v_mfma_f32_32x32x16_f16 per product: "f16x3", ~2^-22 - the error of the fp32 mode - at ~0.97 of bf16x3's speed), with fp16's
 * range: activations must stay below 65504 in magnitude (weights below 255; they are stored times 2^8 and every epilogue undoes it).
 * In that library every entry point and constant named bf16x3 means f16x3; weight packings and plane buffers of the two libraries are
 * not interchangeable.  Returns 0 (bf16 pieces) or 1 (fp16 pieces). */
int pf_x3_element(void);

/* ---- per-op entry points (unit-testable kernels; same kernels the plan launches) ---------- */
/* Host helper: torch weight [N, K, kh, kw] (kh=kw=1 or 3) -> packed [kh*kw][K/4][Npad][4], Npad = roundup(N,64). */
size_t pf_packed_gemm_weight_floats(int n, int k, int taps);
int pf_pack_gemm_weight(const float* w, int n, int k, int taps, float* dst);
/* same bytes, bf16x3 packing [kh*kw][K/8][hi|lo][Npad][8] (bf16); needs k % 8 == 0 */
int pf_pack_gemm_weight_bf16x3(const float* w, int n, int k, int taps, void* dst);
/* [n][k][3][3] conv weight of an UpSample layer -> folded packing [4 parities x 4 taps][k/8][plane][Npad][8] (host; k % 8 == 0) */
int pf_pack_upfold_weight_bf16x3(const float* w, int n, int k, void* dst);
/* Winograd F(2x2, 3x3) packing of a 3x3 conv weight [n][k][3][3] (n % 64 == 0, k % 16 == 0) for pf_conv_args.w_wino: U = G g G^T per (n, k),
 * split into hi | lo pieces, laid out in matrix-operand order; pf_wino_weight_bytes(n, k) = 16 * k * n * 4 bytes */
size_t pf_wino_weight_bytes(int n, int k);
int pf_pack_wino_weight_bf16x3(const float* w, int n, int k, void* dst);

/* GroupNorm statistics on NHWC (optionally the channel-concat of two tensors) -> per-(b,c)
 * scale/shift so that y = x*scale + shift equals GroupNorm(x) (unet.py:321-336; eps 1e-5 / 1e-6). */
int pf_gn_scale_shift(const float* x0, int c0, const float* x1, int c1, int batch, int hw, int groups, float eps,
                      const float* gamma, const float* beta, float* scale, float* shift,
                      void* scratch, size_t scratch_bytes, void* stream);
/* LayerNorm statistics over the last dim: mean[m], rstd[m] (unet_attention.py:104-110, eps 1e-5). */
int pf_ln_stats(const float* x, int rows, int c, float eps, float* mean, float* rstd, void* stream);
/* The stem convolution (unet.py:78-80): 3x3, padding 1, x NCHW [batch][cin][h][w], w [cout][cin][3][3], out NHWC [batch][h][w][cout], fp32.
 * cout % 4 == 0 and cout * cin * 36 bytes <= 64 KB.  cin <= 2 with cout == 64 runs the register-weight kernel, which can also emit the
 * per-tile channel (sum, sumsq) of what it stores: stats [batch][pf_conv_in_stats_tiles][64][2] over 16x16-pixel tiles, tile ty * tilesx + tx,
 * in-image pixels only (the layout pf_gn_finalize_tiles reads).  stats on any other shape is refused (pf_conv_in_stats_tiles returns 0). */
int pf_conv_in(const float* x_nchw, const float* w, const float* bias, float* out_nhwc, int batch, int cin, int cout, int h, int w_,
               float* stats, void* stream);
int pf_conv_in_stats_tiles(int cin, int cout, int h, int w_);
/* The head (unet.py:145-149): out = conv3x3(silu(x * sc + sh)) + bias with per-sample GroupNorm rows sc / sh [batch][cin]; x NHWC
 * [batch][h][w][cin], w packed [9][cin][cout] (tap = ky * 3 + kx), out NCHW [batch][cout][h][w].  The zero padding is of the ACTIVATED tensor.
 * cout in 1..4, cin % 16 == 0, batch * h * w * cin < 2^31. */
int pf_conv_out(const float* x_nhwc, const float* sc, const float* sh, const float* w, const float* bias, float* out_nchw, int batch, int cin,
                int cout, int h, int w_, void* stream);
/* Time embedding with the SiLU of the ResBlocks' emb_layers folded in (unet.py:63-68,151-169):
 * out[b] = silu(W2 . silu(W0 . [cos(t_b f) | sin(t_b f)] + b0) + b2), f_j = exp(-ln(10000) j / (channels / 2)) in fp32; w0 [d_t][channels],
 * w2 [d_t][d_t], out [batch][d_t].  t int64 [batch], or NULL: row b is the embedding of time-step value b (the table of
 * pf_unet_prepare_time).  channels even, channels + d_t <= 8192. */
int pf_time_embed(const int64_t* t, const float* w0, const float* b0, const float* w2, const float* b2, float* out_silu, int batch,
                  int channels, int d_t, void* stream);
/* Batched mat-vec y[b][n] = W[n][:] . x[b][:] + bias[n] (bias may be NULL), W row-major [n][k], rows of x / y ldx / ldy floats apart,
 * k <= 2048.  n_per_group > 0: the block-diagonal form, output n reads x + (n / n_per_group) * x_group_stride.  exp_flag: y = expf(...)
 * (ungrouped only).  A row's sum is accumulated in the same order whatever its position in the batch. */
int pf_matvec(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int batch, int n, int k, int n_per_group,
              int x_group_stride, int exp_flag, void* stream);
/* One GRU cell update of the encoders, in place (torch gate order r | z | n): h = (1 - z) n + z h with r = sigmoid(gi_r + gh_r),
 * z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n); gi = W_ih x + b_ih, gh = W_hh h + b_hh [rows][3 hidden], h rows ld_h floats apart.
 * lens == NULL: row b reads gi + b * ld_gi (ld_gi >= 3 hidden; seq_len, step, reverse unused).  lens != NULL: the update over packed
 * variable-length sequences, gi [rows][seq_len][3 hidden] (ld_gi unused): row b takes part while step < lens[b] and reads element step
 * (forward) or lens[b] - 1 - step (reverse); any other row keeps its bits.  Null pointers, non-positive sizes, ld_h < hidden, a negative
 * step and rows * hidden >= 2^31 are refused. */
int pf_gru_gates(const float* gi, int ld_gi, const float* gh, float* h, int ld_h, int rows, int hidden, const int* lens, int seq_len,
                 int step, int reverse, void* stream);
/* One fused GRU step of the decoders for R rows: gi = Wx . x + add1 + add2, gh = Wh . h_in + b_hh, h_out = (1 - z) n + z h_in (gates as
 * above).  x [R][ldx] (Kx columns read; ldx 0: one row for every row of the batch; Kx 0: no x part), Wx [3H][ldwx] (a column slice of
 * a wider matrix: ldwx >= Kx), Wh [3H][H], h_in / h_out [R][H], add1 / add2 [R][ld1 / ld2] or NULL (a stride of 0 broadcasts one row).
 * Refused before anything is enqueued: H % 4 != 0, wh or h_in not 16-byte aligned, 8 (H + Kx) floats above 64 KiB, h_out == h_in. */
typedef struct pf_gru_step_args {
  const float* x; int ldx, Kx; const float* wx; int ldwx;
  const float* h_in; const float* wh; const float* b_hh;
  const float* add1; int ld1; const float* add2; int ld2;
  float* h_out; int R, H;
} pf_gru_step_args;
int pf_gru_step(const pf_gru_step_args* a, void* stream);
/* LayerNorm applied and split into bf16 hi/lo planes [rows][c] | [rows][c] (the A operand of pf_conv2d with a_planes=1);
 * replaces pf_ln_stats + the LayerNorm GEMM prologue for the transformer block's q/k/v and GeGLU projections */
int pf_ln_planes(const float* x, int rows, int c, float eps, const float* gamma, const float* beta, void* planes, void* stream);
/* The feed-forward half of BasicTransformerBlock as ONE launch (unet_attention.py:119-124 `x = ff(norm3(x)) + x`, :296-333 FeedForward /
 * GeGLU) for d_model 256, hidden 1024, bf16x3 arithmetic:  out = x + W2 . (a * gelu(g)) + b2 with [a|g] = W1 . LayerNorm(x) + b1.
 * x fp32 [batch*l][256], l % 64 == 0.  w1_bf16x3: the bf16x3 packing (pf_pack_gemm_weight_bf16x3) of ff.net.0.proj with its 2048 rows
 * reordered value/gate-interleaved in blocks of 32 (row 64 i + j <- value 32 i + j, row 64 i + 32 + j <- gate 32 i + j), b1 in the same
 * order; w2_bf16x3: packing of ff.net.2 ([256][1024]).  The result goes to fp32 `out` or, when out_planes != NULL, to bf16 hi/lo planes
 * [M][256] | [M][256].  Bit-identical to pf_ln_planes + pf_conv2d(geglu, out_planes) + pf_conv2d(a_planes, res = x). */
int pf_mlp_geglu_fused(const float* x, int batch, int l, const float* ln_gamma, const float* ln_beta, float ln_eps,
                       const void* w1_bf16x3, const float* b1, const void* w2_bf16x3, const float* b2,
                       float* out, void* out_planes, void* stream);
/* The same launch with the SpatialTransformer's closing 1x1 convolution chained on (unet_attention.py:77-79 `proj_out(x) + x_in` after the
 * last transformer layer): out = res3 + b3 + W3 . (x + ff(norm3(x))), the ff result never leaving the chip.  w3_bf16x3: bf16x3 packing
 * of proj_out ([256][256]); res3: the block input [batch*l][256]; stats3 (optional): per-64-row-tile channel (sum, sumsq) of `out`,
 * [batch][l/64][256][2], for the GroupNorm that consumes it.  Bit-identical to pf_mlp_geglu_fused(out_planes) + pf_conv2d(a_planes, res). */
int pf_mlp_geglu_proj_fused(const float* x, int batch, int l, const float* ln_gamma, const float* ln_beta, float ln_eps,
                            const void* w1_bf16x3, const float* b1, const void* w2_bf16x3, const float* b2,
                            const void* w3_bf16x3, const float* b3, const float* res3, float* out, float* stats3, void* stream);
/* Implicit-GEMM convolution / linear on NHWC with fused prologue and epilogue (fp32 MFMA).
 *   ks 1|3, stride 1|2, ups 0|1 (nearest x2 folded into the input read, unet.py:236-238)
 *   prologue: 0 none | 1 y=silu(x*sc+sh) | 2 y=x*sc+sh (sc,sh [B][Cin]) | 3 LayerNorm (mean,rstd per row; sc,sh = gamma,beta [Cin])
 *   epilogue: + bias[n] + sbias[b][n] + res[m][n]; geglu!=0: out[m][j] = v*gelu_erf(g) on interleaved halves */
typedef struct pf_conv_args {
  const float* x0; int32_t c0; const float* x1; int32_t c1; /* input = concat(x0, x1) along channels */
  int32_t batch, hin, win;                                   /* input spatial size per sample (dense: hin=1, win=rows per sample) */
  int32_t ks, stride, ups;
  const float* w; int32_t n;                                 /* packed weights, logical N */
  int32_t prologue; const float* sc; const float* sh; const float* mean; const float* rstd;
  const float* bias; const float* sbias; int32_t ld_sbias; const float* res; int32_t ld_res;
  int32_t geglu;
  float* out; int32_t ld_out;
  int32_t precision;                                         /* PF_PREC_F32 (w = fp32 packing) | PF_PREC_BF16X3 (w = bf16x3 packing) */
  float* stats_out;                                          /* optional [B][tiles][N][2] per-tile (sum, sumsq) of the outputs; see pf_conv_stats_tiles */
  void* splitk_ws; size_t splitk_ws_bytes;                   /* optional scratch for split-K (small-M layers); see pf_conv_splitk_ws_bytes */
  int32_t a_planes;                                          /* x0 is NOT fp32 but bf16 hi/lo planes [M][K] | [M][K] from a producer's out_planes (ks=1, prologue 0, bf16x3) */
  void* out_planes;                                          /* optional: write the result as bf16 hi/lo planes [M][ld_out] | [M][ld_out] instead of fp32 `out` */
  void* qkv_planes;                                          /* optional (ks=1, N = 3C, d_head 64): instead of `out`, write the fused q|k|v projection
                                                                as bf16 hi/lo planes [qh|ql|kh|kl|vTh|vTl] (each B*L*C) for pf_attention_bf16x3 */
  /* optional fused 1x1 projection of a second tensor, accumulated into the same output tile (the ResBlock's
   * skip_connection conv folded into its second 3x3 conv, unet.py:262-277): out += skip_w . concat(skip_x0, skip_x1) + skip_bias.
   * bf16x3, ks = 3, stride 1, no upsampling; skip_w is the bf16x3 packing of the [n][skip_c0+skip_c1] weight, channel
   * counts multiples of 32. */
  /* ups = 1 only: `w` is the PARITY-FOLDED bf16x3 packing (pf_pack_upfold_weight_bf16x3) - nearest x2 upsampling followed by a
   * 3x3 conv equals, per output parity (y&1, x&1), a 2x2 conv on the source grid with row/column-summed weights: 4/9 of the MACs */
  int32_t ups_fold;
  const float* skip_x0; int32_t skip_c0;
  const float* skip_x1; int32_t skip_c1;
  const void* skip_w;
  const float* skip_bias;
  /* optional (bf16x3, prologue 1 or 2): GroupNorm scale/shift computed INSIDE the launch from the producers' per-tile statistics
   * (what pf_gn_finalize_tiles computes in its own launch): every workgroup reduces its sample's statistics at start-up and writes
   * the sample's rows of `sc` / `sh` (identical values from every workgroup of the sample) before it reads them.  gn_stats0 != NULL
   * enables it; tensors with many tiles per sample (the 128x128 / 64x64 levels) are better served by the separate launch. */
  const float* gn_stats0; int32_t gn_tiles0;
  const float* gn_stats1; int32_t gn_tiles1;
  const float* gn_gamma; const float* gn_beta;
  float gn_eps; int32_t gn_groups;
  /* optional: row of `sbias` per sample - sbias[sbias_rows[b]] instead of sbias[b] (the hoisted time-bias table indexed by the
   * device-resident t[b]); rows outside [0, sbias_nrows) are clamped */
  const int64_t* sbias_rows; int32_t sbias_nrows;
  int32_t no_t16;          /* != 0: never pick the 16x16-pixel tile (PF_OPT_CONV_T16 = off) */
  int32_t no_pp;           /* != 0: never run the two-group ping-pong form of the 128-wide tile (PF_OPT_CONV_PP = off) */
  /* measurement aids (tools/sweep_conv.py): 0 = the library's own choice.  force_tile: 1 + tile index (1: 128 px x 128 ch, 2: 128 px x 64 ch,
   * 3: 64 px x 64 ch; bf16x3 3x3 stride 1 and planes GEMMs without GeGLU, tile 1 needs n % 128 == 0); force_ksplit: K slices across workgroups (bf16x3 3x3 stride 1,
   * must divide the 32-channel chunks; > 1 needs splitk_ws).  Results are the same up to summation order. */
  int32_t force_tile, force_ksplit;
  /* > 0: the SECOND sources (x1, skip_x1, gn_stats1) hold only x1_bmod samples; sample b reads sample b % x1_bmod of them (the shared skip
   * tensors of pf_unet_forward_cfg) */
  int32_t x1_bmod;
  /* Fused Winograd F(2x2, 3x3) form of the ResBlock conv (bf16x3, ks = 3, stride 1, prologue 1, hin / win multiples of 16, n a multiple
   * of 64, no fused skip projection): w_wino = the layer's weights transformed and packed by pf_pack_wino_weight_bf16x3; wino != 0 asks for it.
   * 2.25x fewer matrix-pipe operations; equal to the direct form up to rounding (the transforms amplify the split's operand rounding
   * ~1.5x, tools/micro/winograd_numerics.py).  A launch that does not qualify runs the direct form on `w`. */
  const void* w_wino; int32_t wino;
  /* optional range telemetry: a device word (fp32 bit pattern, start at 0) that receives max(word, largest |value| this launch stores)
   * by atomic max - see pf_unet_track_absmax */
  void* absmax_slot;
  /* ks = 3, stride = 2 only.  0: one zero row / column on every side (Conv2d(3, 2, padding = 1)).  PF_PAD_BOTTOM_RIGHT: none above / left,
   * one below / right - F.pad(x, (0, 1, 0, 1)) followed by Conv2d(3, 2, padding = 0), the DownSample of the first-stage autoencoder
   * (autoencoder.py:406-426); output pixel (y, x) then reads input rows 2y .. 2y+2 instead of 2y-1 .. 2y+1.  hin and win must be even. */
  int32_t pad_mode;
} pf_conv_args;
enum { PF_PAD_SAME = 0, PF_PAD_BOTTOM_RIGHT = 1 };
/* scratch bytes a launch with these arguments would like for split-K (0 = the launch does not split) */
size_t pf_conv_splitk_ws_bytes(const pf_conv_args* a);
/* number of per-sample tiles a pf_conv2d launch with these arguments emits into stats_out (0 on error) */
int pf_conv_stats_tiles(const pf_conv_args* a);
/* What a pf_conv2d launch with these arguments runs (needs no device): the arguments are checked as pf_conv2d checks them (same code and
 * pf_last_error() text on refusal, *out zero-filled), then *out says which kernel form they get, the pixels x channels one workgroup owns,
 * the K split across workgroups they would like and the one they get with the splitk_ws they carry, and the two older queries' answers.
 * Forms: fp32 MFMA direct | split precision direct (1x1, 3x3, strided, upsampling through the halo read) | the same on the 64 px x 64 ch tile with
 * two wave groups of one workgroup halving K | on the 128 px x 128 ch tile with two wave groups half a tap apart | parity-folded upsampling (four
 * 2x2 convs on the source grid) | planes GEMM (a_planes) | fused Winograd F(2x2, 3x3). */
enum { PF_CONV_FORM_F32 = 0, PF_CONV_FORM_SPLIT, PF_CONV_FORM_SPLIT_KG2, PF_CONV_FORM_SPLIT_PINGPONG, PF_CONV_FORM_UPFOLD, PF_CONV_FORM_PLANES, PF_CONV_FORM_WINO };
typedef struct pf_conv_plan_info {
  int32_t form, tile_h, tile_w, tile_n;   /* PF_CONV_FORM_*; output pixels (rows x columns) x channels per workgroup */
  int32_t wave_groups;                    /* 1, or 2 four-wave groups per workgroup */
  int32_t ksplit_wanted, ksplit;          /* K slices across workgroups: wanted / granted (1 = none) */
  int32_t stats_tiles; size_t splitk_ws_bytes;   /* = pf_conv_stats_tiles, pf_conv_splitk_ws_bytes */
  double flops;                           /* operations the launch executes */
} pf_conv_plan_info;
int pf_conv_describe(const pf_conv_args* a, pf_conv_plan_info* out);
/* GroupNorm scale/shift from per-tile statistics of up to two channel-concatenated producers (no pass over the tensors) */
int pf_gn_finalize_tiles(const float* stats0, int tiles0, int c0, const float* stats1, int tiles1, int c1, int batch, int hw,
                         int groups, float eps, const float* gamma, const float* beta, float* scale, float* shift, void* stream);
int pf_conv2d(const pf_conv_args* a, void* stream);

/* softmax(q k^T * d_head^-0.5) v per (batch, head); q [B,Lq,*], k/v [B,Lk,*] with row strides ld*, heads packed
 * along the last dim (unet_attention.py:261-293). d_head in {32,64}. */
/* self-attention on the pre-split planes written by pf_conv2d(qkv_planes=...): d_head 64, L % 128 == 0 (bf16x3 split MFMA);
 * the result goes to fp32 `o` or, when o_planes != NULL, to bf16 hi/lo planes [M][C] | [M][C] for a following planes GEMM */
int pf_attention_bf16x3(const void* qkv_planes, float* o, int ldo, void* o_planes, int batch, int n_heads, int l, int form /* PF_OPT_AUTO | 0: 128-query | 1: 256-query workgroups */,
                        void* stream);
/* The same attention for SMALL batches (128-query form): when (l / 128) * n_heads * batch workgroups would leave three quarters of the CUs idle and
 * l % 512 == 0 (batch 1 / 2 at L = 1024), the keys of every query tile are split over four workgroups - each leaves its un-normalised partial result,
 * running maximum and row sum in `scratch` - and a second launch merges them (the online-softmax combination; equal to the one-launch form up to
 * summation order).  scratch_bytes >= pf_attention_split_scratch_bytes(batch, n_heads, l) (0 = this shape does not split: one launch, scratch unused). */
size_t pf_attention_split_scratch_bytes(int batch, int n_heads, int l);
int pf_attention_bf16x3_split(const void* qkv_planes, float* o, int ldo, void* o_planes, int batch, int n_heads, int l, void* scratch, size_t scratch_bytes,
                              void* stream);
int pf_attention(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                 int batch, int n_heads, int d_head, int lq, int lk, void* stream);

/* ---- vanilla DDPM noise predictor (replaces UNet.__init__ / forward, ddpm/unet.py:291-421, with TimeEmbedding :61-82,
 *      ResidualBlock :85-141, AttentionBlock :147-215, Upsample / Downsample :254-288; the `ddpm` model of params/ddpm.yaml) -------
 * Same life cycle as pf_unet: create, pack every key of the state_dict (keys relative to ddpm.eps_model.; the never-applied
 * AttentionBlock `norm` keys are accepted and dropped), bind the device copy of the blob, forward.  The reference's quirks are kept:
 * compounding channel multipliers, no activation in front of the ResBlock time projection, one attention head with d_k = channels,
 * ConvTranspose2d(4, 2, 1) upsampling, GroupNorm(8) before the final conv.  Precision: PF_PREC_F32 (exact fp32) or PF_PREC_BF16X3
 * (the split; f16x3 in libpfhip_f16.so) for the convs and linears; the attention core is exact fp32 in every mode. */
typedef struct pf_ddpm pf_ddpm;
typedef struct pf_ddpm_cfg {
  int32_t image_channels, n_channels, n_levels;
  int32_t ch_mults[8];   /* out = in * ch_mults[i] (unet.py:360) */
  int32_t is_attn[8];
  int32_t n_blocks;      /* UpDownBlocks per level (unet.py:322, 2) */
  int32_t img_h, img_w;
} pf_ddpm_cfg;
int pf_ddpm_create(const pf_ddpm_cfg* cfg, pf_ddpm** out);
void pf_ddpm_destroy(pf_ddpm* u);
size_t pf_ddpm_weight_bytes(const pf_ddpm* u);
int pf_ddpm_n_params(const pf_ddpm* u);
int pf_ddpm_param_info(const pf_ddpm* u, int i, char* key_buf, size_t key_buf_len, int64_t shape[4], int* ndim);
int pf_ddpm_pack_param(pf_ddpm* u, const char* key, const float* src, const int64_t* shape, int ndim, void* host_blob);
int pf_ddpm_pack_missing(const pf_ddpm* u, char* buf, size_t buf_len);
int pf_ddpm_bind_weights(pf_ddpm* u, const void* dev_blob);
int pf_ddpm_set_precision(pf_ddpm* u, int precision);
int pf_ddpm_get_precision(const pf_ddpm* u);
size_t pf_ddpm_workspace_bytes(const pf_ddpm* u, int batch);
int pf_ddpm_n_launches(const pf_ddpm* u, int batch);
/* algorithmic operations of one forward (convs, linears, attention, in the current precision's plan) */
double pf_ddpm_flops(const pf_ddpm* u, int batch);
/* eps = UNet(x, t): x [B,image_channels,H,W] f32, t [B] i64 on the device, eps like x (unet.py:398-421; p_sample's eps_model call,
 * ddpm/__init__.py p_sample) */
int pf_ddpm_forward(pf_ddpm* u, const float* x, const int64_t* t, int batch, float* eps, void* workspace, size_t workspace_bytes, void* stream);

/* Single-head self-attention with a wide head (AttentionBlock core, unet.py:197-205): o = softmax(q k^T d^-0.5) v per sample, exact fp32,
 * q / k / v rows of stride ld (the fused projection's q | k | v columns), o rows of stride ldo; d % 16 == 0, d <= 1024, l % 64 == 0,
 * l <= 1024.  scratch: pf_attention_wide_scratch_bytes(batch, l) (the probabilities).  Bit-identical from run to run. */
size_t pf_attention_wide_scratch_bytes(int batch, int l);
int pf_attention_wide(const float* q, const float* k, const float* v, int ld, float* o, int ldo, int batch, int l, int d, void* scratch,
                      size_t scratch_bytes, void* stream);
/* ConvTranspose2d(Cin, Cout, 4, stride 2, pad 1) (Upsample, unet.py:254-262) as four parity-folded 2x2 convs on the source grid.
 * torch weight [Cin][Cout][4][4] ->
 *   pf_pack_convt_weight_bf16x3: the 16-tap folded split packing of pf_pack_upfold_weight_bf16x3 (pf_packed_gemm_weight_floats(Cout, Cin, 16)
 *                                floats), run by pf_conv2d with ups = 1, ups_fold = 1, bf16x3 and the ConvT bias as `bias`;
 *   pf_pack_convt_weight_f32:    fp32 [parity][tap][Cin][Cout] (pf_convt_weight_floats), run by pf_conv_transpose_f32 on NHWC x [B][h][w][Cin]
 *                                -> out [B][2h][2w][Cout]. */
size_t pf_convt_weight_floats(int cin, int cout);
int pf_pack_convt_weight_bf16x3(const float* w, int cin, int cout, void* dst);
int pf_pack_convt_weight_f32(const float* w, int cin, int cout, float* dst);
int pf_conv_transpose_f32(const float* x, int batch, int h, int w, int cin, const float* w_packed, int cout, const float* bias, float* out,
                          void* stream);

/* ---- first-stage autoencoder (replaces Autoencoder.encode / decode / forward with Encoder, Decoder, ResnetBlock, AttnBlock, UpSample,
 *      DownSample and GaussianDistribution, stable_diffusion/model/autoencoder.py:27-490; the `autoencoder` model of params/autoencoder.yaml;
 *      LatentDiffusion.autoencoder_encode / autoencoder_decode, latent_diffusion.py:112-136) -------
 * Same life cycle as pf_ddpm: create, pack every key of the state_dict (encoder.*, decoder.*, quant_conv.*, post_quant_conv.*; the
 * training-only loss.* keys are accepted and dropped), bind the device copy of the blob, then encode / decode.  The image size is an
 * argument of the calls, not of the handle: H and W must be multiples of 2^(n_levels-1) (even at every DownSample), and the tokens of the
 * attention, (H / 2^(n_levels-1)) * (W / 2^(n_levels-1)), a multiple of 64 and at most 1024 (pf_attention_wide).  GroupNorm is
 * GroupNorm(32, eps 1e-6); attention is one head of width C with scale C^-0.5, exact fp32 in every mode.  channels * multiplier must be
 * a multiple of 32 at every level, in / out channels and z / emb channels 1..4. */
typedef struct pf_autoenc pf_autoenc;
typedef struct pf_autoenc_cfg {
  int32_t in_channels, out_channels, channels, n_levels;
  int32_t channel_multipliers[8];
  int32_t n_resnet_blocks, z_channels, emb_channels;
} pf_autoenc_cfg;
int pf_autoenc_create(const pf_autoenc_cfg* cfg, pf_autoenc** out);
void pf_autoenc_destroy(pf_autoenc* u);
size_t pf_autoenc_weight_bytes(const pf_autoenc* u);
int pf_autoenc_n_params(const pf_autoenc* u);
int pf_autoenc_param_info(const pf_autoenc* u, int i, char* key_buf, size_t key_buf_len, int64_t shape[4], int* ndim);
int pf_autoenc_pack_param(pf_autoenc* u, const char* key, const float* src, const int64_t* shape, int ndim, void* host_blob);
int pf_autoenc_pack_missing(const pf_autoenc* u, char* buf, size_t buf_len);
int pf_autoenc_bind_weights(pf_autoenc* u, const void* dev_blob);
int pf_autoenc_set_precision(pf_autoenc* u, int precision);
int pf_autoenc_get_precision(const pf_autoenc* u);
/* workspace, kernel launches and algorithmic operations of one encode of [batch, in_channels, h, w] / one decode of a latent
 * [batch, emb_channels, zh, zw], from a dry run of the walk that the call enqueues (no GPU needed; 0 for a shape the model cannot run) */
size_t pf_autoenc_encode_workspace_bytes(const pf_autoenc* u, int batch, int h, int w);
size_t pf_autoenc_decode_workspace_bytes(const pf_autoenc* u, int batch, int zh, int zw);
int pf_autoenc_encode_launches(const pf_autoenc* u, int batch, int h, int w);
int pf_autoenc_decode_launches(const pf_autoenc* u, int batch, int zh, int zw);
double pf_autoenc_encode_flops(const pf_autoenc* u, int batch, int h, int w);
double pf_autoenc_decode_flops(const pf_autoenc* u, int batch, int zh, int zw);
/* Autoencoder.encode + GaussianDistribution (+ .sample()): img NCHW [B, in_channels, h, w] -> mean, log_var (clamped to [-30, 20]) and
 * z = scale * (mean + exp(0.5 log_var) * noise), each NCHW [B, emb_channels, h / 2^(L-1), w / 2^(L-1)]; any of the three outputs may be
 * NULL.  noise: a tensor shaped like z, or NULL - then element i of z uses what pf_randn(seed, stream_id, elem_offset) writes at i.
 * `scale` is the latent scaling factor (1 for the plain posterior sample). */
int pf_autoenc_encode(pf_autoenc* u, const float* img, int batch, int h, int w, float scale, const float* noise, uint64_t seed,
                      uint64_t stream_id, uint64_t elem_offset, float* z, float* mean, float* log_var, void* workspace,
                      size_t workspace_bytes, void* stream);
/* Autoencoder.decode: img = decoder(post_quant_conv(z / scale)); z NCHW [B, emb_channels, zh, zw] -> img NCHW [B, out_channels, zh 2^(L-1), zw 2^(L-1)] */
int pf_autoenc_decode(pf_autoenc* u, const float* z, int batch, int zh, int zw, float scale, float* img, void* workspace,
                      size_t workspace_bytes, void* stream);
/* GaussianDistribution.sample on moments already computed: z[i] = scale * (mean[i] + exp(0.5 log_var[i]) * noise[i]), n elements; noise as
 * for pf_autoenc_encode.  The same arithmetic as the encode launch: bit-identical to the z it writes from the same moments and noise. */
int pf_gaussian_sample(const float* mean, const float* log_var, const float* noise, uint64_t seed, uint64_t stream_id,
                       uint64_t elem_offset, float scale, float* z, size_t n, void* stream);

/* Multi-GPU: one process per GPU.  The path shards over the batch with no exchange in the step loop; the single collective
 * (weight broadcast at start-up) goes either through the host's torch.distributed (backend "nccl" = RCCL over xGMI) on the packed
 * blob or through the library's own pf_comm_* entry points above (librccl opened with dlopen). */

#ifdef __cplusplus
}
#endif
#endif /* PFHIP_H */
