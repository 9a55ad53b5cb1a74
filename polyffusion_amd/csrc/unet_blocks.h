// unet_blocks.h - the block emitters both UNet plans (pf_unet, pf_ddpm) are built from: conv / linear emission, GroupNorm, ResBlock,
// downsample, the parity-folded split upsample, stem and head convs, and the table rows of a ResBlock and of the time-bias matrix.
// The first-stage autoencoder (pf_autoenc) walks the same emitters with GroupNorm eps 1e-6, no time bias and its DownSample's padding.
// What the models differ in (SpatialTransformer vs wide attention, nearest-upsample + conv vs ConvTranspose, the time embeddings) stays
// in unet.hip / ddpm_unet.hip.
#pragma once
#include "plan.h"

namespace pf {

// What a model's plan switches on beyond the plain launches.  The default value is pf_ddpm's: nothing.
struct PlanOpts {
  int precision = PF_PREC_F32;
  bool tile_stats = false;      // producers emit per-tile channel statistics and GroupNorm reads those instead of the data
  void* amax_slot = nullptr;    // pf_unet_track_absmax: caller-owned device word, nullptr = off
  int opt[PF_OPT_COUNT];        // pf_unet_set_option
  PlanOpts() { for (int& v : opt) v = PF_OPT_AUTO; }
};

// All ResBlock time projections gathered into one [sum][d_t] matrix (+ bias): one mat-vec launch per forward
struct TimeBias {
  int d_t = 0, sum = 0;
  size_t w = 0, b = 0;
  int take(int co) { const int o = sum; sum += co; return o; }   // a block's column offset
  void alloc(WeightTable& wt) { w = wt.alloc((size_t)sum * d_t); b = wt.alloc((size_t)sum); }
  void rows(WeightTable& wt, const std::string& prefix, int co, int off) const {
    wt.raw_at(prefix + ".weight", {co, d_t}, w + (size_t)off * d_t);
    wt.raw_at(prefix + ".bias", {co}, b + (size_t)off);
  }
};

// ResBlock: offsets (floats) into the packed blob
struct ResW {
  size_t gn1_g, gn1_b, w1, b1, gn2_g, gn2_b, w2, b2, wskip, bskip;
  size_t wino1 = 0, wino2 = 0;   // Winograd packings of the two 3x3 convs (0: none)
  int emb_off;                   // column offset into the time-bias matrix
};
struct ResNames { const char *norm1, *conv1, *emb, *norm2, *conv2, *skip; };   // sub-module names under the block's prefix
// the block's rows of the weight table, except its time projection (TimeBias::rows).  `wino`: Winograd packings beside the 3x3 convs
void res_rows(WeightTable& wt, const std::string& p, const ResNames& nm, int ci, int co, bool wino, ResW& r);

// A tensor in the workspace: NHWC data + (optionally) the per-tile channel statistics its producer emitted.
struct Tn {
  const float* d = nullptr; int c = 0;
  const float* st = nullptr; int nt = 0;   // [B][nt][c][2] (sum, sumsq); nt == 0: none
  int bmod = 0;                            // > 0: the tensor (and its statistics) holds only bmod samples, shared by samples b and b + bmod (pf_unet_forward_cfg)
};

struct BlockCtx : PlanCtx {
  PlanOpts o;
  // every ResBlock's additive time bias [rows][tb_ld]; with a hoisted table (pf_unet_prepared) tb_rows[b] = t[b] picks the row of sample b
  const float* tb = nullptr; int tb_ld = 0; const int64_t* tb_rows = nullptr; int tb_nrows = 0;

  int x1mod(const Tn& x1) const { return (x1.c > 0 && x1.bmod > 0 && x1.bmod != B) ? x1.bmod : 0; }

  // launch a conv (ks 3) / linear (ks 1); `out`: the output as a tensor, with the per-tile channel statistics the producer emits for a
  // later GroupNorm when the plan uses them (buffer from the persistent or the temp region, matching the lifetime of the output);
  // `w_own`: a split packing of its own instead of the one behind a.w
  void conv(pf_conv_args a, Tn* out = nullptr, bool persist = true, const float* w_own = nullptr);
  // GroupNorm scale/shift of concat(x0, x1): from the producers' tile statistics when the inputs carry them, otherwise by a pass over
  // the data.  `fuse_ok`: the consumer is a split conv that can do the reduction over the tiles in its own prologue (gn_attach)
  struct GnRef { bool fused = false; const float* s0 = nullptr; const float* s1 = nullptr; int t0 = 0, t1 = 0; size_t g = 0, b = 0; float eps = 0.f; int groups = 0; };
  GnRef gn(const Tn& x0, const Tn& x1, int hw, int groups, float eps, size_t g, size_t b_, float* sc, float* sh, bool fuse_ok = false);
  void gn_attach(pf_conv_args& a, const GnRef& r);
  void wino_attach(pf_conv_args& a, size_t wino_off);
  // statistics for a tensor whose producer emitted none
  void stats_pass(Tn& x, int hw, bool persist);

  // conv2(SiLU(GN(conv1(SiLU(GN(x))) + time bias))) + shortcut(x), x = concat(x0, x1); `time_bias` false: a block without a time
  // projection (L.emb_off unused)
  Tn res_block(const ResW& L, const Tn& x0, const Tn& x1, int H, int W_, int co, float eps = 1e-5f, bool time_bias = true);
  Tn downsample(const Tn& x, int H, int W_, size_t wgt, size_t bias, int co, int pad_mode = PF_PAD_SAME);   // 3x3, stride 2
  Tn upsample_fold(const Tn& x, int H, int W_, size_t w_fold, size_t bias, int co);           // split modes: four 2x2 convs on the source grid
  Tn stem(const float* x_nchw, size_t wgt, size_t bias, int cin, int co, int H, int W_);
  void head(const Tn& x, int H, int W_, int groups, size_t g, size_t b_, size_t wgt, size_t bias, int co, float* out_nchw,
            float eps = 1e-5f);   // GN + SiLU + conv3x3 -> NCHW
};

}  // namespace pf
