// unet_blocks.hip - the block emitters shared by the pf_unet and pf_ddpm plans (unet_blocks.h).
#include "unet_blocks.h"
#include "conv_plan.h"

namespace pf {

void res_rows(WeightTable& wt, const std::string& p, const ResNames& nm, int ci, int co, bool wino, ResW& r) {
  const std::string n1 = p + "." + nm.norm1, c1 = p + "." + nm.conv1, n2 = p + "." + nm.norm2, c2 = p + "." + nm.conv2, sk = p + "." + nm.skip;
  r.gn1_g = wt.raw(n1 + ".weight", {ci});
  r.gn1_b = wt.raw(n1 + ".bias", {ci});
  r.w1 = wt.gemm(c1 + ".weight", co, ci, 9);
  // the Winograd F(2x2, 3x3) packing beside it where the fused form can run (conv_wino.hip: 16x16-pixel tiles, 64-channel blocks)
  if (wino) {
    r.wino1 = wt.alloc((size_t)16 * ci * co);
    wt.params.back().dests.push_back(Dest{D_WINO, r.wino1, 9, ci, co, co, 0});
  }
  r.b1 = wt.raw(c1 + ".bias", {co});
  r.gn2_g = wt.raw(n2 + ".weight", {co});
  r.gn2_b = wt.raw(n2 + ".bias", {co});
  r.w2 = wt.gemm(c2 + ".weight", co, co, 9);
  if (wino && ci == co) {   // (a channel-changing block folds its 1x1 shortcut into this conv: direct form only)
    r.wino2 = wt.alloc((size_t)16 * co * co);
    wt.params.back().dests.push_back(Dest{D_WINO, r.wino2, 9, co, co, co, 0});
  }
  r.b2 = wt.raw(c2 + ".bias", {co});
  if (ci != co) {
    r.wskip = wt.gemm(sk + ".weight", co, ci, 1);
    wt.params.back().shape = {co, ci, 1, 1};
    r.bskip = wt.raw(sk + ".bias", {co});
  }
}

void BlockCtx::conv(pf_conv_args a, Tn* out, bool persist, const float* w_own) {
  const int cin_ = a.c0 + a.c1;
  const bool bf3 = o.precision == PF_PREC_BF16X3 && cin_ % 32 == 0;
  if (bf3) a.precision = PF_PREC_BF16X3;   // decided before the tile (and thus the statistics layout) is chosen
  a.absmax_slot = o.amax_slot;
  a.no_t16 = o.opt[PF_OPT_CONV_T16] == PF_OPT_OFF;
  a.no_pp = o.opt[PF_OPT_CONV_PP] == PF_OPT_OFF;
  ConvPlan pl = conv_plan(a);   // (the args carry no K-split scratch yet: the plan says how much it wants, and is then told that it got it)
  if (pl.splitk_ws_bytes) {     // small-M layer: K-split partial sums live in the temp region
    float* ws = talloc(pl.splitk_ws_bytes / 4);
    a.splitk_ws = dry ? (void*)1 : (void*)ws; a.splitk_ws_bytes = pl.splitk_ws_bytes;
    conv_plan_grant_split(pl, a);
  }
  if (out) {
    *out = Tn{a.out, a.n};
    if (o.tile_stats) {
      out->nt = pl.stats_tiles;
      float* sb = persist ? palloc((size_t)B * out->nt * a.n * 2) : talloc((size_t)B * out->nt * a.n * 2);
      a.stats_out = sb;
      out->st = sb;
    }
  }
  launch(a.ks == 3 ? PF_K_CONV3 : PF_K_GEMM, pl.flops, [&] {
    if (w_own) a.w = w_own;                                        // (folded upsampling conv)
    else if (bf3) a.w += split_offset(a.ks * a.ks, cin_, a.n);     // the region's split packing
    return launch_conv(a, s);
  }, 1, pl.direct_flops);
}

void BlockCtx::stats_pass(Tn& x, int hw, bool persist) {
  const int ns = gn_nsplit(hw);
  float* sb = persist ? palloc((size_t)B * ns * x.c * 2) : talloc((size_t)B * ns * x.c * 2);
  launch(PF_K_GNSTAT, 0.0, [&] { return launch_gn_partial(x.d, x.c, nullptr, 0, B, hw, sb, s); });
  x.st = sb; x.nt = ns;
}

BlockCtx::GnRef BlockCtx::gn(const Tn& x0, const Tn& x1, int hw, int groups, float eps, size_t g, size_t b_, float* sc, float* sh, bool fuse_ok) {
  const int cin_ = x0.c + x1.c;
  if (x0.nt == 0 && cin_ <= 1024) {   // no producer statistics: one pass over the data (partial + finalize)
    const size_t sb = gn_scratch_bytes(B, cin_, hw);
    float* scr = talloc(sb / 4);
    launch(PF_K_GNSTAT, 0.0, [&] { return launch_gn_scale_shift(x0.d, x0.c, x1.d, x1.c, B, hw, groups, eps, w(g), w(b_), sc, sh, scr, sb, s); }, 2);
    return GnRef{};
  }
  Tn s0 = x0, s1 = x1;
  // ... and above 1024 channels (pf_ddpm's 2048 / 1280 concats) a statistics pass per source, combined by the finalize launch
  if (x0.nt == 0) { stats_pass(s0, hw, false); stats_pass(s1, hw, false); }
  // Folding the reduction over the tiles into the consumer is worth it when a sample has few statistics tiles (the 32x32 / 16x16 levels:
  // <= 16 tiles), where the 5 us finalize launch is 10-20 % of the convolution it feeds; at the 128x128 / 64x64 levels every consumer
  // workgroup would re-read 32-64 KB, so the launch stays.
  // (<= 32 tiles - the 64x64 level too - measured neutral in round 5 with the batched statistics loads, -0.9 % before them; <= 128: -3 %)
  constexpr int fold_max = 16;
  if (fuse_ok && o.precision == PF_PREC_BF16X3 && cin_ % 32 == 0 && cin_ <= 1024 && s0.nt <= fold_max && (s1.c == 0 || s1.nt <= fold_max)) {
    GnRef r; r.fused = true; r.s0 = s0.st; r.t0 = s0.nt; r.s1 = s1.st; r.t1 = s1.nt; r.g = g; r.b = b_; r.eps = eps; r.groups = groups;
    return r;
  }
  launch(PF_K_GNSTAT, 0.0, [&] { return launch_gn_finalize_tiles(s0.st, s0.nt, s0.c, s1.st, s1.nt, s1.c, B, hw, groups, eps, w(g), w(b_), sc, sh, s, x1mod(x1)); });
  return GnRef{};
}

void BlockCtx::gn_attach(pf_conv_args& a, const GnRef& r) {
  if (!r.fused) return;
  a.gn_stats0 = dry ? (const float*)16 : r.s0; a.gn_tiles0 = r.t0; a.gn_stats1 = r.s1; a.gn_tiles1 = r.t1;
  a.gn_gamma = w(r.g); a.gn_beta = w(r.b); a.gn_eps = r.eps; a.gn_groups = r.groups;
}

// the fused Winograd form of a ResBlock conv (PF_OPT_CONV_WINO; the AUTO rule: conv_wino_auto, conv_plan.hip)
void BlockCtx::wino_attach(pf_conv_args& a, size_t wino_off) {
  const int v = o.opt[PF_OPT_CONV_WINO];
  if (!wino_off || v == PF_OPT_OFF || o.precision != PF_PREC_BF16X3) return;
  if (v == PF_OPT_AUTO && !conv_wino_auto(a)) return;
  a.w_wino = dry ? (const void*)16 : (const void*)w(wino_off);
  a.wino = 1;
}

Tn BlockCtx::res_block(const ResW& L, const Tn& x0, const Tn& x1, int H, int W_, int co, float eps, bool time_bias) {
  const int hw = H * W_, ci = x0.c + x1.c;
  float* out = palloc((size_t)B * hw * co);
  treset();
  float* sc1 = talloc((size_t)B * ci); float* sh1 = talloc((size_t)B * ci);
  float* h = talloc((size_t)B * hw * co);
  float* sc2 = talloc((size_t)B * co); float* sh2 = talloc((size_t)B * co);
  const GnRef g1 = gn(x0, x1, hw, 32, eps, L.gn1_g, L.gn1_b, sc1, sh1, true);
  Tn ht;
  {
    pf_conv_args a = conv_base(x0.d, x0.c, x1.d, x1.c, B, H, W_, 3, w(L.w1), co, h);
    a.prologue = 1; a.sc = sc1; a.sh = sh1; a.bias = w(L.b1);
    gn_attach(a, g1);
    if (time_bias) {
      a.sbias = dry ? nullptr : tb + L.emb_off; a.ld_sbias = tb_ld;
      a.sbias_rows = tb_rows; a.sbias_nrows = tb_nrows;
    }
    a.x1_bmod = x1mod(x1);
    wino_attach(a, L.wino1);
    conv(a, &ht, false);
  }
  const GnRef g2 = gn(ht, Tn{}, hw, 32, eps, L.gn2_g, L.gn2_b, sc2, sh2, true);
  // split modes: the 1x1 shortcut conv is folded into the second 3x3 conv as one more K range (no round trip of the projected tensor
  // through HBM, one launch less)
  const bool fuse_skip = ci != co && o.precision == PF_PREC_BF16X3 && x0.c % 32 == 0 && x1.c % 32 == 0 && co % 32 == 0;
  pf_conv_args a = conv_base(h, co, nullptr, 0, B, H, W_, 3, w(L.w2), co, out);
  a.prologue = 1; a.sc = sc2; a.sh = sh2; a.bias = w(L.b2);
  gn_attach(a, g2);
  if (fuse_skip) {
    a.skip_x0 = x0.d; a.skip_c0 = x0.c; a.skip_x1 = x1.d; a.skip_c1 = x1.c;
    a.skip_w = w_split(L.wskip, 1, ci, co);
    a.skip_bias = w(L.bskip);
    a.x1_bmod = x1mod(x1);
  } else {
    a.res = x0.d; a.ld_res = co;
    if (ci != co) {
      float* sk = talloc((size_t)B * hw * co);
      pf_conv_args p = conv_base(x0.d, x0.c, x1.d, x1.c, B, 1, hw, 1, w(L.wskip), co, sk);
      p.bias = w(L.bskip);
      p.x1_bmod = x1mod(x1);
      conv(p);
      a.res = sk;
    }
  }
  wino_attach(a, L.wino2);
  Tn ot;
  conv(a, &ot, true);
  return ot;
}

Tn BlockCtx::downsample(const Tn& x, int H, int W_, size_t wgt, size_t bias, int co, int pad_mode) {
  float* od = palloc((size_t)B * (H / 2) * (W_ / 2) * co);
  pf_conv_args a = conv_base(x.d, x.c, nullptr, 0, B, H, W_, 3, w(wgt), co, od);
  a.stride = 2; a.bias = w(bias); a.pad_mode = pad_mode;
  Tn ot;
  conv(a, &ot, true);
  return ot;
}

Tn BlockCtx::upsample_fold(const Tn& x, int H, int W_, size_t w_fold, size_t bias, int co) {
  float* od = palloc((size_t)B * (H * 2) * (W_ * 2) * co);
  pf_conv_args a = conv_base(x.d, x.c, nullptr, 0, B, H, W_, 3, w(w_fold), co, od);
  a.ups = 1; a.ups_fold = 1; a.precision = PF_PREC_BF16X3; a.bias = w(bias);
  Tn ot;
  conv(a, &ot, true, w(w_fold));
  return ot;
}

Tn BlockCtx::stem(const float* x_nchw, size_t wgt, size_t bias, int cin, int co, int H, int W_) {
  float* od = palloc((size_t)B * H * W_ * co);
  // the stem conv emits the per-tile channel statistics of its output itself when it can (the usual 2 -> 64 stem); otherwise a
  // statistics pass over the output follows
  const int nst = o.tile_stats ? launch_conv_in_stats_tiles(cin, co, H, W_) : 0;
  float* sb = nst ? palloc((size_t)B * nst * co * 2) : nullptr;
  launch(PF_K_SMALL, 2.0 * B * H * W_ * 9.0 * cin * co, [&] { return launch_conv_in(x_nchw, w(wgt), w(bias), od, B, cin, co, H, W_, s, sb); });
  Tn ot{od, co, sb, nst};
  if (o.tile_stats && !nst) stats_pass(ot, H * W_, true);
  return ot;
}

void BlockCtx::head(const Tn& x, int H, int W_, int groups, size_t g, size_t b_, size_t wgt, size_t bias, int co, float* out_nchw, float eps) {
  treset();
  float* sc = talloc((size_t)B * x.c); float* sh = talloc((size_t)B * x.c);
  gn(x, Tn{}, H * W_, groups, eps, g, b_, sc, sh);
  launch(PF_K_SMALL, 2.0 * B * H * W_ * 9.0 * x.c * co, [&] { return launch_conv_out(x.d, sc, sh, w(wgt), w(bias), out_nchw, B, x.c, co, H, W_, s); });
}

}  // namespace pf
