// ddpm_unet.hip - host-side plan of the vanilla DDPM noise predictor (ddpm/unet.py:291-421 of the reference, the `ddpm` model of
// main.py / params/ddpm.yaml) and the pf_ddpm_* C ABI.
//
// The walk follows UNet.__init__ / forward; the quirks of the reference are kept: channel multipliers compound (out = in * ch_mults[i]),
// the ResBlock's time_emb Linear is applied to the time embedding with no activation in front, AttentionBlock is one head with
// d_k = n_channels and never applies its `norm` (its keys are accepted and dropped), Upsample is ConvTranspose2d(4, 2, 1), the final norm
// is GroupNorm(8, n_channels).  Every arithmetic step is a launch of a gfx950 kernel: the implicit-GEMM convs of conv_mfma.hip /
// conv_bf16x3.hip (GroupNorm + Swish prologue, time bias, fused 1x1 shortcut, stride 2, the parity-folded upsampling path), the GroupNorm
// statistics of norm_stats.hip, the stem / head convs and mat-vec of small_kernels.hip, the wide-head attention, fp32 ConvT and time
// embedding of attention_wide.hip.  As for pf_unet, the library allocates no device memory: one packed weight blob, one workspace.
#include <memory>
#include <vector>
#include "plan.h"

namespace pf {
namespace {

struct DLayer {
  int kind;               // 1 ResidualBlock, 2 AttentionBlock, 3 Downsample, 4 Upsample
  int cin, cskip, cout;   // ResidualBlock input = concat(x [cin], skip [cskip]) (up path); others: cin == cout
  size_t g1, be1, w1, b1, g2, be2, w2, b2, wsk, bsk;   // res (w*: fp32 packing followed by the split packing); attn: w1/b1 = projection, w2/b2 = output
  size_t wt_bf3;          // upsample: parity-folded split packing of the ConvT weight (w1 = its fp32 packing)
  int emb_off;            // res: column offset into the all-ResBlock time-bias matrix
  bool pop;               // up-path ResidualBlock: consumes a skip
};

}  // namespace
}  // namespace pf

using namespace pf;

struct pf_ddpm {
  pf_ddpm_cfg cfg;
  int d_t = 0, sum_emb = 0, final_ch = 0;
  std::vector<DLayer> down, mid, up;   // down / up: in module order; a down entry's output is a skip
  WeightTable wt;
  size_t in_w, in_b, te_w1, te_b1, te_w2, te_b2, emb_w, emb_b, out_g, out_b, out_w, out_bias;
  int precision = PF_PREC_F32;
};

namespace pf {
namespace {

void build_res(pf_ddpm* u, const std::string& p, DLayer& L) {
  const int ci = L.cin + L.cskip, co = L.cout;
  L.g1 = u->wt.raw(p + ".norm1.weight", {ci});
  L.be1 = u->wt.raw(p + ".norm1.bias", {ci});
  L.w1 = u->wt.gemm(p + ".conv1.weight", co, ci, 9);
  L.b1 = u->wt.raw(p + ".conv1.bias", {co});
  L.g2 = u->wt.raw(p + ".norm2.weight", {co});
  L.be2 = u->wt.raw(p + ".norm2.bias", {co});
  L.w2 = u->wt.gemm(p + ".conv2.weight", co, co, 9);
  L.b2 = u->wt.raw(p + ".conv2.bias", {co});
  if (ci != co) {
    L.wsk = u->wt.gemm(p + ".shortcut.weight", co, ci, 1);
    u->wt.params.back().shape = {co, ci, 1, 1};
    L.bsk = u->wt.raw(p + ".shortcut.bias", {co});
  }
  // time_emb rows live in the all-ResBlock matrix (one mat-vec launch per forward)
  u->wt.raw_at(p + ".time_emb.weight", {co, u->d_t}, u->emb_w + (size_t)L.emb_off * u->d_t);
  u->wt.raw_at(p + ".time_emb.bias", {co}, u->emb_b + (size_t)L.emb_off);
}

void build_attn(pf_ddpm* u, const std::string& p, DLayer& L) {
  const int C = L.cout;
  u->wt.add(p + ".norm.weight", {C});   // defined and saved by the reference, never applied (unet.py:170, 185-215): accepted, dropped
  u->wt.add(p + ".norm.bias", {C});
  L.w1 = u->wt.gemm(p + ".projection.weight", 3 * C, C, 1);
  L.b1 = u->wt.raw(p + ".projection.bias", {3 * C});
  L.w2 = u->wt.gemm(p + ".output.weight", C, C, 1);
  L.b2 = u->wt.raw(p + ".output.bias", {C});
}

void build_layer(pf_ddpm* u, const std::string& p, DLayer& L) {
  switch (L.kind) {
    case 1: build_res(u, p, L); break;
    case 2: build_attn(u, p, L); break;
    case 3:
      L.w1 = u->wt.gemm(p + ".conv.weight", L.cout, L.cin, 9);
      L.b1 = u->wt.raw(p + ".conv.bias", {L.cout});
      break;
    case 4: {
      const int C = L.cout;
      L.w1 = u->wt.alloc((size_t)16 * C * C);
      L.wt_bf3 = u->wt.alloc(gemm_floats(16, C, C));
      Param& ps = u->wt.add(p + ".conv.weight", {C, C, 4, 4});
      ps.dests.push_back(Dest{D_CONVT_F32, L.w1, 16, C, C, C, 0});
      ps.dests.push_back(Dest{D_CONVT_BF3, L.wt_bf3, 16, C, C, (C + 63) / 64 * 64, 0});
      L.b1 = u->wt.raw(p + ".conv.bias", {C});
      break;
    }
  }
}

int build(pf_ddpm* u) {
  const pf_ddpm_cfg& c = u->cfg;
  PF_REQUIRE(c.n_levels >= 1 && c.n_levels <= 8 && c.n_blocks >= 1, "ddpm: bad level / block counts");
  PF_REQUIRE(c.n_channels > 0 && c.n_channels % 32 == 0, "ddpm: n_channels must be a multiple of 32 (GroupNorm(32)), got %d", c.n_channels);
  PF_REQUIRE(c.image_channels >= 1 && c.image_channels <= 4, "ddpm: image_channels must be 1..4");
  PF_REQUIRE(c.img_h % (1 << (c.n_levels - 1)) == 0 && c.img_w % (1 << (c.n_levels - 1)) == 0, "ddpm: image size must be divisible by 2^(levels-1)");
  u->d_t = 4 * c.n_channels;
  // architecture walk (unet.py:352-386)
  auto res = [](int ci, int cs, int co, bool pop) { DLayer L{}; L.kind = 1; L.cin = ci; L.cskip = cs; L.cout = co; L.pop = pop; return L; };
  auto one = [](int kind, int ch) { DLayer L{}; L.kind = kind; L.cin = L.cout = ch; return L; };
  std::vector<int> h_ch{c.n_channels};
  int in_ch = c.n_channels, out_ch = c.n_channels;
  for (int i = 0; i < c.n_levels; ++i) {
    PF_REQUIRE(c.ch_mults[i] >= 1, "ddpm: bad channel multiplier");
    out_ch = in_ch * c.ch_mults[i];
    PF_REQUIRE(out_ch % 32 == 0 && out_ch <= 4096, "ddpm: level %d has %d channels", i, out_ch);
    for (int j = 0; j < c.n_blocks; ++j) {
      u->down.push_back(res(in_ch, 0, out_ch, false));
      if (c.is_attn[i]) u->down.push_back(one(2, out_ch));
      in_ch = out_ch;
      h_ch.push_back(in_ch);
    }
    if (i < c.n_levels - 1) { u->down.push_back(one(3, in_ch)); h_ch.push_back(in_ch); }
  }
  u->mid = {res(out_ch, 0, out_ch, false), one(2, out_ch), res(out_ch, 0, out_ch, false)};
  in_ch = out_ch;
  for (int i = c.n_levels - 1; i >= 0; --i) {
    out_ch = in_ch;
    for (int j = 0; j <= c.n_blocks; ++j) {
      if (j == c.n_blocks) out_ch = in_ch / c.ch_mults[i];
      const int sk = h_ch.back(); h_ch.pop_back();
      PF_REQUIRE(sk == out_ch, "ddpm: skip of %d channels meets an UpBlock built for %d (inconsistent ch_mults)", sk, out_ch);
      u->up.push_back(res(in_ch, sk, out_ch, true));
      if (c.is_attn[i]) u->up.push_back(one(2, out_ch));
    }
    in_ch = out_ch;
    if (i > 0) u->up.push_back(one(4, in_ch));
  }
  u->final_ch = in_ch;
  for (auto* v : {&u->down, &u->mid, &u->up})
    for (DLayer& L : *v)
      if (L.kind == 1) { L.emb_off = u->sum_emb; u->sum_emb += L.cout; }
  u->emb_w = u->wt.alloc((size_t)u->sum_emb * u->d_t);
  u->emb_b = u->wt.alloc((size_t)u->sum_emb);

  // parameter table in the reference's state_dict order
  u->in_w = u->wt.raw("image_proj.weight", {c.n_channels, c.image_channels, 3, 3});
  u->in_b = u->wt.raw("image_proj.bias", {c.n_channels});
  u->te_w1 = u->wt.raw("time_emb.lin1.weight", {u->d_t, u->d_t / 4});
  u->te_b1 = u->wt.raw("time_emb.lin1.bias", {u->d_t});
  u->te_w2 = u->wt.raw("time_emb.lin2.weight", {u->d_t, u->d_t});
  u->te_b2 = u->wt.raw("time_emb.lin2.bias", {u->d_t});
  static const char* sub[5] = {"", ".res", ".attn", "", ""};
  int mod = -1;
  for (DLayer& L : u->down) {
    if (L.kind != 2) ++mod;   // a DownBlock's attn shares the block index of its res
    build_layer(u, "down." + std::to_string(mod) + sub[L.kind], L);
  }
  static const char* msub[3] = {"middle.res1", "middle.attn", "middle.res2"};
  for (int i = 0; i < 3; ++i) build_layer(u, msub[i], u->mid[i]);
  mod = -1;
  for (DLayer& L : u->up) {
    if (L.kind != 2) ++mod;
    build_layer(u, "up." + std::to_string(mod) + sub[L.kind], L);
  }
  u->out_g = u->wt.raw("norm.weight", {u->final_ch});
  u->out_b = u->wt.raw("norm.bias", {u->final_ch});
  u->out_w = u->wt.alloc((size_t)c.image_channels * 9 * u->final_ch);
  u->wt.add("final.weight", {c.image_channels, u->final_ch, 3, 3}).dests.push_back(Dest{D_CONVOUT, u->out_w, 9, u->final_ch, c.image_channels, 0, 0});
  u->out_bias = u->wt.raw("final.bias", {c.image_channels});
  return PF_OK;
}

// ---- forward ----
struct DT { const float* d = nullptr; int c = 0; };

struct DCtx : PlanCtx {
  pf_ddpm* u = nullptr;
  void conv(pf_conv_args a) {
    const int cin = a.c0 + a.c1;
    const bool bf3 = u->precision == PF_PREC_BF16X3 && cin % 32 == 0;
    if (bf3) a.precision = PF_PREC_BF16X3;
    if (const size_t wsb = conv_splitk_ws_bytes(a)) {
      float* ws = talloc(wsb / 4);
      a.splitk_ws = dry ? (void*)1 : (void*)ws; a.splitk_ws_bytes = wsb;
    }
    launch(a.ks == 3 ? PF_K_CONV3 : PF_K_GEMM, conv_flops(a), [&] {
      if (bf3) a.w += split_offset(a.ks * a.ks, cin, a.n);   // the region's split packing
      return launch_conv(a, s);
    });
  }
  // GroupNorm scale / shift of concat(x0, x1): one statistics pass + finalize; above 1024 channels (the up path's 2048 / 1280 concats)
  // the two sources get a statistics pass each and the separate finalize launch combines them
  void gn(const DT& x0, const DT& x1, int hw, int groups, size_t g, size_t b, float* sc, float* sh) {
    const int C = x0.c + x1.c;
    if (C <= 1024) {
      const size_t sb = gn_scratch_bytes(B, C, hw);
      float* scr = talloc(sb / 4);
      launch(PF_K_GNSTAT, 0.0, [&] { return launch_gn_scale_shift(x0.d, x0.c, x1.d, x1.c, B, hw, groups, 1e-5f, w(g), w(b), sc, sh, scr, sb, s); },
             2);   // (partial + finalize)
      return;
    }
    const int ns = gn_nsplit(hw);
    float* s0 = talloc((size_t)B * ns * x0.c * 2);
    float* s1 = talloc((size_t)B * ns * x1.c * 2);
    launch(PF_K_GNSTAT, 0.0, [&] { return launch_gn_partial(x0.d, x0.c, nullptr, 0, B, hw, s0, s); });
    launch(PF_K_GNSTAT, 0.0, [&] { return launch_gn_partial(x1.d, x1.c, nullptr, 0, B, hw, s1, s); });
    launch(PF_K_GNSTAT, 0.0, [&] { return launch_gn_finalize_tiles(s0, ns, x0.c, s1, ns, x1.c, B, hw, groups, 1e-5f, w(g), w(b), sc, sh, s); });
  }
};

// ResidualBlock.forward (unet.py:128-141): conv2(Swish(GN(conv1(Swish(GN(x))) + time_emb(t)))) + shortcut(x)
DT run_res(DCtx& c, const DLayer& L, const DT& x0, const DT& x1, int H, int W_, const float* tb) {
  const int B = c.B, hw = H * W_, ci = x0.c + x1.c, co = L.cout;
  float* out = c.palloc((size_t)B * hw * co);
  c.treset();
  float* sc1 = c.talloc((size_t)B * ci); float* sh1 = c.talloc((size_t)B * ci);
  float* h = c.talloc((size_t)B * hw * co);
  float* sc2 = c.talloc((size_t)B * co); float* sh2 = c.talloc((size_t)B * co);
  c.gn(x0, x1, hw, 32, L.g1, L.be1, sc1, sh1);
  {
    pf_conv_args a = conv_base(x0.d, x0.c, x1.d, x1.c, B, H, W_, 3, c.w(L.w1), co, h);
    a.prologue = 1; a.sc = sc1; a.sh = sh1; a.bias = c.w(L.b1);
    a.sbias = c.dry ? nullptr : tb + L.emb_off; a.ld_sbias = c.u->sum_emb;
    c.conv(a);
  }
  c.gn(DT{h, co}, DT{}, hw, 32, L.g2, L.be2, sc2, sh2);
  const float* resid = x0.d;
  const bool fuse = ci != co && c.u->precision == PF_PREC_BF16X3;   // 1x1 shortcut as one more K range of conv2 (split modes)
  if (ci != co && !fuse) {
    float* sk = c.talloc((size_t)B * hw * co);
    pf_conv_args a = conv_base(x0.d, x0.c, x1.d, x1.c, B, 1, hw, 1, c.w(L.wsk), co, sk);
    a.bias = c.w(L.bsk);
    c.conv(a);
    resid = sk;
  }
  pf_conv_args a = conv_base(h, co, nullptr, 0, B, H, W_, 3, c.w(L.w2), co, out);
  a.prologue = 1; a.sc = sc2; a.sh = sh2; a.bias = c.w(L.b2);
  if (fuse) {
    a.skip_x0 = x0.d; a.skip_c0 = x0.c; a.skip_x1 = x1.d; a.skip_c1 = x1.c;
    a.skip_w = c.w_split(L.wsk, 1, ci, co);
    a.skip_bias = c.w(L.bsk);
  } else {
    a.res = resid; a.ld_res = co;
  }
  c.conv(a);
  return DT{out, co};
}

// AttentionBlock.forward (unet.py:185-215): output(softmax(q k^T d^-0.5) v) + x, one head, q | k | v = projection(x); no norm
DT run_attn(DCtx& c, const DLayer& L, const DT& x, int H, int W_) {
  const int B = c.B, l = H * W_, C = L.cout, M = B * l;
  float* out = c.palloc((size_t)M * C);
  c.treset();
  float* qkv = c.talloc((size_t)M * 3 * C);
  float* o = c.talloc((size_t)M * C);
  const size_t sfl = attention_wide_scratch_floats(B, l);
  float* scr = c.talloc(sfl);
  {
    pf_conv_args a = conv_base(x.d, C, nullptr, 0, B, 1, l, 1, c.w(L.w1), 3 * C, qkv);
    a.bias = c.w(L.b1);
    c.conv(a);
  }
  c.launch(PF_K_ATTN, 4.0 * B * (double)l * l * C, [&] { return launch_attention_wide(qkv, qkv + C, qkv + 2 * C, 3 * C, o, C, B, l, C, scr, sfl, c.s); },
           3);   // (scores, softmax, output)
  {
    pf_conv_args a = conv_base(o, C, nullptr, 0, B, 1, l, 1, c.w(L.w2), C, out);
    a.bias = c.w(L.b2); a.res = x.d; a.ld_res = C;
    c.conv(a);
  }
  return DT{out, C};
}

int run(pf_ddpm* u, DCtx& c, const float* x, const int64_t* t, float* eps) {
  const pf_ddpm_cfg& cfg = u->cfg;
  const int B = c.B;
  int H = cfg.img_h, W_ = cfg.img_w;
  float* temb = c.palloc((size_t)B * u->d_t);
  float* tb = c.palloc((size_t)B * u->sum_emb);
  c.launch(PF_K_SMALL, 0.0, [&] { return launch_ddpm_time_embed(t, c.w(u->te_w1), c.w(u->te_b1), c.w(u->te_w2), c.w(u->te_b2), temb, B, u->d_t, c.s); });
  c.launch(PF_K_SMALL, 0.0, [&] { return launch_matvec(temb, u->d_t, c.w(u->emb_w), c.w(u->emb_b), tb, u->sum_emb, B, u->sum_emb, u->d_t, c.s); });

  DT cur{c.palloc((size_t)B * H * W_ * cfg.n_channels), cfg.n_channels};
  c.launch(PF_K_SMALL, 2.0 * B * H * W_ * 9.0 * cfg.image_channels * cfg.n_channels,
           [&] { return launch_conv_in(x, c.w(u->in_w), c.w(u->in_b), const_cast<float*>(cur.d), B, cfg.image_channels, cfg.n_channels, H, W_, c.s); });
  std::vector<DT> skips{cur};
  auto step = [&](const DLayer& L, const DT* skip) {
    switch (L.kind) {
      case 1: cur = run_res(c, L, cur, skip ? *skip : DT{}, H, W_, tb); break;
      case 2: cur = run_attn(c, L, cur, H, W_); break;
      case 3: {
        float* od = c.palloc((size_t)B * (H / 2) * (W_ / 2) * L.cout);
        pf_conv_args a = conv_base(cur.d, cur.c, nullptr, 0, B, H, W_, 3, c.w(L.w1), L.cout, od);
        a.stride = 2; a.bias = c.w(L.b1);
        c.conv(a);
        cur = DT{od, L.cout}; H /= 2; W_ /= 2;
        break;
      }
      case 4: {
        float* od = c.palloc((size_t)B * (2 * H) * (2 * W_) * L.cout);
        if (u->precision == PF_PREC_BF16X3 && L.cin % 32 == 0) {   // the split conv's parity-folded upsampling path on the ConvT fold
          pf_conv_args a = conv_base(cur.d, cur.c, nullptr, 0, B, H, W_, 3, c.w(L.wt_bf3), L.cout, od);
          a.ups = 1; a.ups_fold = 1; a.precision = PF_PREC_BF16X3; a.bias = c.w(L.b1);
          c.launch(PF_K_CONV3, conv_flops(a), [&] { return launch_conv(a, c.s); });
        } else {
          c.launch(PF_K_CONV3, 2.0 * B * (4.0 * H * W_) * L.cout * 4.0 * L.cin,
                   [&] { return launch_convT_f32(cur.d, B, H, W_, L.cin, c.w(L.w1), L.cout, c.w(L.b1), od, c.s); });
        }
        cur = DT{od, L.cout}; H *= 2; W_ *= 2;
        break;
      }
    }
  };
  // h.append(x) after every module of self.down (unet.py:408-410): a DownBlock is its ResidualBlock plus the AttentionBlock behind it
  for (size_t i = 0; i < u->down.size(); ++i) {
    step(u->down[i], nullptr);
    if (i + 1 == u->down.size() || u->down[i + 1].kind != 2) skips.push_back(cur);
  }
  for (const DLayer& L : u->mid) step(L, nullptr);
  for (const DLayer& L : u->up) {
    if (L.pop) {   // x = cat((x, s), dim=1) (unet.py:416-418): channel order [x, skip]
      const DT sk = skips.back();
      skips.pop_back();
      step(L, &sk);
    } else {
      step(L, nullptr);
    }
  }
  // final(Swish(GroupNorm(8)(x))) -> NCHW
  c.treset();
  float* sc = c.talloc((size_t)B * cur.c); float* sh = c.talloc((size_t)B * cur.c);
  c.gn(cur, DT{}, H * W_, 8, u->out_g, u->out_b, sc, sh);
  c.launch(PF_K_SMALL, 2.0 * B * H * W_ * 9.0 * cur.c * cfg.image_channels,
           [&] { return launch_conv_out(cur.d, sc, sh, c.w(u->out_w), c.w(u->out_bias), eps, B, cur.c, cfg.image_channels, H, W_, c.s); });
  return c.rc;
}

DCtx make_ctx(const pf_ddpm* u, int batch) {
  DCtx c;
  c.u = const_cast<pf_ddpm*>(u); c.B = batch;
  return c;
}
PlanSize ddpm_plan(const DCtx& c) { return plan_sizes(c, [](DCtx& d) { run(d.u, d, nullptr, nullptr, nullptr); }); }

}  // namespace
}  // namespace pf

extern "C" {

int pf_ddpm_create(const pf_ddpm_cfg* cfg, pf_ddpm** out) {
  PF_REQUIRE(cfg && out, "pf_ddpm_create: null argument");
  std::unique_ptr<pf_ddpm> u(new pf_ddpm());
  u->cfg = *cfg;
  const int rc = build(u.get());
  if (rc != PF_OK) return rc;
  *out = u.release();
  return PF_OK;
}
void pf_ddpm_destroy(pf_ddpm* u) { delete u; }

size_t pf_ddpm_weight_bytes(const pf_ddpm* u) { return u ? u->wt.blob_floats * sizeof(float) : 0; }
int pf_ddpm_n_params(const pf_ddpm* u) { return u ? (int)u->wt.params.size() : 0; }

int pf_ddpm_param_info(const pf_ddpm* u, int i, char* key_buf, size_t key_buf_len, int64_t shape[4], int* ndim) {
  PF_REQUIRE(u, "pf_ddpm_param_info: bad arguments");
  return u->wt.param_info("pf_ddpm_param_info", i, key_buf, key_buf_len, shape, ndim);
}
int pf_ddpm_pack_param(pf_ddpm* u, const char* key, const float* src, const int64_t* shape, int ndim, void* host_blob) {
  PF_REQUIRE(u, "pf_ddpm_pack_param: null argument");
  return u->wt.pack_param("pf_ddpm_pack_param", "DDPM UNet", key, src, shape, ndim, host_blob);
}
int pf_ddpm_pack_missing(const pf_ddpm* u, char* buf, size_t buf_len) { return u ? u->wt.pack_missing(buf, buf_len) : set_error(PF_EINVAL, "null handle"); }
int pf_ddpm_bind_weights(pf_ddpm* u, const void* dev_blob) {
  PF_REQUIRE(u, "pf_ddpm_bind_weights: null argument");
  return u->wt.bind("pf_ddpm_bind_weights", dev_blob, true);
}

int pf_ddpm_set_precision(pf_ddpm* u, int precision) {
  PF_REQUIRE(u && (precision == PF_PREC_F32 || precision == PF_PREC_BF16X3), "pf_ddpm_set_precision: bad arguments");
  u->precision = precision;
  return PF_OK;
}
int pf_ddpm_get_precision(const pf_ddpm* u) { return u ? u->precision : -1; }

size_t pf_ddpm_workspace_bytes(const pf_ddpm* u, int batch) { return (u && batch > 0) ? ddpm_plan(make_ctx(u, batch)).bytes() : 0; }
int pf_ddpm_n_launches(const pf_ddpm* u, int batch) { return (u && batch > 0) ? ddpm_plan(make_ctx(u, batch)).n_launch : 0; }
double pf_ddpm_flops(const pf_ddpm* u, int batch) { return (u && batch > 0) ? ddpm_plan(make_ctx(u, batch)).flops : 0.0; }

int pf_ddpm_forward(pf_ddpm* u, const float* x, const int64_t* t, int batch, float* eps, void* workspace, size_t workspace_bytes, void* stream) {
  PF_REQUIRE(u && x && t && eps && workspace && batch > 0, "pf_ddpm_forward: bad arguments");
  if (!u->wt.wdev) return set_error(PF_ESTATE, "pf_ddpm_forward: weights not bound (call pf_ddpm_bind_weights)");
  DCtx c = make_ctx(u, batch);
  const int rc = c.use_workspace("pf_ddpm_forward", workspace, workspace_bytes, ddpm_plan(c));
  if (rc != PF_OK) return rc;
  c.s = (hipStream_t)stream; c.W = u->wt.wdev;
  return run(u, c, x, t, eps);
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
