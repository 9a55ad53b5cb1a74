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
#include "unet_blocks.h"

namespace pf {
namespace {

struct DLayer {
  int kind;               // 1 ResidualBlock, 2 AttentionBlock, 3 Downsample, 4 Upsample
  int cin, cskip, cout;   // ResidualBlock input = concat(x [cin], skip [cskip]) (up path); others: cin == cout
  ResW r;                 // res
  size_t w1, b1, w2, b2;  // attn: w1/b1 = projection, w2/b2 = output; down / up: w1/b1
  size_t wt_bf3;          // upsample: parity-folded split packing of the ConvT weight (w1 = its fp32 packing)
  bool pop;               // up-path ResidualBlock: consumes a skip
};

}  // namespace
}  // namespace pf

using namespace pf;

struct pf_ddpm {
  pf_ddpm_cfg cfg;
  int final_ch = 0;
  std::vector<DLayer> down, mid, up;   // down / up: in module order; a down entry's output is a skip
  WeightTable wt;
  TimeBias tbias;
  size_t in_w, in_b, te_w1, te_b1, te_w2, te_b2, out_g, out_b, out_w, out_bias;
  PlanOpts po;            // the precision; nothing else is switched on
};

namespace pf {
namespace {

const ResNames kResNames = {"norm1", "conv1", "time_emb", "norm2", "conv2", "shortcut"};

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
    case 1:
      res_rows(u->wt, p, kResNames, L.cin + L.cskip, L.cout, false, L.r);
      u->tbias.rows(u->wt, p + "." + kResNames.emb, L.cout, L.r.emb_off);
      break;
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
  const int d_t = u->tbias.d_t = 4 * c.n_channels;
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
      if (L.kind == 1) L.r.emb_off = u->tbias.take(L.cout);
  u->tbias.alloc(u->wt);

  // parameter table in the reference's state_dict order
  u->in_w = u->wt.raw("image_proj.weight", {c.n_channels, c.image_channels, 3, 3});
  u->in_b = u->wt.raw("image_proj.bias", {c.n_channels});
  u->te_w1 = u->wt.raw("time_emb.lin1.weight", {d_t, d_t / 4});
  u->te_b1 = u->wt.raw("time_emb.lin1.bias", {d_t});
  u->te_w2 = u->wt.raw("time_emb.lin2.weight", {d_t, d_t});
  u->te_b2 = u->wt.raw("time_emb.lin2.bias", {d_t});
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
// AttentionBlock.forward (unet.py:185-215): output(softmax(q k^T d^-0.5) v) + x, one head, q | k | v = projection(x); no norm
Tn run_attn(BlockCtx& c, const DLayer& L, const Tn& x, int H, int W_) {
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
  return Tn{out, C};
}

int run(const pf_ddpm* u, BlockCtx& c, const float* x, const int64_t* t, float* eps) {
  const pf_ddpm_cfg& cfg = u->cfg;
  const int B = c.B;
  int H = cfg.img_h, W_ = cfg.img_w;
  const TimeBias& tbs = u->tbias;
  float* temb = c.palloc((size_t)B * tbs.d_t);
  float* tb = c.palloc((size_t)B * tbs.sum);
  c.tb = tb; c.tb_ld = tbs.sum;
  c.launch(PF_K_SMALL, 0.0, [&] { return launch_ddpm_time_embed(t, c.w(u->te_w1), c.w(u->te_b1), c.w(u->te_w2), c.w(u->te_b2), temb, B, tbs.d_t, c.s); });
  c.launch(PF_K_SMALL, 0.0, [&] { return launch_matvec(temb, tbs.d_t, c.w(tbs.w), c.w(tbs.b), tb, tbs.sum, B, tbs.sum, tbs.d_t, c.s); });

  Tn cur = c.stem(x, u->in_w, u->in_b, cfg.image_channels, cfg.n_channels, H, W_);
  std::vector<Tn> skips{cur};
  auto step = [&](const DLayer& L, const Tn& skip) {
    switch (L.kind) {
      // ResidualBlock.forward (unet.py:128-141): conv2(Swish(GN(conv1(Swish(GN(x))) + time_emb(t)))) + shortcut(x)
      case 1: cur = c.res_block(L.r, cur, skip, H, W_, L.cout); break;
      case 2: cur = run_attn(c, L, cur, H, W_); break;
      case 3:
        cur = c.downsample(cur, H, W_, L.w1, L.b1, L.cout);
        H /= 2; W_ /= 2;
        break;
      case 4:
        if (c.o.precision == PF_PREC_BF16X3 && L.cin % 32 == 0) {   // the split conv's parity-folded upsampling path on the ConvT fold
          cur = c.upsample_fold(cur, H, W_, L.wt_bf3, L.b1, L.cout);
        } else {
          float* od = c.palloc((size_t)B * (2 * H) * (2 * W_) * L.cout);
          c.launch(PF_K_CONV3, 2.0 * B * (4.0 * H * W_) * L.cout * 4.0 * L.cin,
                   [&] { return launch_convT_f32(cur.d, B, H, W_, L.cin, c.w(L.w1), L.cout, c.w(L.b1), od, c.s); });
          cur = Tn{od, L.cout};
        }
        H *= 2; W_ *= 2;
        break;
    }
  };
  // h.append(x) after every module of self.down (unet.py:408-410): a DownBlock is its ResidualBlock plus the AttentionBlock behind it
  for (size_t i = 0; i < u->down.size(); ++i) {
    step(u->down[i], Tn{});
    if (i + 1 == u->down.size() || u->down[i + 1].kind != 2) skips.push_back(cur);
  }
  for (const DLayer& L : u->mid) step(L, Tn{});
  for (const DLayer& L : u->up) {
    Tn sk;
    if (L.pop) { sk = skips.back(); skips.pop_back(); }   // x = cat((x, s), dim=1) (unet.py:416-418): channel order [x, skip]
    step(L, sk);
  }
  // final(Swish(GroupNorm(8)(x))) -> NCHW
  c.head(cur, H, W_, 8, u->out_g, u->out_b, u->out_w, u->out_bias, cfg.image_channels, eps);
  return c.rc;
}

BlockCtx make_ctx(const pf_ddpm* u, int batch) {
  BlockCtx c;
  c.o = u->po; c.B = batch;
  return c;
}
PlanSize ddpm_plan(const pf_ddpm* u, int batch) { return plan_sizes(make_ctx(u, batch), [u](BlockCtx& d) { run(u, d, nullptr, nullptr, nullptr); }); }

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
  u->po.precision = precision;
  return PF_OK;
}
int pf_ddpm_get_precision(const pf_ddpm* u) { return u ? u->po.precision : -1; }

size_t pf_ddpm_workspace_bytes(const pf_ddpm* u, int batch) { return (u && batch > 0) ? ddpm_plan(u, batch).bytes() : 0; }
int pf_ddpm_n_launches(const pf_ddpm* u, int batch) { return (u && batch > 0) ? ddpm_plan(u, batch).n_launch : 0; }
double pf_ddpm_flops(const pf_ddpm* u, int batch) { return (u && batch > 0) ? ddpm_plan(u, batch).flops : 0.0; }

int pf_ddpm_forward(pf_ddpm* u, const float* x, const int64_t* t, int batch, float* eps, void* workspace, size_t workspace_bytes, void* stream) {
  PF_REQUIRE(u && x && t && eps && workspace && batch > 0, "pf_ddpm_forward: bad arguments");
  if (!u->wt.wdev) return set_error(PF_ESTATE, "pf_ddpm_forward: weights not bound (call pf_ddpm_bind_weights)");
  BlockCtx c = make_ctx(u, batch);
  const int rc = c.use_workspace("pf_ddpm_forward", workspace, workspace_bytes, ddpm_plan(u, batch), stream, u->wt.wdev);
  if (rc != PF_OK) return rc;
  return run(u, c, x, t, eps);
}

}  // extern "C"
