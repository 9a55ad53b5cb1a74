// autoencoder.hip - host-side plans of the first-stage autoencoder (stable_diffusion/model/autoencoder.py of the reference: Autoencoder,
// Encoder, Decoder, ResnetBlock, AttnBlock, UpSample, DownSample, GaussianDistribution; the `autoencoder` model of
// params/autoencoder.yaml) and the pf_autoenc_* C ABI.
//
// Two walks over one weight table: encode (image -> posterior moments and a sample of it) and decode (latent -> image).  Both are built
// from the block emitters of unet_blocks.h with this model's GroupNorm eps (1e-6) and no time bias; what the model adds is the
// DownSample's bottom / right-only padding (pf_conv_args.pad_mode), the AttnBlock (GroupNorm without SiLU as the prologue of ONE 1x1
// launch over the packed q | k | v weights, the wide-head attention with d = C, proj_out with the residual), the encoder tail
// (GroupNorm + SiLU + conv_out + quant_conv + clamp + sample as one launch) and the decoder front (z / scale + post_quant_conv + conv_in
// as one launch), both in small_kernels.hip.  The image size is an argument of the calls.  As for the other handles the library
// allocates no device memory and never synchronises.
#include <memory>
#include <vector>
#include "unet_blocks.h"

namespace pf {
namespace {

constexpr float kEps = 1e-6f;   // normalization() of autoencoder.py:484-490

struct ALayer {
  int kind;                 // 1 ResnetBlock, 2 AttnBlock, 3 DownSample, 4 UpSample
  int cin, cout;
  int level;                // index of the `down` / `up` entry it belongs to (-1: mid)
  std::string name;         // state_dict prefix under encoder. / decoder.
  ResW r;
  size_t ng, nb, qkv, qkv_b, pw, pb;   // attn: norm, packed q | k | v (N = 3C) and its bias, proj_out
  size_t w1, b1, wfold;     // down / up conv; up: + the parity-folded split packing
};

}  // namespace
}  // namespace pf

using namespace pf;

struct pf_autoenc {
  pf_autoenc_cfg cfg;
  int top_ch = 0;           // channels of the lowest resolution (mid blocks, attention)
  std::vector<ALayer> enc, dec;   // in execution order, between conv_in and norm_out
  WeightTable wt;
  size_t e_in_w, e_in_b, e_ng, e_nb, e_ow, e_ob, q_w, q_b, pq_w, pq_b, d_in_w, d_in_b, d_ng, d_nb, d_ow, d_ob;
  PlanOpts po;              // the precision; nothing else is switched on
};

namespace pf {
namespace {

const ResNames kResNames = {"norm1", "conv1", "", "norm2", "conv2", "nin_shortcut"};

void build_layer(pf_autoenc* u, const std::string& top, ALayer& L) {
  const std::string p = top + L.name;
  const int C = L.cout;
  switch (L.kind) {
    case 1: res_rows(u->wt, p, kResNames, L.cin, L.cout, false, L.r); break;
    case 2: {
      L.ng = u->wt.raw(p + ".norm.weight", {C});
      L.nb = u->wt.raw(p + ".norm.bias", {C});
      // q, k, v (three Conv2d(C, C, 1)) share one GEMM region of N = 3C columns and one bias vector: one launch projects all three
      L.qkv = u->wt.alloc_gemm(1, C, 3 * C);
      L.qkv_b = u->wt.alloc((size_t)3 * C);
      static const char* nm[3] = {".q", ".k", ".v"};
      for (int i = 0; i < 3; ++i) {
        u->wt.add(p + nm[i] + ".weight", {C, C, 1, 1}).dests.push_back(Dest{D_GEMM, L.qkv, 1, C, C, (3 * C + 63) / 64 * 64, i * C});
        u->wt.raw_at(p + nm[i] + ".bias", {C}, L.qkv_b + (size_t)i * C);
      }
      L.pw = u->wt.gemm(p + ".proj_out.weight", C, C, 1);
      u->wt.params.back().shape = {C, C, 1, 1};
      L.pb = u->wt.raw(p + ".proj_out.bias", {C});
      break;
    }
    case 3:
    case 4:
      L.w1 = u->wt.gemm(p + ".conv.weight", C, C, 9);
      if (L.kind == 4) {
        L.wfold = u->wt.alloc(gemm_floats(16, C, C));
        u->wt.params.back().dests.push_back(Dest{D_UPFOLD, L.wfold, 16, C, C, (C + 63) / 64 * 64, 0});
      }
      L.b1 = u->wt.raw(p + ".conv.bias", {C});
      break;
  }
}

ALayer layer(int kind, int ci, int co, int level, std::string name) {
  ALayer L{};
  L.kind = kind; L.cin = ci; L.cout = co; L.level = level; L.name = std::move(name);
  return L;
}

void push_mid(std::vector<ALayer>& v, int C) {
  v.push_back(layer(1, C, C, -1, "mid.block_1"));
  v.push_back(layer(2, C, C, -1, "mid.attn_1"));
  v.push_back(layer(1, C, C, -1, "mid.block_2"));
}

int build(pf_autoenc* u) {
  const pf_autoenc_cfg& c = u->cfg;
  PF_REQUIRE(c.n_levels >= 1 && c.n_levels <= 8 && c.n_resnet_blocks >= 1, "autoenc: bad level / block counts");
  PF_REQUIRE(c.in_channels >= 1 && c.in_channels <= 4 && c.out_channels >= 1 && c.out_channels <= 4, "autoenc: in / out channels must be 1..4");
  PF_REQUIRE(c.z_channels >= 1 && c.z_channels <= 4 && c.emb_channels >= 1 && c.emb_channels <= 4, "autoenc: z / emb channels must be 1..4");
  PF_REQUIRE(c.channels > 0 && c.channels % 32 == 0, "autoenc: channels must be a multiple of 32 (GroupNorm(32)), got %d", c.channels);
  for (int i = 0; i < c.n_levels; ++i)
    PF_REQUIRE(c.channel_multipliers[i] >= 1 && c.channels * c.channel_multipliers[i] <= 1024, "autoenc: level %d: bad channel multiplier %d", i,
               c.channel_multipliers[i]);
  const int L = c.n_levels;
  auto ch = [&](int i) { return c.channels * c.channel_multipliers[i]; };
  u->top_ch = ch(L - 1);
  PF_REQUIRE((size_t)u->top_ch * c.z_channels * 9 * 4 <= 64 * 1024, "autoenc: decoder conv_in %d -> %d does not fit its kernel", c.z_channels, u->top_ch);

  // Encoder.__init__ (autoencoder.py:136-175): level i maps channels_list[i] -> channels_list[i + 1], channels_list = [1] + multipliers
  int cur = c.channels;
  for (int i = 0; i < L; ++i) {
    for (int j = 0; j < c.n_resnet_blocks; ++j) {
      u->enc.push_back(layer(1, cur, ch(i), i, "down." + std::to_string(i) + ".block." + std::to_string(j)));
      cur = ch(i);
    }
    if (i != L - 1) u->enc.push_back(layer(3, cur, cur, i, "down." + std::to_string(i) + ".downsample"));
  }
  push_mid(u->enc, cur);
  // Decoder.__init__ (autoencoder.py:231-273): from the last level up, n_resnet_blocks + 1 blocks per level, UpSample except at level 0
  cur = u->top_ch;
  push_mid(u->dec, cur);
  for (int i = L - 1; i >= 0; --i) {
    for (int j = 0; j <= c.n_resnet_blocks; ++j) {
      u->dec.push_back(layer(1, cur, ch(i), i, "up." + std::to_string(i) + ".block." + std::to_string(j)));
      cur = ch(i);
    }
    if (i != 0) u->dec.push_back(layer(4, cur, cur, i, "up." + std::to_string(i) + ".upsample"));
  }

  // parameter table in the reference's state_dict order: encoder, decoder (`up` in index order: the ModuleList is filled by insert(0)),
  // quant_conv, post_quant_conv
  WeightTable& wt = u->wt;
  u->e_in_w = wt.raw("encoder.conv_in.weight", {c.channels, c.in_channels, 3, 3});
  u->e_in_b = wt.raw("encoder.conv_in.bias", {c.channels});
  for (ALayer& l : u->enc) build_layer(u, "encoder.", l);
  u->e_ng = wt.raw("encoder.norm_out.weight", {u->top_ch});
  u->e_nb = wt.raw("encoder.norm_out.bias", {u->top_ch});
  u->e_ow = wt.alloc((size_t)2 * c.z_channels * 9 * u->top_ch);
  wt.add("encoder.conv_out.weight", {2 * c.z_channels, u->top_ch, 3, 3}).dests.push_back(Dest{D_CONVOUT, u->e_ow, 9, u->top_ch, 2 * c.z_channels, 0, 0});
  u->e_ob = wt.raw("encoder.conv_out.bias", {2 * c.z_channels});
  u->d_in_w = wt.raw("decoder.conv_in.weight", {u->top_ch, c.z_channels, 3, 3});
  u->d_in_b = wt.raw("decoder.conv_in.bias", {u->top_ch});
  for (ALayer& l : u->dec) if (l.level < 0) build_layer(u, "decoder.", l);
  for (int i = 0; i < L; ++i)
    for (ALayer& l : u->dec) if (l.level == i) build_layer(u, "decoder.", l);
  u->d_ng = wt.raw("decoder.norm_out.weight", {ch(0)});
  u->d_nb = wt.raw("decoder.norm_out.bias", {ch(0)});
  u->d_ow = wt.alloc((size_t)c.out_channels * 9 * ch(0));
  wt.add("decoder.conv_out.weight", {c.out_channels, ch(0), 3, 3}).dests.push_back(Dest{D_CONVOUT, u->d_ow, 9, ch(0), c.out_channels, 0, 0});
  u->d_ob = wt.raw("decoder.conv_out.bias", {c.out_channels});
  u->q_w = wt.raw("quant_conv.weight", {2 * c.emb_channels, 2 * c.z_channels, 1, 1});
  u->q_b = wt.raw("quant_conv.bias", {2 * c.emb_channels});
  u->pq_w = wt.raw("post_quant_conv.weight", {c.z_channels, c.emb_channels, 1, 1});
  u->pq_b = wt.raw("post_quant_conv.bias", {c.z_channels});
  return PF_OK;
}

// ---- forward ----
// AttnBlock.forward (autoencoder.py:348-380): x + proj_out(softmax(q^T k C^-0.5) v), q | k | v = 1x1 convs of GroupNorm(x) (no SiLU)
Tn run_attn(BlockCtx& c, const ALayer& L, const Tn& x, int H, int W_) {
  const int B = c.B, l = H * W_, C = L.cout, M = B * l;
  float* out = c.palloc((size_t)M * C);
  c.treset();
  float* sc = c.talloc((size_t)B * C); float* sh = c.talloc((size_t)B * C);
  float* qkv = c.talloc((size_t)M * 3 * C);
  float* o = c.talloc((size_t)M * C);
  const size_t sfl = attention_wide_scratch_floats(B, l);
  float* scr = c.talloc(sfl);
  c.gn(x, Tn{}, l, 32, kEps, L.ng, L.nb, sc, sh);
  {
    pf_conv_args a = conv_base(x.d, C, nullptr, 0, B, 1, l, 1, c.w(L.qkv), 3 * C, qkv);
    a.prologue = 2; a.sc = sc; a.sh = sh; a.bias = c.w(L.qkv_b);
    c.conv(a);
  }
  c.launch(PF_K_ATTN, 4.0 * B * (double)l * l * C, [&] { return launch_attention_wide(qkv, qkv + C, qkv + 2 * C, 3 * C, o, C, B, l, C, scr, sfl, c.s); },
           3);   // (scores, softmax, output)
  {
    pf_conv_args a = conv_base(o, C, nullptr, 0, B, 1, l, 1, c.w(L.pw), C, out);
    a.bias = c.w(L.pb); a.res = x.d; a.ld_res = C;
    c.conv(a);
  }
  return Tn{out, C};
}

// the layers between conv_in and norm_out of either half
Tn run_layers(BlockCtx& c, const std::vector<ALayer>& v, Tn cur, int& H, int& W_) {
  for (const ALayer& L : v) {
    switch (L.kind) {
      case 1: cur = c.res_block(L.r, cur, Tn{}, H, W_, L.cout, kEps, false); break;
      case 2: cur = run_attn(c, L, cur, H, W_); break;
      case 3:   // F.pad(x, (0, 1, 0, 1)) + Conv2d(3, stride 2, padding 0) (autoencoder.py:419-426)
        cur = c.downsample(cur, H, W_, L.w1, L.b1, L.cout, PF_PAD_BOTTOM_RIGHT);
        H /= 2; W_ /= 2;
        break;
      case 4:   // F.interpolate(scale 2, nearest) + Conv2d(3, padding 1) (autoencoder.py:396-403)
        if (c.o.precision == PF_PREC_BF16X3) {
          cur = c.upsample_fold(cur, H, W_, L.wfold, L.b1, L.cout);
        } else {   // nearest-neighbour upsampling inside the conv's gather
          float* od = c.palloc((size_t)c.B * (H * 2) * (W_ * 2) * L.cout);
          pf_conv_args a = conv_base(cur.d, cur.c, nullptr, 0, c.B, H, W_, 3, c.w(L.w1), L.cout, od);
          a.ups = 1; a.bias = c.w(L.b1);
          c.conv(a, &cur, true);
        }
        H *= 2; W_ *= 2;
        break;
    }
  }
  return cur;
}

struct EncArgs { const float* img; float scale; const float* noise; uint64_t seed, sid, off; float *z, *mean, *log_var; };

int run_encode(const pf_autoenc* u, BlockCtx& c, int H, int W_, const EncArgs& e) {
  const pf_autoenc_cfg& cfg = u->cfg;
  Tn cur = c.stem(e.img, u->e_in_w, u->e_in_b, cfg.in_channels, cfg.channels, H, W_);
  cur = run_layers(c, u->enc, cur, H, W_);
  // conv_out(swish(norm_out(x))), quant_conv, GaussianDistribution and its sample: one launch behind the GroupNorm statistics
  c.treset();
  const int C = cur.c, z2 = 2 * cfg.z_channels, e2 = 2 * cfg.emb_channels;
  float* sc = c.talloc((size_t)c.B * C); float* sh = c.talloc((size_t)c.B * C);
  c.gn(cur, Tn{}, H * W_, 32, kEps, u->e_ng, u->e_nb, sc, sh);
  c.launch(PF_K_SMALL, 2.0 * c.B * H * W_ * (9.0 * C * z2 + (double)z2 * e2), [&] {
    return launch_ae_tail(cur.d, sc, sh, c.w(u->e_ow), c.w(u->e_ob), c.w(u->q_w), c.w(u->q_b), z2, e2, e.noise, e.seed, e.sid, e.off, e.scale, e.z,
                          e.mean, e.log_var, c.B, C, H, W_, c.s);
  });
  return c.rc;
}

int run_decode(const pf_autoenc* u, BlockCtx& c, int H, int W_, const float* z, float scale, float* img) {
  const pf_autoenc_cfg& cfg = u->cfg;
  const int C = u->top_ch;
  // conv_in(post_quant_conv(z / scale)) as one launch, NCHW -> NHWC
  float* h0 = c.palloc((size_t)c.B * H * W_ * C);
  c.launch(PF_K_SMALL, 2.0 * c.B * H * W_ * (9.0 * cfg.z_channels * C + (double)cfg.z_channels * cfg.emb_channels), [&] {
    return launch_ae_front(z, scale, c.w(u->pq_w), c.w(u->pq_b), c.w(u->d_in_w), c.w(u->d_in_b), h0, c.B, cfg.emb_channels, cfg.z_channels, C, H, W_, c.s);
  });
  Tn cur = run_layers(c, u->dec, Tn{h0, C}, H, W_);
  c.head(cur, H, W_, 32, u->d_ng, u->d_nb, u->d_ow, u->d_ob, cfg.out_channels, img, kEps);
  return c.rc;
}

BlockCtx make_ctx(const pf_autoenc* u, int batch) {
  BlockCtx c;
  c.o = u->po; c.B = batch;
  return c;
}

// the latent size (zh, zw) a model can run: the attention's token count, and 32-bit element offsets at the full resolution
bool latent_ok(const pf_autoenc* u, int batch, int zh, int zw) {
  if (!u || batch <= 0 || zh <= 0 || zw <= 0) return false;
  const int l = zh * zw, f = 1 << (u->cfg.n_levels - 1);
  if (l % 64 != 0 || l > 1024) return false;
  return (size_t)batch * zh * f * zw * f * 1024 < ((size_t)1 << 31);
}
bool image_ok(const pf_autoenc* u, int batch, int h, int w) {
  if (!u || h <= 0 || w <= 0) return false;
  const int f = 1 << (u->cfg.n_levels - 1);
  return h % f == 0 && w % f == 0 && latent_ok(u, batch, h / f, w / f);
}
PlanSize enc_plan(const pf_autoenc* u, int batch, int h, int w) {
  return plan_sizes(make_ctx(u, batch), [=](BlockCtx& d) { run_encode(u, d, h, w, EncArgs{}); });
}
PlanSize dec_plan(const pf_autoenc* u, int batch, int zh, int zw) {
  return plan_sizes(make_ctx(u, batch), [=](BlockCtx& d) { run_decode(u, d, zh, zw, nullptr, 1.f, nullptr); });
}

}  // namespace
}  // namespace pf

extern "C" {

int pf_autoenc_create(const pf_autoenc_cfg* cfg, pf_autoenc** out) {
  PF_REQUIRE(cfg && out, "pf_autoenc_create: null argument");
  std::unique_ptr<pf_autoenc> u(new pf_autoenc());
  u->cfg = *cfg;
  const int rc = build(u.get());
  if (rc != PF_OK) return rc;
  *out = u.release();
  return PF_OK;
}
void pf_autoenc_destroy(pf_autoenc* u) { delete u; }

size_t pf_autoenc_weight_bytes(const pf_autoenc* u) { return u ? u->wt.blob_floats * sizeof(float) : 0; }
int pf_autoenc_n_params(const pf_autoenc* u) { return u ? (int)u->wt.params.size() : 0; }
int pf_autoenc_param_info(const pf_autoenc* u, int i, char* key_buf, size_t key_buf_len, int64_t shape[4], int* ndim) {
  PF_REQUIRE(u, "pf_autoenc_param_info: bad arguments");
  return u->wt.param_info("pf_autoenc_param_info", i, key_buf, key_buf_len, shape, ndim);
}
int pf_autoenc_pack_param(pf_autoenc* u, const char* key, const float* src, const int64_t* shape, int ndim, void* host_blob) {
  PF_REQUIRE(u && key, "pf_autoenc_pack_param: null argument");
  // Autoencoder.loss (LPIPSWithDiscriminator, autoencoder.py:46-48) is saved with the model and used in training only: accepted, dropped
  if (strncmp(key, "loss.", 5) == 0) return PF_OK;
  return u->wt.pack_param("pf_autoenc_pack_param", "Autoencoder", key, src, shape, ndim, host_blob);
}
int pf_autoenc_pack_missing(const pf_autoenc* u, char* buf, size_t buf_len) { return u ? u->wt.pack_missing(buf, buf_len) : set_error(PF_EINVAL, "null handle"); }
int pf_autoenc_bind_weights(pf_autoenc* u, const void* dev_blob) {
  PF_REQUIRE(u, "pf_autoenc_bind_weights: null argument");
  return u->wt.bind("pf_autoenc_bind_weights", dev_blob, true);
}

int pf_autoenc_set_precision(pf_autoenc* u, int precision) {
  PF_REQUIRE(u && (precision == PF_PREC_F32 || precision == PF_PREC_BF16X3), "pf_autoenc_set_precision: bad arguments");
  u->po.precision = precision;
  return PF_OK;
}
int pf_autoenc_get_precision(const pf_autoenc* u) { return u ? u->po.precision : -1; }

size_t pf_autoenc_encode_workspace_bytes(const pf_autoenc* u, int batch, int h, int w) { return image_ok(u, batch, h, w) ? enc_plan(u, batch, h, w).bytes() : 0; }
size_t pf_autoenc_decode_workspace_bytes(const pf_autoenc* u, int batch, int zh, int zw) { return latent_ok(u, batch, zh, zw) ? dec_plan(u, batch, zh, zw).bytes() : 0; }
int pf_autoenc_encode_launches(const pf_autoenc* u, int batch, int h, int w) { return image_ok(u, batch, h, w) ? enc_plan(u, batch, h, w).n_launch : 0; }
int pf_autoenc_decode_launches(const pf_autoenc* u, int batch, int zh, int zw) { return latent_ok(u, batch, zh, zw) ? dec_plan(u, batch, zh, zw).n_launch : 0; }
double pf_autoenc_encode_flops(const pf_autoenc* u, int batch, int h, int w) { return image_ok(u, batch, h, w) ? enc_plan(u, batch, h, w).flops : 0.0; }
double pf_autoenc_decode_flops(const pf_autoenc* u, int batch, int zh, int zw) { return latent_ok(u, batch, zh, zw) ? dec_plan(u, batch, zh, zw).flops : 0.0; }

int pf_autoenc_encode(pf_autoenc* u, const float* img, int batch, int h, int w, float scale, const float* noise, uint64_t seed, uint64_t stream_id,
                      uint64_t elem_offset, float* z, float* mean, float* log_var, void* workspace, size_t workspace_bytes, void* stream) {
  PF_REQUIRE(u && img && workspace && batch > 0 && (z || mean || log_var), "pf_autoenc_encode: bad arguments");
  PF_REQUIRE(image_ok(u, batch, h, w), "pf_autoenc_encode: image %dx%d (batch %d): sides must be multiples of %d and the latent hold a multiple of 64, at most 1024, pixels",
             h, w, batch, 1 << (u->cfg.n_levels - 1));
  if (!u->wt.wdev) return set_error(PF_ESTATE, "pf_autoenc_encode: weights not bound (call pf_autoenc_bind_weights)");
  BlockCtx c = make_ctx(u, batch);
  const int rc = c.use_workspace("pf_autoenc_encode", workspace, workspace_bytes, enc_plan(u, batch, h, w), stream, u->wt.wdev);
  if (rc != PF_OK) return rc;
  return run_encode(u, c, h, w, EncArgs{img, scale, noise, seed, stream_id, elem_offset, z, mean, log_var});
}

int pf_autoenc_decode(pf_autoenc* u, const float* z, int batch, int zh, int zw, float scale, float* img, void* workspace, size_t workspace_bytes,
                      void* stream) {
  PF_REQUIRE(u && z && img && workspace && batch > 0 && scale != 0.f, "pf_autoenc_decode: bad arguments");
  PF_REQUIRE(latent_ok(u, batch, zh, zw), "pf_autoenc_decode: latent %dx%d (batch %d) must hold a multiple of 64, at most 1024, pixels", zh, zw, batch);
  if (!u->wt.wdev) return set_error(PF_ESTATE, "pf_autoenc_decode: weights not bound (call pf_autoenc_bind_weights)");
  BlockCtx c = make_ctx(u, batch);
  const int rc = c.use_workspace("pf_autoenc_decode", workspace, workspace_bytes, dec_plan(u, batch, zh, zw), stream, u->wt.wdev);
  if (rc != PF_OK) return rc;
  return run_decode(u, c, zh, zw, z, scale, img);
}

int pf_gaussian_sample(const float* mean, const float* log_var, const float* noise, uint64_t seed, uint64_t stream_id, uint64_t elem_offset,
                       float scale, float* z, size_t n, void* stream) {
  return launch_gaussian_sample(mean, log_var, noise, seed, stream_id, elem_offset, scale, z, n, (hipStream_t)stream);
}

}  // extern "C"
