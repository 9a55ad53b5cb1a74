// unet.hip - host-side plan of the denoiser forward and the pf_unet_* C ABI.
//
// The architecture walk follows the reference constructor (unet.py:30-149) and forward
// (unet.py:171-196); every arithmetic step is a launch of one of the gfx950 kernels in
// conv_mfma.hip / attention.hip / norm_stats.hip / small_kernels.hip.  No device memory is
// allocated here: weights live in ONE caller-owned packed blob, activations in a
// caller-owned workspace carved by two bump allocators (persistent block outputs = the
// U-Net skips; per-layer temporaries that are recycled layer after layer).
#include <algorithm>
#include <memory>
#include <vector>
#include "unet_blocks.h"

namespace pf {

struct Layer {
  int kind;  // 0 conv_in, 1 res, 2 st, 3 down, 4 up
  int cin, cout;
  int hw_h = 0, hw_w = 0;   // res: spatial size of the level (decides whether the Winograd packings exist)
  // offsets (floats) into the packed blob
  ResW r;                   // res
  size_t w1, b1;            // down / up conv
  size_t wfold = 0;         // upsample: parity-folded bf16x3 packing (16 taps)
  // spatial transformer
  size_t norm_g, norm_b, pin_w, pin_b, pout_w, pout_b;
  struct TB { int cross_off; size_t n1g, n1b, n2g, n2b, n3g, n3b, qkv, o1w, o1b, q2, kv2, o2w, o2b, v2raw, o2raw, ff1w, ff1b, ff2w, ff2b; };
  std::vector<TB> tbs;
};
struct Block { std::vector<Layer> layers; };

}  // namespace pf

using namespace pf;

struct pf_unet {
  pf_unet_cfg cfg;
  std::vector<Block> in_blocks, out_blocks;
  Block mid;
  WeightTable wt;
  TimeBias tbias;
  size_t te_w0, te_b0, te_w2, te_b2, out_g, out_b, out_w, out_bias, in_w, in_b;
  // n_cond == 1 cross-attention collapse: to_v / to_out / bias of ALL transformer blocks, contiguous
  size_t cross_v = 0, cross_o = 0, cross_b = 0;
  int cross_total = 0;          // sum of C over transformer blocks
  bool cross_uniform = true;    // every block has the same C -> two grouped launches
  int cross_c = 0;
  int cross_cursor = 0;
  size_t cross_o_cursor = 0;
  PlanOpts po;                  // precision, telemetry word, plan options
  bool profiling = false;
  Profiler prof;   // records of the last profiled forward
  pf_unet() { po.tile_stats = true; }
};

namespace pf {

// every layer with its state_dict prefix, in the reference's module order
template <class U, class F>
static void for_each_layer(U* u, F&& f) {
  for (size_t bi = 0; bi < u->in_blocks.size(); ++bi)
    for (size_t li = 0; li < u->in_blocks[bi].layers.size(); ++li) f("input_blocks." + std::to_string(bi) + "." + std::to_string(li), u->in_blocks[bi].layers[li]);
  for (size_t li = 0; li < u->mid.layers.size(); ++li) f("middle_block." + std::to_string(li), u->mid.layers[li]);
  for (size_t bi = 0; bi < u->out_blocks.size(); ++bi)
    for (size_t li = 0; li < u->out_blocks[bi].layers.size(); ++li) f("output_blocks." + std::to_string(bi) + "." + std::to_string(li), u->out_blocks[bi].layers[li]);
}

static const ResNames kResNames = {"in_layers.0", "in_layers.2", "emb_layers.1", "out_layers.0", "out_layers.3", "skip_connection"};

static void build_res(pf_unet* u, const std::string& p, Layer& L) {
  const int ci = L.cin, co = L.cout;
  const bool wino_ok = L.hw_h >= 32 && L.hw_w >= 32 && L.hw_h % 16 == 0 && L.hw_w % 16 == 0 && co % 64 == 0 && ci % 32 == 0 && ci <= 1024;
  res_rows(u->wt, p, kResNames, ci, co, wino_ok, L.r);
  L.r.emb_off = u->tbias.take(co);
}

static void build_st(pf_unet* u, const std::string& p, Layer& L) {
  const int C = L.cin, dc = u->cfg.d_cond;
  L.norm_g = u->wt.raw(p + ".norm.weight", {C});
  L.norm_b = u->wt.raw(p + ".norm.bias", {C});
  L.pin_w = u->wt.gemm(p + ".proj_in.weight", C, C, 1);
  u->wt.params.back().shape = {C, C, 1, 1};
  L.pin_b = u->wt.raw(p + ".proj_in.bias", {C});
  for (int i = 0; i < u->cfg.tf_layers; ++i) {
    Layer::TB t{};
    const std::string tb = p + ".transformer_blocks." + std::to_string(i);
    // attn1: q,k,v fused into one [C -> 3C] matrix
    t.qkv = u->wt.alloc_gemm(1, C, 3 * C);
    const char* nm[3] = {".attn1.to_q.weight", ".attn1.to_k.weight", ".attn1.to_v.weight"};
    for (int j = 0; j < 3; ++j)
      u->wt.add(tb + nm[j], {C, C}).dests.push_back(Dest{D_GEMM, t.qkv, 1, C, C, (3 * C + 63) / 64 * 64, j * C});
    t.o1w = u->wt.gemm(tb + ".attn1.to_out.0.weight", C, C, 1);
    t.o1b = u->wt.raw(tb + ".attn1.to_out.0.bias", {C});
    // attn2: general (n_cond > 1) form + collapsed (n_cond == 1) raw form of to_v / to_out
    t.q2 = u->wt.gemm(tb + ".attn2.to_q.weight", C, C, 1);
    t.kv2 = u->wt.alloc_gemm(1, dc, 2 * C);
    u->wt.add(tb + ".attn2.to_k.weight", {C, dc}).dests.push_back(Dest{D_GEMM, t.kv2, 1, dc, C, (2 * C + 63) / 64 * 64, 0});
    {
      Param& ps = u->wt.add(tb + ".attn2.to_v.weight", {C, dc});
      ps.dests.push_back(Dest{D_GEMM, t.kv2, 1, dc, C, (2 * C + 63) / 64 * 64, C});
      t.cross_off = u->cross_cursor;
      u->cross_cursor += C;
      t.v2raw = u->cross_v + (size_t)t.cross_off * dc;
      ps.dests.push_back(Dest{D_RAW, t.v2raw, 1, 0, 0, 0, 0});
    }
    t.o2w = u->wt.gemm(tb + ".attn2.to_out.0.weight", C, C, 1);
    t.o2raw = u->cross_o + u->cross_o_cursor;
    u->cross_o_cursor += (size_t)C * C;
    u->wt.params.back().dests.push_back(Dest{D_RAW, t.o2raw, 1, 0, 0, 0, 0});
    t.o2b = u->wt.raw(tb + ".attn2.to_out.0.bias", {C});
    u->wt.params.back().dests.push_back(Dest{D_RAW, u->cross_b + (size_t)t.cross_off, 1, 0, 0, 0, 0});
    t.n1g = u->wt.raw(tb + ".norm1.weight", {C}); t.n1b = u->wt.raw(tb + ".norm1.bias", {C});
    t.n2g = u->wt.raw(tb + ".norm2.weight", {C}); t.n2b = u->wt.raw(tb + ".norm2.bias", {C});
    t.n3g = u->wt.raw(tb + ".norm3.weight", {C}); t.n3b = u->wt.raw(tb + ".norm3.bias", {C});
    t.ff1w = u->wt.alloc_gemm(1, C, 8 * C);
    u->wt.add(tb + ".ff.net.0.proj.weight", {8 * C, C}).dests.push_back(Dest{D_GEGLU_W, t.ff1w, 1, C, 8 * C, 8 * C, 0});
    t.ff1b = u->wt.alloc((size_t)8 * C);
    u->wt.add(tb + ".ff.net.0.proj.bias", {8 * C}).dests.push_back(Dest{D_GEGLU_B, t.ff1b, 1, 0, 8 * C, 8 * C, 0});
    t.ff2w = u->wt.gemm(tb + ".ff.net.2.weight", C, 4 * C, 1);
    t.ff2b = u->wt.raw(tb + ".ff.net.2.bias", {C});
    L.tbs.push_back(t);
  }
  L.pout_w = u->wt.gemm(p + ".proj_out.weight", C, C, 1);
  u->wt.params.back().shape = {C, C, 1, 1};
  L.pout_b = u->wt.raw(p + ".proj_out.bias", {C});
}

static void build_layer(pf_unet* u, const std::string& p, Layer& L) {
  switch (L.kind) {
    case 0:
      u->in_w = u->wt.raw(p + ".weight", {L.cout, L.cin, 3, 3});
      u->in_b = u->wt.raw(p + ".bias", {L.cout});
      break;
    case 1: build_res(u, p, L); break;
    case 2: build_st(u, p, L); break;
    case 3:
      L.w1 = u->wt.gemm(p + ".op.weight", L.cout, L.cin, 9);
      L.b1 = u->wt.raw(p + ".op.bias", {L.cout});
      break;
    case 4:
      L.w1 = u->wt.gemm(p + ".conv.weight", L.cout, L.cin, 9);
      if (L.cin % 8 == 0) {   // bf16x3 mode runs the layer as four 2x2 convs on the source grid
        L.wfold = u->wt.alloc(gemm_floats(16, L.cin, L.cout));
        u->wt.params.back().dests.push_back(Dest{D_UPFOLD, L.wfold, 16, L.cin, L.cout, (L.cout + 63) / 64 * 64, 0});
      }
      L.b1 = u->wt.raw(p + ".conv.bias", {L.cout});
      break;
  }
}

static bool in_list(const int32_t* v, int n, int x) {
  for (int i = 0; i < n; ++i) if (v[i] == x) return true;
  return false;
}

static int build(pf_unet* u) {
  const pf_unet_cfg& c = u->cfg;
  PF_REQUIRE(c.n_levels >= 1 && c.n_levels <= 8 && c.n_attention_levels >= 0 && c.n_attention_levels <= 8, "unet: bad level counts");
  PF_REQUIRE(c.channels > 0 && c.channels % 32 == 0, "unet: channels must be a multiple of 32 (GroupNorm32), got %d", c.channels);
  PF_REQUIRE(c.in_channels >= 1 && c.out_channels >= 1 && c.out_channels <= 4, "unet: out_channels must be 1..4");
  PF_REQUIRE(c.n_heads > 0 && c.tf_layers >= 1 && c.d_cond > 0 && c.d_cond % 4 == 0, "unet: bad attention config");
  PF_REQUIRE(c.img_h % (1 << (c.n_levels - 1)) == 0 && c.img_w % (1 << (c.n_levels - 1)) == 0, "unet: image size must be divisible by 2^(levels-1)");
  const int d_t = u->tbias.d_t = c.channels * 4;
  u->te_w0 = u->wt.raw("time_embed.0.weight", {d_t, c.channels});
  u->te_b0 = u->wt.raw("time_embed.0.bias", {d_t});
  u->te_w2 = u->wt.raw("time_embed.2.weight", {d_t, d_t});
  u->te_b2 = u->wt.raw("time_embed.2.bias", {d_t});

  int ch = c.channels;
  std::vector<int> stack;
  std::vector<int> widths;
  for (int i = 0; i < c.n_levels; ++i) widths.push_back(c.channels * c.channel_multipliers[i]);
  {
    Block b; Layer L{}; L.kind = 0; L.cin = c.in_channels; L.cout = ch; b.layers.push_back(L);
    u->in_blocks.push_back(b); stack.push_back(ch);
  }
  for (int lvl = 0; lvl < c.n_levels; ++lvl) {
    const bool att = in_list(c.attention_levels, c.n_attention_levels, lvl);
    for (int r = 0; r < c.n_res_blocks; ++r) {
      Block b; Layer L{}; L.kind = 1; L.cin = ch; L.cout = widths[lvl]; L.hw_h = c.img_h >> lvl; L.hw_w = c.img_w >> lvl; b.layers.push_back(L);
      ch = widths[lvl];
      if (att) {
        PF_REQUIRE(ch % c.n_heads == 0 && (ch / c.n_heads == 32 || ch / c.n_heads == 64), "unet: d_head %d unsupported (32 or 64)", ch / c.n_heads);
        Layer S{}; S.kind = 2; S.cin = S.cout = ch; b.layers.push_back(S);
      }
      u->in_blocks.push_back(b); stack.push_back(ch);
    }
    if (lvl != c.n_levels - 1) {
      Block b; Layer L{}; L.kind = 3; L.cin = L.cout = ch; b.layers.push_back(L);
      u->in_blocks.push_back(b); stack.push_back(ch);
    }
  }
  {
    PF_REQUIRE(ch % c.n_heads == 0 && (ch / c.n_heads == 32 || ch / c.n_heads == 64), "unet: d_head %d unsupported (32 or 64)", ch / c.n_heads);
    Layer a{}; a.kind = 1; a.cin = a.cout = ch;
    Layer s{}; s.kind = 2; s.cin = s.cout = ch;
    Layer d{}; d.kind = 1; d.cin = d.cout = ch;
    u->mid.layers = {a, s, d};
  }
  for (int lvl = c.n_levels - 1; lvl >= 0; --lvl) {
    const bool att = in_list(c.attention_levels, c.n_attention_levels, lvl);
    for (int j = 0; j <= c.n_res_blocks; ++j) {
      const int sk = stack.back(); stack.pop_back();
      Block b; Layer L{}; L.kind = 1; L.cin = ch + sk; L.cout = widths[lvl]; L.hw_h = c.img_h >> lvl; L.hw_w = c.img_w >> lvl; b.layers.push_back(L);
      ch = widths[lvl];
      if (att) { Layer S{}; S.kind = 2; S.cin = S.cout = ch; b.layers.push_back(S); }
      if (lvl != 0 && j == c.n_res_blocks) { Layer U{}; U.kind = 4; U.cin = U.cout = ch; b.layers.push_back(U); }
      u->out_blocks.push_back(b);
    }
  }

  // n_cond == 1 cross-attention collapse: one contiguous region for all blocks' to_v / to_out / bias
  {
    size_t o_floats = 0;
    for_each_layer(u, [&](const std::string&, const Layer& L) {
      if (L.kind != 2) return;
      for (int i = 0; i < c.tf_layers; ++i) {
        if (u->cross_c == 0) u->cross_c = L.cin;
        if (L.cin != u->cross_c) u->cross_uniform = false;
        u->cross_total += L.cin;
        o_floats += (size_t)L.cin * L.cin;
      }
    });
    u->cross_v = u->wt.alloc((size_t)u->cross_total * c.d_cond);
    u->cross_o = u->wt.alloc(o_floats);
    u->cross_b = u->wt.alloc((size_t)u->cross_total);
  }

  // parameter table in the reference key order
  for_each_layer(u, [&](const std::string& p, Layer& L) { build_layer(u, p, L); });
  u->out_g = u->wt.raw("out.0.weight", {ch});
  u->out_b = u->wt.raw("out.0.bias", {ch});
  u->out_w = u->wt.alloc((size_t)c.out_channels * 9 * ch);
  u->wt.add("out.2.weight", {c.out_channels, ch, 3, 3}).dests.push_back(Dest{D_CONVOUT, u->out_w, 9, ch, c.out_channels, 0, 0});
  u->out_bias = u->wt.raw("out.2.bias", {c.out_channels});

  // the emb_layers rows come after everything else
  u->tbias.alloc(u->wt);
  for_each_layer(u, [&](const std::string& p, Layer& L) {
    if (L.kind == 1) u->tbias.rows(u->wt, p + "." + kResNames.emb, L.cout, L.r.emb_off);
  });
  return PF_OK;
}

// ---- forward ----
struct Ctx : BlockCtx {
  pf_unet* u = nullptr;
  int n_cond = 0;
  // hoisted step-invariant prefix (pf_unet_prepared): supplied parts are not recomputed; dry runs only need to know WHETHER they are
  bool has_time = false, has_cross = false;
  const float* prep_time = nullptr; int prep_time_rows = 0; const float* prep_cross = nullptr;
  // classifier-free guidance with a shared prefix (pf_unet_forward_cfg / _cfgn): while `shared` the plan runs on the first Bfull / groups samples only
  int groups = 0;   // 0: plain forward; 2 / 3: that many stacked evaluations of one x
  bool shared = false; int Bfull = 0;

  void lnp(const float* x, int rows, int c, size_t gamma, size_t beta, float* planes) {   // LayerNorm -> hi/lo planes
    launch(PF_K_LNSTAT, 0.0, [&] { return launch_ln_planes(x, rows, c, 1e-5f, w(gamma), w(beta), planes, s); });
  }
  void ln(const float* x, int rows, int c, float* mu, float* rs) {
    launch(PF_K_LNSTAT, 0.0, [&] { return launch_ln_stats(x, rows, c, 1e-5f, mu, rs, s); });
  }
};

static int device_copy(float* dst, const float* src, size_t nfloats, hipStream_t s) {
  if (hipMemcpyAsync(dst, src, nfloats * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
    return set_error(PF_EHIP, "pf_unet_forward_cfg: device copy failed");
  return PF_OK;
}

// The fused feed-forward launch (mlp_fused_bf3.hip) gives every 64-row tile to one four-wave workgroup that streams all 3 MB of ff
// weights and occupies a whole CU (152 KB of LDS), so it runs in rounds of 256 tiles: measured 95 us per round against 113 us per
// 16384 rows for the three launches it replaces (B = 16, L = 1024).  It is used when the last round is at least 85 % full
// (B = 16 and B = 32 at the 32x32 level; never at the 16x16 level below B = 55).  pf_unet_set_option(PF_OPT_MLP_FUSED) forces it off / on.
static bool mlp_fused_wanted(int C, int hw, int M, int force) {
  if (C != 256 || hw % 64 != 0) return false;
  if (force != PF_OPT_AUTO) return force != PF_OPT_OFF;
  const int cus = num_cus(), tiles = M / 64, rounds = (tiles + cus - 1) / cus;
  return tiles * 100 >= 85 * cus * rounds;
}

static Tn run_st(Ctx& c, const Layer& L, const Tn& xin, int H, int W_, const float* cond, const float* cross_all) {
  const int B = c.B, hw = H * W_, C = L.cin, M = B * hw, nh = c.u->cfg.n_heads, dh = C / nh, dc = c.u->cfg.d_cond;
  const float* x = xin.d;
  float* out = c.palloc((size_t)M * C);
  c.treset();
  float* sc = c.talloc((size_t)B * C); float* sh = c.talloc((size_t)B * C);
  float* ta = c.talloc((size_t)M * C); float* tbuf = c.talloc((size_t)M * C); float* tc = c.talloc((size_t)M * C);
  float* mu = c.talloc(M); float* rs = c.talloc(M);
  float* qkv = c.talloc((size_t)M * 3 * C);
  float* att = c.talloc((size_t)M * C);
  float* ff = c.talloc((size_t)M * 4 * C);
  float* kv = nullptr;
  if (c.n_cond > 1) kv = c.talloc((size_t)B * c.n_cond * 2 * C);
  const Ctx::GnRef gin = c.gn(xin, Tn{}, hw, 32, 1e-6f, L.norm_g, L.norm_b, sc, sh, true);
  // bf16x3 mode, d_head 64, L % 128 == 0: every linear layer of the block runs on pre-split hi/lo planes (see the loop below)
  const bool planes_ok = c.o.precision == PF_PREC_BF16X3 && dh == 64 && hw % 128 == 0 && C % 32 == 0 && C <= 1024;
  {
    pf_conv_args a = conv_base(x, C, nullptr, 0, B, 1, hw, 1, c.w(L.pin_w), C, ta);
    a.prologue = 2; a.sc = sc; a.sh = sh; a.bias = c.w(L.pin_b);
    c.gn_attach(a, gin);
    c.conv(a);
  }
  float* t0 = ta; float* t1 = tbuf; float* t2 = tc;
  bool last_planes = false;
  for (size_t i = 0; i < L.tbs.size(); ++i) {
    const Layer::TB& t = L.tbs[i];
    // x = attn1(LN1(x)) + x
    // bf16x3 mode, d_head 64, L % 128 == 0: every linear layer of the block runs as a planes GEMM (both operands stream
    // global->LDS): LayerNorm is applied once per row into hi/lo planes instead of once per column tile in a GEMM prologue,
    // the projection writes pre-split q/k/v^T planes and attention runs on the bf16 pipe
    const bool planes = planes_ok;
    if (planes) {
      c.lnp(t0, M, C, t.n1g, t.n1b, att);   // `att` is free until attention writes it
      pf_conv_args a = conv_base(att, C, nullptr, 0, B, 1, hw, 1, c.w(t.qkv), 3 * C, qkv);
      a.a_planes = 1;
      a.qkv_planes = c.dry ? (void*)1 : (void*)qkv;   // same bytes as the fp32 [M][3C] buffer
      c.conv(a);
    } else {
      c.ln(t0, M, C, mu, rs);
      pf_conv_args a = conv_base(t0, C, nullptr, 0, B, 1, hw, 1, c.w(t.qkv), 3 * C, qkv);
      a.prologue = 3; a.sc = c.w(t.n1g); a.sh = c.w(t.n1b); a.mean = mu; a.rstd = rs;
      c.conv(a);
    }
    // small batches (few query tiles, many key tiles each): key slices across workgroups + a merging launch, partial results in the temp region
    int att_ns = 1;
    const size_t att_sf = planes ? attention_bf3_split_floats(B, nh, hw, &att_ns) : 0;
    float* att_scratch = att_sf ? c.talloc(att_sf) : nullptr;
    // PF_OPT_ATTN_WIDE forced on holds where the 256-query form exists (L % 256 == 0); elsewhere the level runs the 128-query form
    const int att_form = (c.o.opt[PF_OPT_ATTN_WIDE] == PF_OPT_ON && hw % 256 != 0) ? PF_OPT_OFF : c.o.opt[PF_OPT_ATTN_WIDE];
    const bool merge = att_sf && att_form != PF_OPT_ON;   // (a second, merging launch)
    c.launch(PF_K_ATTN, 4.0 * B * nh * (double)hw * hw * dh, [&] {
      return planes ? launch_attention_bf3(qkv, nullptr, C, att, B, nh, hw, att_form, c.s, att_scratch, att_sf)   // att as hi/lo planes for the to_out GEMM
                    : launch_attention(qkv, 3 * C, qkv + C, 3 * C, qkv + 2 * C, 3 * C, att, C, B, nh, dh, hw, hw, c.s);
    }, merge ? 2 : 1);
    last_planes = planes && (i + 1 == L.tbs.size());
    const bool fuse_mlp = planes && mlp_fused_wanted(C, hw, M, c.o.opt[PF_OPT_MLP_FUSED]) && !c.o.amax_slot;
    {
      pf_conv_args a = conv_base(att, C, nullptr, 0, B, 1, hw, 1, c.w(t.o1w), C, t1);
      a.bias = c.w(t.o1b); a.res = t0; a.ld_res = C; a.a_planes = planes ? 1 : 0;
      if (c.n_cond == 1) {  // x = attn2(LN2(x), c) + x collapses to a per-sample bias (softmax over one key == 1)
        a.sbias = c.dry ? nullptr : cross_all + t.cross_off;
        a.ld_sbias = c.u->cross_total;
      }
      c.conv(a);
    }
    if (c.n_cond > 1) {
      c.ln(t1, M, C, mu, rs);
      float* q2 = qkv;  // reuse: [M][C]
      {
        pf_conv_args a = conv_base(t1, C, nullptr, 0, B, 1, hw, 1, c.w(t.q2), C, q2);
        a.prologue = 3; a.sc = c.w(t.n2g); a.sh = c.w(t.n2b); a.mean = mu; a.rstd = rs;
        c.conv(a);
      }
      {
        pf_conv_args a = conv_base(cond, dc, nullptr, 0, B, 1, c.n_cond, 1, c.w(t.kv2), 2 * C, kv);
        c.conv(a);
      }
      c.launch(PF_K_ATTN, 4.0 * B * nh * (double)hw * c.n_cond * dh,
               [&] { return launch_attention(q2, C, kv, 2 * C, kv + C, 2 * C, att, C, B, nh, dh, hw, c.n_cond, c.s); });
      {
        pf_conv_args a = conv_base(att, C, nullptr, 0, B, 1, hw, 1, c.w(t.o2w), C, t2);
        a.bias = c.w(t.o2b); a.res = t1; a.ld_res = C;
        c.conv(a);
      }
      std::swap(t1, t2);
    }
    // x = ff(LN3(x)) + x
    if (fuse_mlp) {
      // one launch: LayerNorm, GeGLU projection, output projection and residual per 64-row tile, hidden tensor kept on chip
      if (last_planes) {
        // the block's proj_out rides on the same launch: ff output + residual stay in LDS as its A operand, the result lands in `out`
        // together with the 64-row-tile statistics the next GroupNorm reads
        const int nt = hw / 64;
        float* sb = c.palloc((size_t)B * nt * C * 2);
        c.launch(PF_K_GEMM, 2.0 * M * ((double)C * 8 * C + 4.0 * C * C + (double)C * C), [&] {
          return launch_mlp_fused(t1, B, hw, c.w(t.n3g), c.w(t.n3b), 1e-5f, c.w_split(t.ff1w, 1, C, 8 * C), c.w(t.ff1b), c.w_split(t.ff2w, 1, 4 * C, C),
                                  c.w(t.ff2b), out, nullptr, c.s, c.w_split(L.pout_w, 1, C, C), c.w(L.pout_b), x, sb);
        });
        Tn ot;
        ot.d = out; ot.c = C; ot.st = sb; ot.nt = nt;
        return ot;
      }
      c.launch(PF_K_GEMM, 2.0 * M * ((double)C * 8 * C + 4.0 * C * C), [&] {
        return launch_mlp_fused(t1, B, hw, c.w(t.n3g), c.w(t.n3b), 1e-5f, c.w_split(t.ff1w, 1, C, 8 * C), c.w(t.ff1b), c.w_split(t.ff2w, 1, 4 * C, C),
                                c.w(t.ff2b), t2, nullptr, c.s);
      });
      std::swap(t0, t2);
      continue;
    }
    if (planes) {
      c.lnp(t1, M, C, t.n3g, t.n3b, att);   // `att` has been consumed by to_out
      pf_conv_args a = conv_base(att, C, nullptr, 0, B, 1, hw, 1, c.w(t.ff1w), 8 * C, ff);
      a.a_planes = 1; a.bias = c.w(t.ff1b); a.geglu = 1; a.ld_out = 4 * C;
      a.out_planes = c.dry ? (void*)1 : (void*)ff;   // GeGLU product straight into hi/lo planes for the ff2 GEMM
      c.conv(a);
    } else {
      c.ln(t1, M, C, mu, rs);
      pf_conv_args a = conv_base(t1, C, nullptr, 0, B, 1, hw, 1, c.w(t.ff1w), 8 * C, ff);
      a.prologue = 3; a.sc = c.w(t.n3g); a.sh = c.w(t.n3b); a.mean = mu; a.rstd = rs; a.bias = c.w(t.ff1b);
      a.geglu = 1; a.ld_out = 4 * C;
      c.conv(a);
    }
    {
      pf_conv_args a = conv_base(ff, 4 * C, nullptr, 0, B, 1, hw, 1, c.w(t.ff2w), C, t2);
      a.bias = c.w(t.ff2b); a.res = t1; a.ld_res = C; a.a_planes = planes ? 1 : 0;
      if (last_planes) a.out_planes = c.dry ? (void*)1 : (void*)t2;   // only proj_out reads it: hand it over as planes
      c.conv(a);
    }
    std::swap(t0, t2);
  }
  Tn ot;
  {
    pf_conv_args a = conv_base(t0, C, nullptr, 0, B, 1, hw, 1, c.w(L.pout_w), C, out);
    a.bias = c.w(L.pout_b); a.res = x; a.ld_res = C; a.a_planes = last_planes ? 1 : 0;
    c.conv(a, &ot, true);
  }
  return ot;
}

// n_cond == 1: cross[b] = to_out(to_v(cond[b])) + bias of EVERY transformer block (softmax over one key == 1, unet_attention.py:186-212):
// two grouped mat-vec launches (one per block when the blocks differ in width).  Shared by the forward plan and pf_unet_prepare_cond.
static void cross_bias_launches(pf_unet* u, Ctx& c, const float* cond, int B, float* cross, float* vtmp) {
  const int T = u->cross_total, dc = u->cfg.d_cond;
  c.launch(PF_K_SMALL, 0, [&] { return launch_matvec(cond, dc, c.w(u->cross_v), nullptr, vtmp, T, B, T, dc, c.s); });
  if (u->cross_uniform) {
    c.launch(PF_K_SMALL, 0, [&] { return launch_matvec(vtmp, T, c.w(u->cross_o), c.w(u->cross_b), cross, T, B, T, u->cross_c, c.s, u->cross_c, u->cross_c); });
    return;
  }
  for_each_layer(u, [&](const std::string&, const Layer& L) {
    if (L.kind != 2) return;
    for (const Layer::TB& tb : L.tbs) {
      c.launch(PF_K_SMALL, 0, [&] { return launch_matvec(vtmp + tb.cross_off, T, c.w(tb.o2raw), c.w(tb.o2b), cross + tb.cross_off, T, B, L.cin, L.cin, c.s); });
    }
  });
}

static int run(pf_unet* u, Ctx& c, const float* x, const int64_t* t, const float* cond, float* eps) {
  const pf_unet_cfg& cfg = u->cfg;
  const int B = c.B;
  int H = cfg.img_h, W_ = cfg.img_w;
  // time embedding and every ResBlock's additive time bias
  // (the workspace layout does not depend on what the caller prepared: the small buffers are carved either way)
  const TimeBias& tbs = u->tbias;
  float* tsilu = c.palloc((size_t)B * tbs.d_t);
  float* tb = c.palloc((size_t)B * tbs.sum);
  c.tb = tb; c.tb_ld = tbs.sum;
  if (c.has_time) {   // hoisted: row t[b] of the caller's table (pf_unet_prepare_time) instead of two launches per forward
    c.tb = c.prep_time; c.tb_rows = t; c.tb_nrows = c.prep_time_rows;
  } else {
    c.launch(PF_K_SMALL, 0, [&] { return launch_time_embed(t, c.w(u->te_w0), c.w(u->te_b0), c.w(u->te_w2), c.w(u->te_b2), tsilu, B, cfg.channels, tbs.d_t, c.s); });
    c.launch(PF_K_SMALL, 0, [&] { return launch_matvec(tsilu, tbs.d_t, c.w(tbs.w), c.w(tbs.b), tb, tbs.sum, B, tbs.sum, tbs.d_t, c.s); });
  }
  const float* cross_all = nullptr;  // [B][cross_total]: to_out(to_v(c)) + bias of every transformer block
  if (c.n_cond == 1 && u->cross_total > 0) {
    const int T = u->cross_total;
    float* cross_ws = c.palloc((size_t)B * T);
    float* vtmp = c.palloc((size_t)B * T);
    cross_all = cross_ws;
    if (c.has_cross) cross_all = c.prep_cross;   // hoisted (pf_unet_prepare_cond)
    else cross_bias_launches(u, c, cond, B, cross_ws, vtmp);
  }

  std::vector<Tn> skips;
  Tn cur;
  // Classifier-free guidance with a shared prefix: until the first SpatialTransformer the plan runs on the first group of the batch only
  // (the groups - two halves, or the three thirds of dual guidance - are identical there: the condition has not entered yet); right before it
  // the running tensor and its statistics are copied once per group and the plan continues on the whole batch.  Skip tensors produced in the
  // shared phase keep their one-group size and are read with the sample index modulo the group (Tn::bmod -> pf_conv_args.x1_bmod).
  const int G = c.groups;
  if (G) { c.Bfull = c.B; c.B = c.B / G; c.shared = true; }
  auto dup_rows = [&](const float* src, size_t floats_per_group) -> const float* {
    float* dst = c.palloc(G * floats_per_group);
    for (int h = 0; h < G; ++h)
      c.launch(PF_K_SMALL, 0, [&] { return device_copy(dst + h * floats_per_group, src, floats_per_group, c.s); });
    return dst;
  };
  auto leave_shared_phase = [&](Tn& a0, int h, int w_) {
    if (!c.shared) return;
    const int Bh = c.B;
    a0.d = dup_rows(a0.d, (size_t)Bh * h * w_ * a0.c);
    if (a0.nt > 0) a0.st = dup_rows(a0.st, (size_t)Bh * a0.nt * a0.c * 2);   // (nt, not st: a dry run carries no pointers)
    a0.bmod = 0;
    c.B = c.Bfull; c.shared = false;
  };
  auto run_layers = [&](const Block& b, Tn in0, Tn in1) {
    Tn a0 = in0, a1 = in1;
    for (const Layer& L : b.layers) {
      Tn o;
      if (L.kind == 2) leave_shared_phase(a0, H, W_);
      switch (L.kind) {
        case 0: o = c.stem(x, u->in_w, u->in_b, L.cin, L.cout, H, W_); break;
        case 1: o = c.res_block(L.r, a0, a1, H, W_, L.cout); break;
        case 2: o = run_st(c, L, a0, H, W_, cond, cross_all); break;
        case 3:
          o = c.downsample(a0, H, W_, L.w1, L.b1, L.cout);
          H /= 2; W_ /= 2;
          break;
        case 4:
          if (c.o.precision == PF_PREC_BF16X3 && L.wfold && L.cin % 32 == 0) {
            o = c.upsample_fold(a0, H, W_, L.wfold, L.b1, L.cout);
          } else {   // nearest-neighbour upsampling inside the conv's gather
            float* od = c.palloc((size_t)c.B * (H * 2) * (W_ * 2) * L.cout);
            pf_conv_args a = conv_base(a0.d, a0.c, nullptr, 0, c.B, H, W_, 3, c.w(L.w1), L.cout, od);
            a.ups = 1; a.bias = c.w(L.b1);
            c.conv(a, &o, true);
          }
          H *= 2; W_ *= 2;
          break;
      }
      if (c.dry) o.c = L.cout;
      if (c.shared) o.bmod = c.B;
      a0 = o; a1 = Tn{};
    }
    cur = a0;
  };

  for (const Block& b : u->in_blocks) {
    run_layers(b, cur, Tn{});
    skips.push_back(cur);
  }
  run_layers(u->mid, cur, Tn{});
  for (const Block& b : u->out_blocks) {
    const Tn sk = skips.back();
    skips.pop_back();
    run_layers(b, cur, sk);  // channel order [x, skip] (unet.py:192)
  }
  // out: GN + SiLU + conv3x3 -> NCHW
  c.head(cur, H, W_, 32, u->out_g, u->out_b, u->out_w, u->out_bias, cfg.out_channels, eps);
  if (c.shared) {   // a UNet without any transformer block never looked at the condition: every group of eps is the same image
    const size_t n = (size_t)c.B * cfg.out_channels * H * W_;
    for (int h = 1; h < G; ++h)
      c.launch(PF_K_SMALL, 0, [&] { return device_copy(eps + h * n, eps, n, c.s); });
    c.B = c.Bfull; c.shared = false;
  }
  return c.rc;
}

static Ctx make_ctx(const pf_unet* u, int batch, int n_cond, int groups, bool has_time = false, bool has_cross = false) {
  Ctx c;
  c.u = const_cast<pf_unet*>(u); c.o = u->po; c.B = batch; c.n_cond = n_cond; c.groups = groups; c.has_time = has_time; c.has_cross = has_cross;
  return c;
}
// a stacked guidance batch the shared-prefix plan accepts: two or three groups of the same size
static bool groups_ok(int batch_total, int groups) { return (groups == 2 || groups == 3) && batch_total > 0 && batch_total % groups == 0; }
static PlanSize unet_plan(const Ctx& c) { return plan_sizes(c, [](Ctx& d) { run(d.u, d, nullptr, nullptr, nullptr, nullptr); }); }

}  // namespace pf

extern "C" {

int pf_unet_create(const pf_unet_cfg* cfg, pf_unet** out) {
  PF_REQUIRE(cfg && out, "pf_unet_create: null argument");
  std::unique_ptr<pf_unet> u(new pf_unet());
  u->cfg = *cfg;
  int rc = build(u.get());
  if (rc != PF_OK) return rc;
  *out = u.release();
  return PF_OK;
}

void pf_unet_destroy(pf_unet* u) { delete u; }

size_t pf_unet_weight_bytes(const pf_unet* u) { return u ? u->wt.blob_floats * sizeof(float) : 0; }
int pf_unet_n_params(const pf_unet* u) { return u ? (int)u->wt.params.size() : 0; }

int pf_unet_param_info(const pf_unet* u, int i, char* key_buf, size_t key_buf_len, int64_t shape[4], int* ndim) {
  PF_REQUIRE(u, "pf_unet_param_info: bad arguments");
  return u->wt.param_info("pf_unet_param_info", i, key_buf, key_buf_len, shape, ndim);
}
int pf_unet_pack_param(pf_unet* u, const char* key, const float* src, const int64_t* shape, int ndim, void* host_blob) {
  PF_REQUIRE(u, "pf_unet_pack_param: null argument");
  return u->wt.pack_param("pf_unet_pack_param", "UNet", key, src, shape, ndim, host_blob);
}
int pf_unet_pack_missing(const pf_unet* u, char* buf, size_t buf_len) { return u ? u->wt.pack_missing(buf, buf_len) : set_error(PF_EINVAL, "null handle"); }
int pf_unet_bind_weights(pf_unet* u, const void* dev_blob) {
  PF_REQUIRE(u, "pf_unet_bind_weights: null argument");
  return u->wt.bind("pf_unet_bind_weights", dev_blob, true);
}

size_t pf_unet_workspace_bytes(const pf_unet* u, int batch, int n_cond) {
  return (u && batch > 0 && n_cond > 0) ? unet_plan(make_ctx(u, batch, n_cond, 0)).bytes() : 0;
}
int pf_unet_n_launches(const pf_unet* u, int batch, int n_cond) {
  return (u && batch > 0 && n_cond > 0) ? unet_plan(make_ctx(u, batch, n_cond, 0)).n_launch : 0;
}

int pf_unet_forward(pf_unet* u, const float* x, const int64_t* t, const float* cond, int batch, int n_cond, float* eps,
                    void* workspace, size_t workspace_bytes, void* stream) {
  return pf_unet_forward_prepared(u, x, t, cond, batch, n_cond, nullptr, eps, workspace, workspace_bytes, stream);
}

static int forward_impl(pf_unet* u, const float* x, const int64_t* t, const float* cond, int batch, int n_cond, const pf_unet_prepared* prep,
                        float* eps, void* workspace, size_t workspace_bytes, void* stream, int groups) {
  PF_REQUIRE(u && x && t && cond && eps && workspace, "pf_unet_forward: null argument");
  PF_REQUIRE(!prep || !prep->time_table || prep->n_time_rows > 0, "pf_unet_forward: time table without rows");
  PF_REQUIRE(!prep || !prep->cross_bias || n_cond == 1, "pf_unet_forward: the collapsed cross-attention bias exists only for n_cond == 1");
  PF_REQUIRE(batch > 0 && n_cond > 0, "pf_unet_forward: batch and n_cond must be positive");
  PF_REQUIRE(!groups || groups_ok(batch, groups), "pf_unet_forward_cfg: the batch is 2 or 3 guidance groups of one size (got %d rows, %d groups)", batch, groups);
  if (!u->wt.wdev) return set_error(PF_ESTATE, "pf_unet_forward: weights not bound (call pf_unet_bind_weights)");
  PF_REQUIRE(n_cond == 1 || u->cfg.d_cond % 32 == 0, "pf_unet_forward: n_cond > 1 needs d_cond %% 32 == 0");
  Ctx c = make_ctx(u, batch, n_cond, groups);
  const int rc = c.use_workspace("pf_unet_forward", workspace, workspace_bytes, unet_plan(c), stream, u->wt.wdev);   // (the layout does not depend on `prep`)
  if (rc != PF_OK) return rc;
  if (prep && prep->time_table) { c.has_time = true; c.prep_time = prep->time_table; c.prep_time_rows = prep->n_time_rows; }
  if (prep && prep->cross_bias && u->cross_total > 0) { c.has_cross = true; c.prep_cross = prep->cross_bias; }
  if (u->profiling) { u->prof.rec.clear(); c.prof = &u->prof; }
  return run(u, c, x, t, cond, eps);
}

int pf_unet_forward_prepared(pf_unet* u, const float* x, const int64_t* t, const float* cond, int batch, int n_cond, const pf_unet_prepared* prep,
                             float* eps, void* workspace, size_t workspace_bytes, void* stream) {
  return forward_impl(u, x, t, cond, batch, n_cond, prep, eps, workspace, workspace_bytes, stream, 0);
}

int pf_unet_forward_cfg(pf_unet* u, const float* x, const int64_t* t, const float* cond, int batch2, int n_cond, const pf_unet_prepared* prep,
                        float* eps2, void* workspace, size_t workspace_bytes, void* stream) {
  return pf_unet_forward_cfgn(u, x, t, cond, batch2, 2, n_cond, prep, eps2, workspace, workspace_bytes, stream);
}
size_t pf_unet_workspace_bytes_cfg(const pf_unet* u, int batch2, int n_cond) { return pf_unet_workspace_bytes_cfgn(u, batch2, 2, n_cond); }
int pf_unet_n_launches_cfg(const pf_unet* u, int batch2, int n_cond, int has_time, int has_cross) {
  return pf_unet_n_launches_cfgn(u, batch2, 2, n_cond, has_time, has_cross);
}

int pf_unet_forward_cfgn(pf_unet* u, const float* x, const int64_t* t, const float* cond, int batch_total, int groups, int n_cond,
                         const pf_unet_prepared* prep, float* eps, void* workspace, size_t workspace_bytes, void* stream) {
  PF_REQUIRE(groups_ok(batch_total, groups), "pf_unet_forward_cfgn: the batch is 2 or 3 guidance groups of one size (got %d rows, %d groups)", batch_total, groups);
  return forward_impl(u, x, t, cond, batch_total, n_cond, prep, eps, workspace, workspace_bytes, stream, groups);
}
size_t pf_unet_workspace_bytes_cfgn(const pf_unet* u, int batch_total, int groups, int n_cond) {
  return (u && groups_ok(batch_total, groups) && n_cond > 0) ? unet_plan(make_ctx(u, batch_total, n_cond, groups)).bytes() : 0;
}
int pf_unet_n_launches_cfgn(const pf_unet* u, int batch_total, int groups, int n_cond, int has_time, int has_cross) {
  if (!u || !groups_ok(batch_total, groups) || n_cond <= 0) return 0;
  return unet_plan(make_ctx(u, batch_total, n_cond, groups, has_time != 0, has_cross != 0 && n_cond == 1)).n_launch;
}

int pf_unet_time_bias_width(const pf_unet* u) { return u ? u->tbias.sum : 0; }
int pf_unet_cross_bias_width(const pf_unet* u) { return u ? u->cross_total : 0; }

int pf_unet_prepare_time(pf_unet* u, int n_rows, float* table, void* scratch, size_t scratch_bytes, void* stream) {
  PF_REQUIRE(u && table && scratch && n_rows > 0, "pf_unet_prepare_time: bad arguments");
  if (!u->wt.wdev) return set_error(PF_ESTATE, "pf_unet_prepare_time: weights not bound (call pf_unet_bind_weights)");
  PF_REQUIRE(scratch_bytes >= (size_t)n_rows * u->tbias.d_t * sizeof(float), "pf_unet_prepare_time: scratch too small (%zu < %zu)", scratch_bytes,
             (size_t)n_rows * u->tbias.d_t * sizeof(float));
  const float* W = u->wt.wdev;
  float* tsilu = static_cast<float*>(scratch);
  // the same two launches forward issues per call (row r <- time-step value r): bit-identical to the unprepared path
  int rc = launch_time_embed(nullptr, W + u->te_w0, W + u->te_b0, W + u->te_w2, W + u->te_b2, tsilu, n_rows, u->cfg.channels, u->tbias.d_t, (hipStream_t)stream);
  if (rc != PF_OK) return rc;
  return launch_matvec(tsilu, u->tbias.d_t, W + u->tbias.w, W + u->tbias.b, table, u->tbias.sum, n_rows, u->tbias.sum, u->tbias.d_t, (hipStream_t)stream);
}

int pf_unet_prepare_cond(pf_unet* u, const float* cond, int batch, float* cross, void* scratch, size_t scratch_bytes, void* stream) {
  PF_REQUIRE(u && cond && cross && scratch && batch > 0, "pf_unet_prepare_cond: bad arguments");
  if (!u->wt.wdev) return set_error(PF_ESTATE, "pf_unet_prepare_cond: weights not bound (call pf_unet_bind_weights)");
  PF_REQUIRE(u->cross_total > 0, "pf_unet_prepare_cond: this UNet has no transformer block");
  PF_REQUIRE(scratch_bytes >= (size_t)batch * u->cross_total * sizeof(float), "pf_unet_prepare_cond: scratch too small");
  Ctx c = make_ctx(u, batch, 1, 0);   // a live context without a workspace (and without the profiler)
  c.dry = false; c.s = (hipStream_t)stream; c.W = u->wt.wdev;
  cross_bias_launches(u, c, cond, batch, cross, static_cast<float*>(scratch));
  return c.rc;
}

int pf_unet_n_launches_prepared(const pf_unet* u, int batch, int n_cond, int has_time, int has_cross) {
  if (!u || batch <= 0 || n_cond <= 0) return 0;
  return unet_plan(make_ctx(u, batch, n_cond, 0, has_time != 0, has_cross != 0 && n_cond == 1)).n_launch;
}

int pf_unet_set_option(pf_unet* u, int option, int value) {
  PF_REQUIRE(u && option >= 0 && option < PF_OPT_COUNT && value >= PF_OPT_AUTO && value <= PF_OPT_ON, "pf_unet_set_option: bad arguments");
  u->po.opt[option] = value;
  return PF_OK;
}
int pf_unet_track_absmax(pf_unet* u, void* device_word) {
  PF_REQUIRE(u, "null handle");
  u->po.amax_slot = device_word;
  return PF_OK;
}
int pf_unet_get_option(const pf_unet* u, int option) { return (u && option >= 0 && option < PF_OPT_COUNT) ? u->po.opt[option] : -2; }

int pf_unet_set_precision(pf_unet* u, int precision) {
  PF_REQUIRE(u && (precision == PF_PREC_F32 || precision == PF_PREC_BF16X3), "pf_unet_set_precision: bad arguments");
  u->po.precision = precision;
  return PF_OK;
}
int pf_unet_get_precision(const pf_unet* u) { return u ? u->po.precision : -1; }

int pf_unet_set_profiling(pf_unet* u, int enabled) {
  PF_REQUIRE(u, "null handle");
  u->profiling = enabled != 0;
  u->prof.rec.clear();
  return PF_OK;
}

int pf_unet_profile_read(pf_unet* u, int* kind, float* ms, double* flops, int capacity) {
  PF_REQUIRE(u && kind && ms && flops, "pf_unet_profile_read: null argument");
  const Profiler& p = u->prof;
  const int n = std::min((int)p.rec.size(), capacity);
  for (int i = 0; i < n; ++i) {
    PF_CHECK_HIP(hipEventSynchronize(p.ev[(size_t)i * 2 + 1]));
    float v = 0.f;
    PF_CHECK_HIP(hipEventElapsedTime(&v, p.ev[(size_t)i * 2], p.ev[(size_t)i * 2 + 1]));
    kind[i] = p.rec[i].kind; ms[i] = v; flops[i] = p.rec[i].flops;
  }
  return n;
}

int pf_unet_profile_read_direct(pf_unet* u, double* direct_flops, int capacity) {
  PF_REQUIRE(u && direct_flops, "pf_unet_profile_read_direct: null argument");
  const int n = std::min((int)u->prof.rec.size(), capacity);
  for (int i = 0; i < n; ++i) direct_flops[i] = u->prof.rec[i].direct;
  return n;
}

}  // extern "C"
