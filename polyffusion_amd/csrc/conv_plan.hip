// conv_plan.hip - host only: the checks, the plan and the parameter block of a pf_conv2d launch (conv_plan.h).
#include <math.h>
#include "conv_plan.h"

namespace pf {

static int chip_cus() { return num_cus(); }   // the one place the conv family asks (the thresholds below were measured on 256 CUs; they are rounds of the chip, not literals)

int conv_validate(const pf_conv_args& a) {
  PF_REQUIRE(a.ks == 1 || a.ks == 3, "conv: ks must be 1 or 3 (got %d)", a.ks);
  PF_REQUIRE(a.stride == 1 || a.stride == 2, "conv: stride must be 1 or 2");
  PF_REQUIRE(!(a.ks == 1 && (a.stride != 1 || a.ups)), "conv: 1x1 supports stride 1 without upsampling only");
  PF_REQUIRE(!(a.ups && a.stride != 1), "conv: upsample fold needs stride 1");
  PF_REQUIRE(a.pad_mode == PF_PAD_SAME || (a.pad_mode == PF_PAD_BOTTOM_RIGHT && a.ks == 3 && a.stride == 2 && a.hin % 2 == 0 && a.win % 2 == 0),
             "conv: pad_mode %d needs ks=3, stride 2 and an even input size", a.pad_mode);
  PF_REQUIRE(a.c0 > 0 && a.c0 % 32 == 0 && a.c1 >= 0 && a.c1 % 32 == 0, "conv: channel counts must be multiples of 32 (c0=%d c1=%d)", a.c0, a.c1);
  PF_REQUIRE(a.x0 && (a.c1 == 0 || a.x1), "conv: null input");
  PF_REQUIRE(a.n > 0 && a.w && a.out, "conv: null weight/output");
  PF_REQUIRE(a.prologue >= 0 && a.prologue <= 3, "conv: bad prologue %d", a.prologue);
  PF_REQUIRE(a.prologue == 0 || (a.sc && a.sh), "conv: prologue needs sc/sh");
  PF_REQUIRE(!a.gn_stats0 || (a.precision == PF_PREC_BF16X3 && (a.prologue == 1 || a.prologue == 2) && a.gn_gamma && a.gn_beta && a.gn_groups > 0 &&
                              (a.c0 + a.c1) % a.gn_groups == 0 && a.c0 + a.c1 <= 1024 && a.gn_tiles0 > 0 && (a.c1 == 0 || (a.gn_stats1 && a.gn_tiles1 > 0))),
             "conv: fused GroupNorm finalize needs the bf16x3 path, prologue 1/2, gamma/beta, statistics of every source and <= 1024 channels");
  PF_REQUIRE(a.prologue != 3 || (a.mean && a.rstd && a.ks == 1), "conv: LayerNorm prologue needs mean/rstd and ks=1");
  PF_REQUIRE(!a.geglu || (a.n % 64 == 0 && !a.sbias && !a.res), "conv: geglu needs N %% 64 == 0 and no residual");
  PF_REQUIRE((a.ks == 3 && (a.prologue == 0 || a.prologue == 1)) || a.ks == 1, "conv: 3x3 supports prologue 0/1 only");
  PF_REQUIRE(!(a.ks == 3 && a.prologue == 1 && (a.ups || a.stride == 2)), "conv: GN prologue only on plain 3x3");
  PF_REQUIRE(!(a.ks == 3 && a.prologue == 0 && !a.ups && a.stride == 1), "conv: plain 3x3 without prologue is not instantiated");
  PF_REQUIRE(!(a.ks == 1 && a.prologue == 1), "conv: 1x1 with SiLU prologue is not instantiated");
  PF_REQUIRE(!(a.stats_out && a.geglu), "conv: statistics are not available with the GeGLU epilogue");
  PF_REQUIRE(!a.qkv_planes || (a.ks == 1 && a.n % 192 == 0 && a.win % 16 == 0 && !a.geglu && !a.res && !a.sbias && !a.stats_out),
             "conv: qkv planes need ks=1, N = 3*heads*64 and L %% 16 == 0");

  PF_REQUIRE(a.precision == PF_PREC_F32 || a.precision == PF_PREC_BF16X3, "conv: bad precision %d", a.precision);
  PF_REQUIRE(!a.ups_fold || (a.ups && a.precision == PF_PREC_BF16X3 && a.ks == 3 && a.stride == 1 && a.prologue == 0 && !a.res && !a.skip_w),
             "conv: ups_fold needs ups=1, bf16x3, ks=3, no prologue / residual");
  PF_REQUIRE(!a.skip_w || (a.precision == PF_PREC_BF16X3 && a.ks == 3 && a.stride == 1 && !a.ups && a.skip_x0 && a.skip_c0 > 0 &&
                           a.skip_c0 % 32 == 0 && a.skip_c1 % 32 == 0 && (a.skip_c1 == 0 || a.skip_x1) && !a.geglu),
             "conv: fused skip projection needs bf16x3, ks=3, stride 1, channel counts multiples of 32");
  PF_REQUIRE(!a.out_planes || (a.precision == PF_PREC_BF16X3 && a.ks == 1 && !a.stats_out && a.ld_out % 8 == 0 &&
                               (a.geglu ? a.n / 2 : a.n) % 8 == 0),
             "conv: out_planes needs bf16x3, ks=1, no statistics, ld_out and n multiples of 8");
  PF_REQUIRE(!a.a_planes || (a.precision == PF_PREC_BF16X3 && a.ks == 1 && a.prologue == 0 && a.c1 == 0),
             "conv: a_planes needs bf16x3, ks=1, no prologue, single source");
  PF_REQUIRE(!a.a_planes || (size_t)a.batch * a.win * a.c0 * 2 * 2 < ((size_t)1 << 31),
             "gemm_planes: the A plane pair must stay below 2 GiB (32-bit offsets of the direct-to-LDS loads)");
  return PF_OK;
}

bool conv_wino_eligible(const pf_conv_args& a) {
  return a.wino > 0 && a.w_wino && a.precision == PF_PREC_BF16X3 && a.ks == 3 && a.stride == 1 && !a.ups && !a.ups_fold && a.prologue == 1 &&
         a.hin % 16 == 0 && a.win % 16 == 0 && a.n % 64 == 0 && a.c0 % 32 == 0 && a.c1 % 32 == 0 && !a.geglu && !a.out_planes && !a.qkv_planes &&
         a.c0 + a.c1 <= 1024 && a.hin * a.win < (1 << 20) &&
         (long long)a.batch * a.hin * a.win * (a.c0 > a.c1 ? a.c0 : a.c1) * 4 < (1ll << 31) &&      // 32-bit buffer offsets
         (long long)a.batch * a.hin * a.win * (a.ld_out > a.ld_res ? a.ld_out : a.ld_res) * 4 < (1ll << 31) &&
         !a.skip_w && (a.ld_out & 3) == 0 && (!a.res || (a.ld_res & 3) == 0);
}
// PF_OPT_CONV_WINO = AUTO follows the same-box A/B of profiles/r06_ab_winograd.md: the form wins where the K loop is long enough to
// carry its per-tile exchange - 192 input channels and more, or 128 and more from the 32x32 level down - and when its 16x16-pixel x
// 64-channel workgroups fill at least three quarters of the CUs.
bool conv_wino_auto(const pf_conv_args& a) {
  const int cin_ = a.c0 + a.c1;
  const int wgs = a.batch * (a.hin / 16) * (a.win / 16) * (a.n / 64);
  const bool deep = cin_ >= 192 || (cin_ >= 128 && a.hin * a.win <= 1024);
  return deep && wgs * 4 >= chip_cus() * 3;
}

// tile choice shared by both arithmetic modes: 0 = 128 px x 128 ch, 1 = 128 px x 64 ch, 2 = 64 px x 64 ch
static int conv_pick_tile(const pf_conv_args& a, int hout, int wout, int cus) {
  if (a.geglu) return 0;
  const int npad = (a.n + 63) / 64 * 64;
  const int mt128 = a.ks == 1 ? a.batch * hout * cdiv(wout, 128) : a.batch * cdiv(hout, 8) * cdiv(wout, 16);
  if (a.ks == 3 && a.stride == 2) return 2;
  if (a.force_tile >= 1 && a.force_tile <= 3 && a.precision == PF_PREC_BF16X3 && a.stride == 1 && !a.ups && !a.ups_fold &&
      (a.ks == 3 || a.a_planes) && (a.force_tile != 1 || npad % 128 == 0)) return a.force_tile - 1;   // measurement aid (pf_conv_args.force_tile)
  // bf16x3 3x3: the wide tile + split-K beats twice as many narrow tiles; planes GEMMs (both operands direct-to-LDS): one 128x128 workgroup
  // per CU beats two 128x64 ones as soon as every CU gets one (measured at M = 16384, N = 256: K = 256 18.1 -> 16.1 us, K = 1024 37.5 -> 33.9 us)
  // bf16x3 3x3 with 64 output channels in all (the 128x128 level): a 16x16-pixel tile when that still gives every CU two rounds of
  // two workgroups - each wave then owns 128 pixels x 32 channels (four A fragments per weight fragment instead of two)
  if (a.precision == PF_PREC_BF16X3 && a.ks == 3 && a.stride == 1 && !a.ups && !a.ups_fold && npad == 64 && hout % 16 == 0 && wout % 16 == 0 &&
      a.batch * (hout / 16) * (wout / 16) >= 4 * cus && !a.skip_w && a.c0 + a.c1 >= 128 && !a.no_t16) return 3;
  // (the same 16x16-pixel footprint for the 128-channel tile - 128 x 64 per wave, one workgroup per CU - measured worse at the 64x64
  // level: r64_128_128 55.3 -> 57 us, the fused-skip form 79 -> 82, only the K = 3456 conv gained 2.5 %)
  const bool wide_at_256 = a.precision == PF_PREC_BF16X3 && (a.ks == 3 || a.a_planes);
  if (npad % 128 == 0 && mt128 * (npad / 128) >= (wide_at_256 ? cus : 2 * cus)) return 0;
  // bf16x3 3x3: the 128 px x 64 ch tile as soon as it gives every CU a workgroup - at B = 8 the 32x32 level has exactly 256 of them and they
  // beat 512 narrow tiles by 6-10 % (tools/sweep_conv.py, profiles/r05_sweep_conv_before.log); below that the 64 px tile fills more CUs
  const bool bf3x3 = a.precision == PF_PREC_BF16X3 && a.ks == 3 && a.stride == 1 && !a.ups;
  if (mt128 * (npad / 64) >= (bf3x3 ? cus : 2 * cus)) return 1;
  return 2;
}

// split-K (bf16x3 3x3 only): layers whose tile grid cannot fill the chip (the 16x16 level at batch 16, most levels at
// small batch) run ksplit K-slices per tile and a reduce kernel that also applies the epilogue
static int ksplit_wanted(const pf_conv_args& a, const ConvPlan& pl, bool wino, int cus) {
  if (a.precision != PF_PREC_BF16X3 || a.ks != 3 || a.stride != 1 || a.geglu || a.ups_fold || wino) return 1;
  if ((pl.hout * pl.wout) % 64 != 0) return 1;
  const int blocks = a.batch * cdiv(pl.hout, pl.th) * cdiv(pl.wout, pl.tw) * cdiv((a.n + 63) / 64 * 64, 64);
  const int nchunk = (a.c0 + a.c1) / 32;
  if (a.force_ksplit >= 1 && nchunk % a.force_ksplit == 0) return a.force_ksplit;   // measurement aid (pf_conv_args.force_ksplit)
  // Round 5, from a sweep of every layer shape at B = 1 / 8 / 16 (tools/sweep_conv.py, profiles/r05_sweep_conv_before.log): the split pays
  // only for DEEP K on FEW workgroups - its fp32 partial sums and the reduce launch cost ~8 us, which a K = 2304 loop (25 us unsplit on
  // any number of workgroups, 17 us with the intra-workgroup split) never earns back: B = 8, 16x16 level 22.9 -> 17.4 us, B = 1, 64x64
  // level 19.5 -> 11.5 us without it.  K >= 4608 on at most half the CUs, or K >= 3456 on at most a quarter: four slices (+10 ... +30 %).
  if (nchunk % 4 == 0 && ((nchunk >= 16 && blocks <= cus / 2) || (nchunk >= 12 && blocks <= cus / 4))) return 4;
  return 1;
}

// everything that depends on whether the wanted split got its scratch: the split, the form of the plain split 3x3 conv, the statistics layout
static void conv_plan_resolve(ConvPlan& pl, const pf_conv_args& a, bool granted, int cus) {
  pl.ksplit = granted ? pl.ksplit_wanted : 1;
  pl.wave_groups = 1;
  if (pl.form == PF_CONV_FORM_SPLIT || pl.form == PF_CONV_FORM_SPLIT_KG2 || pl.form == PF_CONV_FORM_SPLIT_PINGPONG) {
    pl.form = PF_CONV_FORM_SPLIT;
    if (a.ks == 3 && a.stride == 1 && !a.ups) {
      const int cin = a.c0 + a.c1, scin = a.skip_c0 + a.skip_c1;
      // no more tiles than CUs (and an even number of K chunks): two wave groups per workgroup split K (see conv_bf3_kernel)
      const int blocks = a.batch * cdiv(pl.hout, pl.th) * cdiv(pl.wout, 16) * cdiv((a.n + 63) / 64 * 64, pl.bn);
      const bool two = pl.ksplit == 1 && blocks <= cus && (cin / 32) % 2 == 0 && (!a.skip_w || (scin / 32) % 2 == 0);
      // (the 128x128 tile split the same way measured neutral - its two wave groups run in lockstep behind the shared barrier - DESIGN.md 3)
      if (pl.tile == 2 && two) pl.form = PF_CONV_FORM_SPLIT_KG2;
      // ... but run as two groups half a tap apart (conv_bf3_pingpong) it gains: one group's fragment reads / copies / halo arithmetic
      // hide behind the other's MFMAs (B = 16: the 32x32 level; B = 8: the 64x64 level)
      // (from K = 2304 up: at K = 576 ... 1728 the two-group form measured 3-6 % behind the four-wave one - r32_128_256, r64_128_128 at B = 8)
      else if (!a.no_pp && pl.tile == 0 && two && cin >= 256) pl.form = PF_CONV_FORM_SPLIT_PINGPONG;
      if (pl.form != PF_CONV_FORM_SPLIT) pl.wave_groups = 2;
    }
  }
  if (pl.form == PF_CONV_FORM_WINO) pl.stats_tiles = (pl.hout / 16) * (pl.wout / 16);   // one statistics tile per 16x16-pixel workgroup
  else if (pl.ksplit > 1) pl.stats_tiles = pl.hout * pl.wout / 64;   // the reduce kernel emits one statistics tile per 64 rows
  else if (a.ups_fold) pl.stats_tiles = cdiv(a.hin, pl.th) * cdiv(a.win, pl.tw) * 4;   // tiles walk the source grid, one statistics tile per parity
  else pl.stats_tiles = cdiv(pl.hout, pl.th) * cdiv(pl.wout, pl.tw);
}

ConvPlan conv_plan(const pf_conv_args& a) {
  ConvPlan pl;
  memset(&pl, 0, sizeof pl);
  const int cus = chip_cus();
  pl.hout = a.hin; pl.wout = a.win;
  if (a.ups) { pl.hout *= 2; pl.wout *= 2; }
  if (a.stride == 2) { pl.hout = (pl.hout - 1) / 2 + 1; pl.wout = (pl.wout - 1) / 2 + 1; }
  const bool wino = conv_wino_eligible(a);
  pl.form = a.a_planes ? PF_CONV_FORM_PLANES : a.precision != PF_PREC_BF16X3 ? PF_CONV_FORM_F32 : wino ? PF_CONV_FORM_WINO :
            (a.ks == 3 && a.ups_fold) ? PF_CONV_FORM_UPFOLD : PF_CONV_FORM_SPLIT;
  pl.ks = pl.form == PF_CONV_FORM_UPFOLD ? 2 : a.ks; pl.stride = a.stride; pl.ups = a.ups && pl.form != PF_CONV_FORM_UPFOLD; pl.pro = a.prologue;
  pl.tile = conv_pick_tile(a, pl.hout, pl.wout, cus);
  if (a.ks == 1) { pl.th = 1; pl.tw = pl.tile == 2 ? 64 : 128; }
  else if (a.stride == 2) { pl.th = 4; pl.tw = 16; }
  else { pl.th = pl.tile == 3 ? 16 : pl.tile == 2 ? 4 : 8; pl.tw = 16; }
  pl.bn = pl.tile == 0 ? 128 : 64;
  pl.skip = a.skip_w != nullptr;
  pl.ksplit_wanted = ksplit_wanted(a, pl, wino, cus);
  pl.splitk_ws_bytes = pl.ksplit_wanted > 1 ? (size_t)pl.ksplit_wanted * a.batch * pl.hout * pl.wout * a.n * sizeof(float) : 0;
  if (wino) { pl.th = 16; pl.tw = 16; pl.bn = 64; }
  // planes GEMM ring depth: the deepest that still lets two workgroups share a CU's 160 KB (a 128x128 stage is 32 KB); the 64-row tile
  // is the register path's row tiling, so the GroupNorm statistics tiles of the two agree
  if (pl.form == PF_CONV_FORM_PLANES) pl.ring = pl.tile == 0 ? 2 : 3;
  const double skip = a.skip_w ? (double)(a.skip_c0 + a.skip_c1) : 0.0;   // fused 1x1 projection of a second tensor
  const double per_tap = 2.0 * a.batch * pl.hout * pl.wout * (double)a.n;
  // folded upsampling conv: 2x2 taps per output pixel; Winograd F(2x2, 3x3): 16 products per 2x2 output pixels (work actually done)
  pl.direct_flops = per_tap * ((a.c0 + a.c1) * (a.ups_fold ? 4.0 : (double)(a.ks * a.ks)) + skip);
  pl.flops = wino ? per_tap * ((a.c0 + a.c1) * 4.0 + skip) : pl.direct_flops;
  conv_plan_resolve(pl, a, pl.splitk_ws_bytes && a.splitk_ws && a.splitk_ws_bytes >= pl.splitk_ws_bytes, cus);
  return pl;
}

void conv_plan_grant_split(ConvPlan& pl, const pf_conv_args& a) { conv_plan_resolve(pl, a, pl.splitk_ws_bytes != 0, chip_cus()); }

ConvP conv_params(const pf_conv_args& a, const ConvPlan& pl) {
  ConvP p;
  memset(&p, 0, sizeof p);
  p.x0 = a.x0; p.x1 = a.x1; p.c0 = a.c0; p.c1 = a.c1; p.x1_bmod = a.x1_bmod;
  p.B = a.batch; p.Hin = a.hin; p.Win = a.win; p.Hout = pl.hout; p.Wout = pl.wout;
  p.w = a.w; p.N = a.n; p.Npad = (a.n + 63) / 64 * 64;
  p.sc = a.sc; p.sh = a.sh; p.mean = a.mean; p.rstd = a.rstd;
  p.bias = a.bias; p.sbias = a.sbias; p.ld_sbias = a.ld_sbias; p.res = a.res; p.ld_res = a.ld_res;
  p.sb_rows = reinterpret_cast<const long long*>(a.sbias_rows); p.sb_nrows = a.sbias_nrows;
  p.geglu = a.geglu; p.out = a.out; p.ld_out = a.ld_out; p.stats = a.stats_out;
  p.qkv = a.qkv_planes; p.out_planes = a.out_planes;
  p.ksplit = pl.ksplit;
  p.partial = pl.ksplit > 1 ? static_cast<float*>(a.splitk_ws) : nullptr;
  if (a.gn_stats0 && (a.prologue == 1 || a.prologue == 2)) {
    p.gn_s0 = a.gn_stats0; p.gn_t0 = a.gn_tiles0; p.gn_s1 = a.gn_stats1; p.gn_t1 = a.gn_tiles1;
    p.gn_gamma = a.gn_gamma; p.gn_beta = a.gn_beta; p.gn_eps = a.gn_eps; p.gn_groups = a.gn_groups;
  }
  p.sx0 = a.skip_x0; p.sc0 = a.skip_c0; p.sx1 = a.skip_x1; p.sc1 = a.skip_c1; p.sw = a.skip_w; p.bias2 = a.skip_w ? a.skip_bias : nullptr;
  p.amax = static_cast<unsigned*>(a.absmax_slot);
  p.pad_br = a.pad_mode == PF_PAD_BOTTOM_RIGHT;
  if (pl.form == PF_CONV_FORM_WINO) p.w = a.w_wino;                                    // the transformed packing (N % 64 == 0: Npad = N)
  if (pl.form == PF_CONV_FORM_PLANES) { p.Hin = 1; p.Hout = 1; }                       // rows of a matrix: x0 = hi | lo planes [M][K]
  if (pl.form == PF_CONV_FORM_UPFOLD) { p.Hout = a.hin; p.Wout = a.win; p.fold = 1; }  // tiles walk the source grid; every workgroup stores one parity of its pixels
  p.tiles_x = cdiv(p.Wout, pl.tw); p.tiles_y = cdiv(p.Hout, pl.th); p.nt = cdiv(p.Npad, pl.bn);
  conv_fill_divs(p);
  return p;
}

int launch_conv(const pf_conv_args& a, hipStream_t stream) {
  if (int rc = conv_validate(a)) return rc;
  const ConvPlan pl = conv_plan(a);
  ConvP p = conv_params(a, pl);
  if (pl.form == PF_CONV_FORM_F32) return launch_conv_f32(p, pl, stream);
  if (pl.form == PF_CONV_FORM_PLANES) return launch_gemm_planes(p, pl, stream);
  return pl.form == PF_CONV_FORM_WINO ? launch_conv_wino(p, pl, stream) : launch_conv_bf3(p, pl, stream);
}

bool split_hi_lo(float v, unsigned short* hi, unsigned short* lo) {
#ifdef PF_X3_F16
  const float vs = fminf(fmaxf(v * PF_X3_WS, -65504.f), 65504.f);
  const _Float16 fh = (_Float16)vs, fl = (_Float16)(vs - (float)fh);
  memcpy(hi, &fh, 2); memcpy(lo, &fl, 2);
  return vs == v * PF_X3_WS;
#else
  auto f2bf_rne = [](float f) { unsigned int u; memcpy(&u, &f, 4); u += 0x7FFFu + ((u >> 16) & 1u); return (unsigned short)(u >> 16); };
  const unsigned int hu = (unsigned int)(*hi = f2bf_rne(v)) << 16;
  float hf; memcpy(&hf, &hu, 4);
  *lo = f2bf_rne(v - hf);
  return true;
#endif
}

}  // namespace pf
