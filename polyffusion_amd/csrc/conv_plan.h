// conv_plan.h - what a pf_conv2d launch is, decided in one place (conv_plan.hip, host only): the argument checks, the form / tile / K split
// a set of arguments gets, and the one copy of the arguments into the kernels' parameter block.  The launchers only map a plan to a template
// instantiation; the block emitters and the query entries read the same plan, so a consumer's statistics layout is the launcher's by construction.
#pragma once
#include "conv_common.h"

namespace pf {

struct ConvPlan {
  int form;                  // PF_CONV_FORM_* (include/pfhip.h)
  int ks, stride, ups, pro;  // the kernel's: taps per side (2: the parity-folded conv), stride, halo read through nearest x2, prologue
  int hout, wout;            // output size, `ups` and `stride` applied
  int tile;                  // 0: 128 px x 128 ch, 1: 128 px x 64 ch, 2: 64 px x 64 ch, 3: 16x16 px x 64 ch (the direct forms' choice)
  int th, tw, bn;            // pixels x channels a workgroup of this form owns (planes GEMM: 1 x rows; Winograd: 16 x 16 x 64)
  int wave_groups;           // 2: two 4-wave groups split K inside the workgroup (KG2, ping-pong)
  int skip, ring;            // the fused 1x1 skip projection runs; planes GEMM: stages of the operand ring
  int ksplit_wanted;         // K slices across workgroups the arguments would like ...
  size_t splitk_ws_bytes;    // ... the scratch they need (0: no split) ...
  int ksplit;                // ... and what they get with the splitk_ws they carry (1: none; a reduce launch follows otherwise)
  int stats_tiles;           // per-sample tiles emitted into stats_out
  double flops, direct_flops;   // operations executed / of the direct form (they differ for Winograd)
};

int conv_validate(const pf_conv_args& a);          // PF_OK, or PF_EINVAL with pf_last_error() set
ConvPlan conv_plan(const pf_conv_args& a);         // touches no device; arguments need not be valid
// the caller has attached the scratch the plan wanted since (BlockCtx::conv sizes it from the plan; form and statistics layout depend on it)
void conv_plan_grant_split(ConvPlan& pl, const pf_conv_args& a);
ConvP conv_params(const pf_conv_args& a, const ConvPlan& pl);
// eligibility of a launch for the fused Winograd form, and the PF_OPT_AUTO rule of the blocks that ask for it
bool conv_wino_eligible(const pf_conv_args& a);
bool conv_wino_auto(const pf_conv_args& a);
// form launchers (obey the plan; no decisions)
int launch_conv_f32(ConvP& p, const ConvPlan& pl, hipStream_t stream);
int launch_conv_bf3(ConvP& p, const ConvPlan& pl, hipStream_t stream);      // + the split-K reduce when pl.ksplit > 1
int launch_conv_wino(ConvP& p, const ConvPlan& pl, hipStream_t stream);
int launch_gemm_planes(ConvP& p, const ConvPlan& pl, hipStream_t stream);

// hi = round(v), lo = round(v - hi) in the split kernels' element type (bf16, or fp16 of v * PF_X3_WS); false: v does not fit (fp16: clamped)
bool split_hi_lo(float v, unsigned short* hi, unsigned short* lo);

}  // namespace pf
