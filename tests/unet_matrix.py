"""The UNet plan matrix: architectures, image shapes, batches and plan options that pf_unet_create accepts and that no other test of the
suite builds, with seeded inputs and the float64 oracle (oracle/unet_ref.py on float64 weights) of every case.  Used by
tests/test_unet_matrix.py (no GPU: the oracle pinned to the real reference at three of these architectures, host plan facts, reach checks)
and tests/test_gpu_unet_matrix.py (-m gpu).

What is under test is the host code that wires the kernels - run() and run_st() of csrc/unet.hip and the shared emitters of
csrc/unet_blocks.hip: buffer rotation, which launch form runs, which statistics feed which GroupNorm, what guidance groups share.  Each
kernel has a float64 matrix of its own (conv_matrix, attn_matrix, small_matrix, ...).

Every configuration has in_channels = out_channels = 2 unless the line says otherwise ("32, (1,2), 1, att (1,), 2 heads, tf 1, d_cond 32" is
SMALL, the net the rest of the suite uses).  Images are H x W.

  a      32, (1,2), 2 ResBlocks, att (1,), 2 heads, tf 2, d_cond 32; 16x16, B 3, n_cond 1
         two transformer layers on the fp32-A path (d_head 32): the t0 / t1 / t2 rotation of run_st; two ResBlocks per level
  b      as a; 16x16, B 2, n_cond 3
         the general cross-attention inside the two-layer rotation (swap(t1, t2) twice)
  c-n1   32, (1,2), 1, att (0,1), 1 head, tf 1, d_cond 32; 32x16, B 2, n_cond 1
  c-n5   the same, n_cond 5
         transformer widths 32 (d_head 32, 512 tokens) and 64 (d_head 64, 128 tokens): cross_uniform is false, the per-block mat-vecs
         of cross_bias_launches (and of pf_unet_prepare_cond); the planes path at C = 64 in the split modes only; attention at level 0:
         the shared-prefix plan leaves its shared phase after a single ResBlock; non-square
  d-16x8   64, (1,), 1, att (0,), 1 head, tf 2, d_cond 8; 16x8, B 3, n_cond 1; automatic, and attn_wide=True beside it (added: 128
           tokens have no 256-query form, the forced option must leave the level on the 128-query one - the plan used to hand the
           kernel a form it refuses)
  d-32x16  the same; 32x16, B 1, n_cond 1; automatic, and attn_wide=True beside it
         one level (no DownSample, no UpSample); the planes path with two layers (last_planes true for the second only); 512 tokens at
         B 1: the key-split attention with its merging launch inside a plan
  e-b3   64, (1,4), 1, att (1,), 4 heads, tf 2, d_cond 64; 32x16, B 3, n_cond 1; automatic, and mlp_fused=True beside it
  e-n4   the same; 32x16, B 1, n_cond 4; automatic, and mlp_fused=True beside it
         C = 256 at 128 tokens.  Forced: layer 0 is the plain fused launch (the `continue` of run_st), layer 1 the launch with proj_out
         and the tile statistics the next GroupNorm reads.  Automatic (far below the rule's row count): the chain
  f      64, (1,2), 1, att (1,), 2 heads, tf 1, d_cond 32; 32x48, B 2, n_cond 1; automatic, conv_wino=True and conv_wino=False
         the fused Winograd form at the lower edge of wino_ok (32 pixels, co % 64) and on a non-square level, 384 tokens of planes
         attention below it
  g      32, (1,2), 1, att (), 1 head, tf 1, d_cond 32; 16x16, B 2, n_cond 1
         only the middle block has a transformer: under shared_x the whole down path stays shared and every skip is read through x1_bmod
  h-3to1 SMALL with in 3 / out 1, d_cond 4; 16x16, B 5, n_cond 1
  h-4to4 SMALL with in 4 / out 4; 16x16, B 1, n_cond 2
         the ends of the stem's and the head's channel ranges (the stem's statistics fall back to stats_pass); the smallest d_cond
  i      32, (1,2,2), 2 ResBlocks, att (1,2), 2 heads, tf 1, d_cond 32; 32x32, B 2, n_cond 1
         three levels with a repeated multiplier: ResBlocks with ci == co after a down step; 64 tokens at the deepest level
  j-6x10 SMALL; 6x10, B 2, n_cond 2
  j-b17  SMALL; 8x8, B 17, n_cond 1
         15 and 16 tokens, every tile wider than the image; an odd batch above 16

No case of the issue's table is dropped.  Weights are synth_unet_state(cfg, seed) with seed 0 (the seed the reference was compared with
at these architectures), x and cond are synth.gaussian tensors, t is taken from T_LIST so that both ends of the schedule are present in
every batch of two or more."""
from __future__ import annotations

from functools import lru_cache
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from oracle import unet_ref
from polyffusion_amd import synth
from polyffusion_amd.arch import UNetConfig
from polyffusion_amd.weights import synth_unet_state

T_LIST = (0, 999, 417, 3, 500, 77, 998, 250, 1, 640, 833, 12, 365, 700, 123, 950, 42)
Form = Tuple[Tuple[str, Optional[bool]], ...]   # plan options to force, as (name, value) pairs; (): everything automatic
AUTO: Form = ()


class Case(NamedTuple):
    name: str
    cfg: UNetConfig
    H: int
    W: int
    B: int
    n_cond: int
    seed: int = 0                      # weight seed
    forms: Tuple[Form, ...] = (AUTO,)  # every setting of the plan options the case runs under
    t_off: int = 0                     # where in T_LIST the batch's time steps start


def _cfg(channels, mult, blocks, att, heads, tf, d_cond, cin=2, cout=2):
    return UNetConfig(in_channels=cin, out_channels=cout, channels=channels, n_res_blocks=blocks, attention_levels=att,
                      channel_multipliers=mult, n_heads=heads, tf_layers=tf, d_cond=d_cond)


SMALL = _cfg(32, (1, 2), 1, (1,), 2, 1, 32)
CFG_A = _cfg(32, (1, 2), 2, (1,), 2, 2, 32)
CFG_C = _cfg(32, (1, 2), 1, (0, 1), 1, 1, 32)
CFG_D = _cfg(64, (1,), 1, (0,), 1, 2, 8)
CFG_E = _cfg(64, (1, 4), 1, (1,), 4, 2, 64)
CFG_F = _cfg(64, (1, 2), 1, (1,), 2, 1, 32)
CFG_G = _cfg(32, (1, 2), 1, (), 1, 1, 32)
CFG_H31 = _cfg(32, (1, 2), 1, (1,), 2, 1, 4, cin=3, cout=1)
CFG_H44 = _cfg(32, (1, 2), 1, (1,), 2, 1, 32, cin=4, cout=4)
CFG_I = _cfg(32, (1, 2, 2), 2, (1, 2), 2, 1, 32)

WIDE, FUSED = (("attn_wide", True),), (("mlp_fused", True),)
WINO_ON, WINO_OFF = (("conv_wino", True),), (("conv_wino", False),)

CASES = [
    Case("a", CFG_A, 16, 16, 3, 1),
    Case("b", CFG_A, 16, 16, 2, 3),
    Case("c-n1", CFG_C, 32, 16, 2, 1),
    Case("c-n5", CFG_C, 32, 16, 2, 5),
    Case("d-16x8", CFG_D, 16, 8, 3, 1, forms=(AUTO, WIDE)),
    Case("d-32x16", CFG_D, 32, 16, 1, 1, forms=(AUTO, WIDE), t_off=1),
    Case("e-b3", CFG_E, 32, 16, 3, 1, forms=(AUTO, FUSED)),
    Case("e-n4", CFG_E, 32, 16, 1, 4, forms=(AUTO, FUSED)),
    Case("f", CFG_F, 32, 48, 2, 1, forms=(AUTO, WINO_ON, WINO_OFF)),
    Case("g", CFG_G, 16, 16, 2, 1),
    Case("h-3to1", CFG_H31, 16, 16, 5, 1),
    Case("h-4to4", CFG_H44, 16, 16, 1, 2, t_off=1),
    Case("i", CFG_I, 32, 32, 2, 1),
    Case("j-6x10", SMALL, 6, 10, 2, 2),
    Case("j-b17", SMALL, 8, 8, 17, 1),
]
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
GOLDEN_CASES = ("b", "c-n5", "d-16x8")   # tests/golden/unet_matrix.npz (tools/make_goldens_unet_matrix.py)


def form_id(form: Form) -> str:
    return "auto" if not form else "+".join(f"{k}={'on' if v else 'off'}" for k, v in form)


def case_forms():
    """(case, form) pairs of the whole table, and their ids"""
    pairs = [(c, f) for c in CASES for f in c.forms]
    return pairs, [f"{c.name}-{form_id(f)}" for c, f in pairs]


def rms(a) -> float:
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def case_state(case):
    return synth_unet_state(case.cfg, case.seed)


def case_inputs(case, group: int = 0):
    """(x, t, cond) of a case as numpy (float32, int64, float32): what the GPU gets.  `group` > 0: the same x and t with another
    condition - the further guidance groups of a shared_x evaluation."""
    k = 1000 + 10 * CASES.index(BY_NAME[case.name])
    x = synth.gaussian((case.B, case.cfg.in_channels, case.H, case.W), k + 1)
    cond = synth.gaussian((case.B, case.n_cond, case.cfg.d_cond), k + 2 + 3 * group)
    t = np.array([T_LIST[(case.t_off + i) % len(T_LIST)] for i in range(case.B)], dtype=np.int64)
    return x, t, cond


@lru_cache(maxsize=None)
def _weights64(cfg, seed):
    return unet_ref.to_torch(synth_unet_state(cfg, seed), torch.float64)


@lru_cache(maxsize=None)
def oracle_case(case, group: int = 0):
    """The float64 truth of a case, computed once per process and shared: x, t, cond and eps.  Callers must leave the arrays unchanged."""
    x, t, cond = case_inputs(case, group)
    with torch.no_grad():
        eps = unet_ref.unet_forward(_weights64(case.cfg, case.seed), case.cfg, torch.from_numpy(x).double(), torch.from_numpy(t),
                                    torch.from_numpy(cond).double())
    out = {"x": x, "t": t, "cond": cond, "eps": eps.numpy()}
    for v in out.values():
        v.setflags(write=False)
    return out


def make_model(case, x3=None):
    """The product's handle of a case's architecture at its image size (no weights: pack_state_dict / load_state_dict)."""
    from polyffusion_amd.unet import UNetModel
    cfg = case.cfg
    return UNetModel(in_channels=cfg.in_channels, out_channels=cfg.out_channels, channels=cfg.channels, n_res_blocks=cfg.n_res_blocks,
                     attention_levels=cfg.attention_levels, channel_multipliers=cfg.channel_multipliers, n_heads=cfg.n_heads,
                     tf_layers=cfg.tf_layers, d_cond=cfg.d_cond, img_h=case.H, img_w=case.W, x3=x3)


def apply_form(model, form: Form):
    """Every plan option automatic, then the form's settings."""
    for name in model._OPTS:
        model.set_option(name, None)
    for name, value in form:
        model.set_option(name, value)
    return model
