"""ORACLE (test infrastructure - NOT product code).

CPU restatement of the first-stage autoencoder (the model behind ``pf_autoenc``), written functionally over a plain
``{key: tensor}`` dict keyed like ``weights.synth_autoencoder_state`` (= the reference ``Autoencoder`` state_dict without
``loss.*``).  Only ``tests/`` may import it; the product path (``polyffusion_amd``) never does.

Written from the architecture as this repository documents it: the ``pf_autoenc`` section of ``include/pfhip.h``,
``polyffusion_amd/autoencoder.py`` (``autoencoder_param_shapes`` walks the same modules) and the comments of
``csrc/autoencoder.hip`` / ``csrc/small_kernels.hip``:

  Encoder   conv_in 3x3; per level ``n_resnet_blocks`` ResnetBlocks, then (all but the last level) a DownSample
            = F.pad(x, (0, 1, 0, 1)) + Conv2d(3, stride 2, padding 0); mid = ResnetBlock, AttnBlock, ResnetBlock;
            GroupNorm, SiLU, conv_out 3x3 to 2 * z_channels
  moments   quant_conv 1x1 (2 z -> 2 emb); mean | log_var = its halves; log_var clamped to [-30, 20]
  sample    scale * (mean + exp(log_var / 2) * noise)
  Decoder   post_quant_conv 1x1 (emb -> z) on z / scale; conv_in 3x3 to the top width; mid; from the last level up
            ``n_resnet_blocks + 1`` ResnetBlocks per level, then (all but level 0) an UpSample = nearest x2 + Conv2d(3, padding 1);
            GroupNorm, SiLU, conv_out 3x3
  ResnetBlock  GroupNorm, SiLU, conv1, GroupNorm, SiLU, conv2; + x, through the 1x1 ``nin_shortcut`` where the widths differ
  AttnBlock    GroupNorm (no SiLU), q | k | v 1x1, ONE head of width C, softmax over keys of q.k * C^-0.5, proj_out 1x1, + x
  every GroupNorm is GroupNorm(32, eps 1e-6)

Arithmetic runs in the dtype of the state passed in: ``to_torch(state, torch.float64)`` gives the truth the GPU tests compare against,
float32 the "reference CPU path".  Pinning: ``tests/test_oracle_autoencoder.py`` holds the float64 run to every array of
``tests/golden/autoencoder.npz`` (float32 runs of the real reference) within the reference's own roundoff.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch
import torch.nn.functional as F

Tensors = Dict[str, torch.Tensor]

EPS = 1e-6
LOG_VAR_MIN, LOG_VAR_MAX = -30.0, 20.0


def to_torch(state, dtype=torch.float64) -> Tensors:
    return {k: torch.as_tensor(v).to(dtype) for k, v in state.items()}


def _conv(w: Tensors, p: str, x: torch.Tensor, **kw) -> torch.Tensor:
    return F.conv2d(x, w[p + ".weight"], w[p + ".bias"], **kw)


def _norm(w: Tensors, p: str, x: torch.Tensor) -> torch.Tensor:
    return F.group_norm(x, 32, w[p + ".weight"], w[p + ".bias"], eps=EPS)


def resnet_block(w: Tensors, p: str, x: torch.Tensor) -> torch.Tensor:
    h = _conv(w, p + ".conv1", F.silu(_norm(w, p + ".norm1", x)), padding=1)
    h = _conv(w, p + ".conv2", F.silu(_norm(w, p + ".norm2", h)), padding=1)
    if p + ".nin_shortcut.weight" in w:
        x = _conv(w, p + ".nin_shortcut", x)
    return x + h


def attn_block(w: Tensors, p: str, x: torch.Tensor) -> torch.Tensor:
    b, c, h, wd = x.shape
    y = _norm(w, p + ".norm", x)
    q, k, v = (_conv(w, p + n, y).flatten(2) for n in (".q", ".k", ".v"))      # [B, C, tokens]
    scores = (q.transpose(1, 2) @ k) / (c ** 0.5)                               # [B, query, key]
    out = (v @ F.softmax(scores, dim=-1).transpose(1, 2)).reshape(b, c, h, wd)  # out[:, :, query] = sum over keys of p * v[:, :, key]
    return x + _conv(w, p + ".proj_out", out)


def mid(w: Tensors, p: str, x: torch.Tensor) -> torch.Tensor:
    x = resnet_block(w, p + ".block_1", x)
    x = attn_block(w, p + ".attn_1", x)
    return resnet_block(w, p + ".block_2", x)


def encoder(w: Tensors, cfg, x: torch.Tensor) -> torch.Tensor:
    """image [B, in_channels, H, W] -> [B, 2 * z_channels, H / f, W / f]"""
    n_levels = len(cfg.channel_multipliers)
    x = _conv(w, "encoder.conv_in", x, padding=1)
    for i in range(n_levels):
        for j in range(cfg.n_resnet_blocks):
            x = resnet_block(w, f"encoder.down.{i}.block.{j}", x)
        if i != n_levels - 1:
            x = _conv(w, f"encoder.down.{i}.downsample.conv", F.pad(x, (0, 1, 0, 1)), stride=2)
    x = mid(w, "encoder.mid", x)
    return _conv(w, "encoder.conv_out", F.silu(_norm(w, "encoder.norm_out", x)), padding=1)


def decoder(w: Tensors, cfg, z: torch.Tensor) -> torch.Tensor:
    """[B, z_channels, h, w] -> image [B, out_channels, h * f, w * f]"""
    n_levels = len(cfg.channel_multipliers)
    x = _conv(w, "decoder.conv_in", z, padding=1)
    x = mid(w, "decoder.mid", x)
    for i in reversed(range(n_levels)):
        for j in range(cfg.n_resnet_blocks + 1):
            x = resnet_block(w, f"decoder.up.{i}.block.{j}", x)
        if i != 0:
            x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)   # nearest x2
            x = _conv(w, f"decoder.up.{i}.upsample.conv", x, padding=1)
    return _conv(w, "decoder.conv_out", F.silu(_norm(w, "decoder.norm_out", x)), padding=1)


def encode(w: Tensors, cfg, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The posterior's (mean, log_var), each [B, emb_channels, H / f, W / f], log_var clamped to [-30, 20]."""
    moments = _conv(w, "quant_conv", encoder(w, cfg, x))
    mean, log_var = torch.chunk(moments, 2, dim=1)
    return mean, torch.clamp(log_var, LOG_VAR_MIN, LOG_VAR_MAX)


def sample(mean: torch.Tensor, log_var: torch.Tensor, noise: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    return scale * (mean + torch.exp(0.5 * log_var) * noise)


def decode(w: Tensors, cfg, z: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    return decoder(w, cfg, _conv(w, "post_quant_conv", z / scale))


def forward(w: Tensors, cfg, x: torch.Tensor, noise: torch.Tensor):
    """(decode(sample), mean, log_var) with the given noise, at scale 1."""
    mean, log_var = encode(w, cfg, x)
    return decode(w, cfg, sample(mean, log_var, noise)), mean, log_var
