"""The first-stage autoencoder of the reference (``main.py --model autoencoder``) on the HIP path.

Mirrors ``stable_diffusion/model/autoencoder.py`` (``Autoencoder``, ``GaussianDistribution``), ``models/model_autoencoder.py``
(``Polyffusion_Autoencoder.load_trained``) and what ``LatentDiffusion.autoencoder_encode`` / ``autoencoder_decode`` ask of it.  Both
halves are plans of the ``pf_autoenc`` handle of ``libpfhip.so`` (``csrc/autoencoder.hip``); PyTorch holds the buffers.  Inference
only: ``get_loss_dict`` (LPIPS + discriminator) is training code and raises.

The latent scaling factor is an argument of ``encode`` / ``decode`` (``scale=``, default 1): the encoder's last launch multiplies the
sample by it, the decoder's first launch divides ``z`` by it, which is how ``LatentDiffusion`` calls this model.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict
from dataclasses import dataclass
from typing import Mapping, Optional, Tuple

import torch

from . import _lib
from ._handle import ModelHandle
from .params import AUTOENCODER_PARAMS

PREFIX = "autoencoder."
LOG_VAR_MIN, LOG_VAR_MAX = -30.0, 20.0


@dataclass(frozen=True)
class AutoencoderConfig:
    """Constructor arguments of the reference ``Encoder`` / ``Decoder`` / ``Autoencoder`` (autoencoder.py:34-36, 117-125, 212-220)."""
    in_channels: int = 3
    out_channels: int = 3
    channels: int = 64
    channel_multipliers: Tuple[int, ...] = (1, 2, 4, 4)
    n_resnet_blocks: int = 2
    z_channels: int = 4
    emb_channels: int = 4

    @classmethod
    def from_params(cls, p: Mapping) -> "AutoencoderConfig":
        """From the keys of ``params/autoencoder.yaml`` (``n_res_blocks`` is the yaml's name for ``n_resnet_blocks``)."""
        return cls(int(p["in_channels"]), int(p["out_channels"]), int(p["channels"]), tuple(int(v) for v in p["channel_multipliers"]),
                   int(p["n_res_blocks"]), int(p["z_channels"]), int(p["emb_channels"]))

    @property
    def downscale(self) -> int:
        return 1 << (len(self.channel_multipliers) - 1)


def autoencoder_param_shapes(cfg: AutoencoderConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """The reference Autoencoder's state_dict keys and shapes without the training-only ``loss.*``, walked as ``Encoder.__init__`` /
    ``Decoder.__init__`` build it (autoencoder.py:136-175, 231-273).  ``pf_autoenc_param_info`` lists the same table."""
    out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()

    def conv(p, co, ci, k):
        out[p + ".weight"] = (co, ci, k, k); out[p + ".bias"] = (co,)

    def norm(p, c):
        out[p + ".weight"] = (c,); out[p + ".bias"] = (c,)

    def res(p, ci, co):
        norm(p + ".norm1", ci); conv(p + ".conv1", co, ci, 3)
        norm(p + ".norm2", co); conv(p + ".conv2", co, co, 3)
        if ci != co:
            conv(p + ".nin_shortcut", co, ci, 1)

    def mid(p, c):
        res(p + ".block_1", c, c)
        norm(p + ".attn_1.norm", c)
        for n in ("q", "k", "v", "proj_out"):
            conv(p + ".attn_1." + n, c, c, 1)
        res(p + ".block_2", c, c)

    L = len(cfg.channel_multipliers)
    ch = [m * cfg.channels for m in cfg.channel_multipliers]
    conv("encoder.conv_in", cfg.channels, cfg.in_channels, 3)
    cur = cfg.channels
    for i in range(L):
        for j in range(cfg.n_resnet_blocks):
            res(f"encoder.down.{i}.block.{j}", cur, ch[i])
            cur = ch[i]
        if i != L - 1:
            conv(f"encoder.down.{i}.downsample.conv", cur, cur, 3)
    mid("encoder.mid", cur)
    norm("encoder.norm_out", cur)
    conv("encoder.conv_out", 2 * cfg.z_channels, cur, 3)

    conv("decoder.conv_in", ch[-1], cfg.z_channels, 3)
    mid("decoder.mid", ch[-1])
    ins = {}
    cur = ch[-1]
    for i in reversed(range(L)):     # the order the blocks run in fixes their input widths ...
        ins[i] = cur
        cur = ch[i]
    for i in range(L):               # ... and the ModuleList, filled by insert(0), lists them by level
        cur = ins[i]
        for j in range(cfg.n_resnet_blocks + 1):
            res(f"decoder.up.{i}.block.{j}", cur, ch[i])
            cur = ch[i]
        if i != 0:
            conv(f"decoder.up.{i}.upsample.conv", cur, cur, 3)
    norm("decoder.norm_out", ch[0])
    conv("decoder.conv_out", cfg.out_channels, ch[0], 3)
    conv("quant_conv", 2 * cfg.emb_channels, 2 * cfg.z_channels, 1)
    conv("post_quant_conv", cfg.z_channels, cfg.emb_channels, 1)
    return out


class GaussianDistribution:
    """``GaussianDistribution`` of the reference (autoencoder.py:305-324) on moments the encoder already clamped.  ``sample`` draws
    with the library's kernel: from ``noise`` (a tensor shaped like ``mean``) or, without one, from the counter-based Philox stream
    ``(seed, stream_id, offset)`` - element i is what ``pf_randn(seed, stream_id, offset)`` writes at i.  The result is multiplied by
    the ``scale`` the distribution was encoded with."""

    def __init__(self, mean: torch.Tensor, log_var: torch.Tensor, scale: float = 1.0, lib=None):
        self.mean, self.log_var = mean, log_var
        self.std = torch.exp(0.5 * log_var)
        self.scale = float(scale)
        self._lib = lib or _lib.load()

    def sample(self, noise: Optional[torch.Tensor] = None, seed: int = 0, stream_id: int = 0, offset: int = 0) -> torch.Tensor:
        if noise is not None:
            if tuple(noise.shape) != tuple(self.mean.shape):
                raise RuntimeError(f"GaussianDistribution.sample: noise {tuple(noise.shape)}, expected {tuple(self.mean.shape)}")
            noise = noise.to(device=self.mean.device, dtype=torch.float32).contiguous()
        z = torch.empty_like(self.mean)
        _lib.check(self._lib.pf_gaussian_sample(self.mean.data_ptr(), self.log_var.data_ptr(), _lib.ptr(noise), int(seed), int(stream_id),
                                                int(offset), self.scale, z.data_ptr(), z.numel(), _lib.current_stream()),
                   "pf_gaussian_sample", self._lib)
        return z


class Autoencoder(ModelHandle):
    """``Autoencoder`` (autoencoder.py:27-109) on the ``pf_autoenc`` plans.  ``x3="f16"``: the model lives in libpfhip_f16.so, whose
    split mode is "f16x3".  Weights (ModelHandle): the reference state_dict (``encoder.*``, ``decoder.*``, ``quant_conv.*``,
    ``post_quant_conv.*``; ``loss.*`` is dropped).  Any image whose sides are multiples of ``cfg.downscale`` and whose latent holds a
    multiple of 64 pixels, at most 1024, runs."""
    PREFIX = "pf_autoenc"

    def __init__(self, cfg: AutoencoderConfig = AutoencoderConfig(), device: Optional[torch.device] = None, x3: Optional[str] = None):
        self.cfg = cfg
        self._split_name = "f16x3" if x3 == "f16" else "bf16x3"
        c = _lib.AutoencCfg()
        c.in_channels, c.out_channels, c.channels, c.n_levels = cfg.in_channels, cfg.out_channels, cfg.channels, len(cfg.channel_multipliers)
        for i, m in enumerate(cfg.channel_multipliers):
            c.channel_multipliers[i] = m
        c.n_resnet_blocks, c.z_channels, c.emb_channels = cfg.n_resnet_blocks, cfg.z_channels, cfg.emb_channels
        super().__init__(_lib.load(x3), C.byref(c), device=device)

    # ---- plans (no GPU needed) ----
    def encode_workspace_bytes(self, batch: int, h: int, w: int) -> int:
        return int(self._lib.pf_autoenc_encode_workspace_bytes(self._h, batch, h, w))

    def decode_workspace_bytes(self, batch: int, zh: int, zw: int) -> int:
        return int(self._lib.pf_autoenc_decode_workspace_bytes(self._h, batch, zh, zw))

    def encode_launches(self, batch: int, h: int, w: int) -> int:
        return int(self._lib.pf_autoenc_encode_launches(self._h, batch, h, w))

    def decode_launches(self, batch: int, zh: int, zw: int) -> int:
        return int(self._lib.pf_autoenc_decode_launches(self._h, batch, zh, zw))

    def encode_flops(self, batch: int, h: int, w: int) -> float:
        return float(self._lib.pf_autoenc_encode_flops(self._h, batch, h, w))

    def decode_flops(self, batch: int, zh: int, zw: int) -> float:
        return float(self._lib.pf_autoenc_decode_flops(self._h, batch, zh, zw))

    # ---- forward ----
    def _image(self, img: torch.Tensor, what: str) -> torch.Tensor:
        if self._blob_dev is None:
            raise RuntimeError(f"Autoencoder.{what}: weights not loaded")
        if img.dim() != 4 or img.shape[1] != self.cfg.in_channels:
            raise RuntimeError(f"Autoencoder.{what}: input {tuple(img.shape)}, expected [B,{self.cfg.in_channels},H,W]")
        return img.to(self.device).contiguous().float()

    def _encode(self, img: torch.Tensor, scale: float, what: str, z: bool, noise=None, seed=0, stream_id=0, offset=0):
        img = self._image(img, what)
        B, _, H, W = img.shape
        f = self.cfg.downscale
        nbytes = self.encode_workspace_bytes(B, H, W)
        if nbytes == 0:
            raise RuntimeError(f"Autoencoder.{what}: an image of {H}x{W} does not fit this model (sides multiples of {f}, latent pixels a "
                               "multiple of 64 and at most 1024)")
        ws = self.workspace_for(nbytes, self.device)
        shape = (B, self.cfg.emb_channels, H // f, W // f)
        mean = torch.empty(shape, dtype=torch.float32, device=self.device)
        log_var = torch.empty_like(mean)
        zt = torch.empty_like(mean) if z else None
        if noise is not None:
            if tuple(noise.shape) != shape:
                raise RuntimeError(f"Autoencoder.{what}: noise {tuple(noise.shape)}, expected {shape}")
            noise = noise.to(device=self.device, dtype=torch.float32).contiguous()
        self._check(self._lib.pf_autoenc_encode(self._h, img.data_ptr(), B, H, W, float(scale), _lib.ptr(noise), int(seed), int(stream_id),
                                                int(offset), _lib.ptr(zt), mean.data_ptr(), log_var.data_ptr(), ws.data_ptr(), ws.numel(),
                                                _lib.current_stream()), "pf_autoenc_encode")
        return GaussianDistribution(mean, log_var, scale, self._lib), zt

    def encode(self, img: torch.Tensor, scale: float = 1.0) -> GaussianDistribution:
        """``Autoencoder.encode``: the posterior of ``img`` [B, in_channels, H, W]."""
        return self._encode(img, scale, "encode", False)[0]

    def encode_sample(self, img: torch.Tensor, scale: float = 1.0, noise: Optional[torch.Tensor] = None, seed: int = 0, stream_id: int = 0,
                      offset: int = 0) -> Tuple[torch.Tensor, GaussianDistribution]:
        """``scale * encode(img).sample()`` with the sample drawn by the encoder's last launch (bit-identical to
        ``encode(img, scale).sample(...)`` with the same arguments); returns (z, posterior)."""
        dist, z = self._encode(img, scale, "encode_sample", True, noise, seed, stream_id, offset)
        return z, dist

    def decode(self, z: torch.Tensor, scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``Autoencoder.decode(z / scale)``: z [B, emb_channels, h, w] -> image [B, out_channels, h * downscale, w * downscale]."""
        if self._blob_dev is None:
            raise RuntimeError("Autoencoder.decode: weights not loaded")
        if z.dim() != 4 or z.shape[1] != self.cfg.emb_channels:
            raise RuntimeError(f"Autoencoder.decode: z {tuple(z.shape)}, expected [B,{self.cfg.emb_channels},h,w]")
        z = z.to(self.device).contiguous().float()
        B, _, zh, zw = z.shape
        f = self.cfg.downscale
        nbytes = self.decode_workspace_bytes(B, zh, zw)
        if nbytes == 0:
            raise RuntimeError(f"Autoencoder.decode: a latent of {zh}x{zw} does not fit this model (pixels a multiple of 64, at most 1024)")
        ws = self.workspace_for(nbytes, self.device)
        if out is None:
            out = torch.empty((B, self.cfg.out_channels, zh * f, zw * f), dtype=torch.float32, device=self.device)
        self._check(self._lib.pf_autoenc_decode(self._h, z.data_ptr(), B, zh, zw, float(scale), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                _lib.current_stream()), "pf_autoenc_decode")
        return out

    def forward(self, input: torch.Tensor, sample_posterior: bool = True, noise: Optional[torch.Tensor] = None, seed: int = 0,
                stream_id: int = 0, offset: int = 0) -> Tuple[torch.Tensor, GaussianDistribution]:
        """``Autoencoder.forward`` (autoencoder.py:81-88): (decode(posterior.sample()), posterior)."""
        if not sample_posterior:
            raise RuntimeError("Autoencoder.forward: sample_posterior=False is not implemented by the reference either")
        z, posterior = self.encode_sample(input, 1.0, noise, seed, stream_id, offset)
        return self.decode(z), posterior

    __call__ = forward

    def get_loss_dict(self, batch, step):
        raise NotImplementedError("Autoencoder.get_loss_dict is training code (LPIPS + discriminator); this library runs inference only")

    def set_precision(self, mode: str):
        """"f32" (exact fp32) or this model's split mode ("bf16x3", or "f16x3" for a model constructed with x3="f16")."""
        if mode not in ("f32", self._split_name):
            raise ValueError(f"precision {mode!r}: this model supports 'f32' and {self._split_name!r}")
        self._check(self._lib.pf_autoenc_set_precision(self._h, 0 if mode == "f32" else 1), "pf_autoenc_set_precision")
        return self

    @property
    def precision(self) -> str:
        return ["f32", self._split_name][self._lib.pf_autoenc_get_precision(self._h)]


class Polyffusion_Autoencoder:
    """``models/model_autoencoder.py``: the trained model keeps the ``Autoencoder`` under ``autoencoder.``."""

    def __init__(self, autoencoder: Autoencoder):
        self.autoencoder = autoencoder

    @staticmethod
    def strip_prefix(state: Mapping[str, object], where: str = "checkpoint") -> "OrderedDict[str, object]":
        out: "OrderedDict[str, object]" = OrderedDict()
        for k, v in state.items():
            if not k.startswith(PREFIX):
                raise RuntimeError(f"{where}: unexpected key {k!r} in an autoencoder checkpoint")
            out[k[len(PREFIX):]] = v
        return out

    @classmethod
    def load_trained(cls, model_dir: str, cfg: Optional[AutoencoderConfig] = None, x3: Optional[str] = None) -> "Polyffusion_Autoencoder":
        """``load_trained`` (model_autoencoder.py:14-19): ``<model_dir>/weights.pt`` holds ``{"model": state_dict}``, read with the
        restricted unpickler; the architecture comes from ``cfg``, else ``<model_dir>/params.yaml``, else ``params/autoencoder.yaml``."""
        from .checkpoint import load_checkpoint
        from .params import load_autoencoder_params
        path = os.path.join(model_dir, "weights.pt")
        state, _ = load_checkpoint(path)
        if cfg is None:
            pfile = os.path.join(model_dir, "params.yaml")
            cfg = AutoencoderConfig.from_params(load_autoencoder_params(pfile) if os.path.exists(pfile) else AUTOENCODER_PARAMS)
        ae = Autoencoder(cfg, x3=x3)
        ae.load_state_dict(cls.strip_prefix(state, path))
        return cls(ae)

    def get_loss_dict(self, batch, step):
        return self.autoencoder.get_loss_dict(batch, step)
