"""Host mirror of the reference denoiser objects, backed by libpfhip.so.

``UNetModel`` keeps the reference constructor surface (keyword names of
``stable_diffusion/model/unet.py:35-47``), ingests weights by the reference
``state_dict`` key names and evaluates ``forward(x, t, cond)`` with the same
argument meaning (``unet.py:171-196``) - but every FLOP runs in the HIP kernels of
``csrc/``.  ``LatentDiffusion`` mirrors ``stable_diffusion/latent_diffusion.py``
(schedule at :90-103, ``forward`` at :138-147) for the attributes the samplers use.

PyTorch is plumbing here: device buffers, the current stream and (for multi-GPU)
the RCCL broadcast of the packed weight blob.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional, Tuple

import torch

from . import _lib, _steps
from ._handle import ModelHandle
from .arch import UNetConfig


class UNetModel(ModelHandle):
    PREFIX = "pf_unet"

    def __init__(self, *, in_channels: int, out_channels: int, channels: int, n_res_blocks: int,
                 attention_levels: Iterable[int], channel_multipliers: Iterable[int], n_heads: int,
                 tf_layers: int = 1, d_cond: int = 768, img_h: int = 128, img_w: int = 128,
                 device: Optional[torch.device] = None, x3: Optional[str] = None):
        """`x3`: which build of the library this model lives in - None: the process default (libpfhip.so, bf16 pieces, unless PF_X3
        says otherwise); "f16": libpfhip_f16.so, whose split mode is "f16x3" (include/pfhip.h pf_x3_element).  Weights are packed by, and
        for, that library; a model never changes library."""
        self.cfg = UNetConfig(in_channels, out_channels, channels, n_res_blocks, tuple(attention_levels),
                              tuple(channel_multipliers), n_heads, tf_layers, d_cond)
        self.img_h, self.img_w = int(img_h), int(img_w)
        self.channels = channels
        self.x3 = x3
        # name of the split mode: "f16x3" for a model asked to live in the fp16 build; a model in the process default keeps "bf16x3"
        # (also under PF_X3=f16, which exists to run unchanged callers against the other build)
        self._split_name = "f16x3" if x3 == "f16" else "bf16x3"
        c = _lib.UNetCfg()
        c.in_channels, c.out_channels, c.channels, c.n_res_blocks = in_channels, out_channels, channels, n_res_blocks
        c.n_attention_levels = len(self.cfg.attention_levels)
        for i, v in enumerate(self.cfg.attention_levels):
            c.attention_levels[i] = v
        c.n_levels = len(self.cfg.channel_multipliers)
        for i, v in enumerate(self.cfg.channel_multipliers):
            c.channel_multipliers[i] = v
        c.n_heads, c.tf_layers, c.d_cond, c.img_h, c.img_w = n_heads, tf_layers, d_cond, self.img_h, self.img_w
        super().__init__(_lib.load(x3), C.byref(c), device=device)
        self._amax: Optional[torch.Tensor] = None      # range telemetry word (track_absmax)
        self._ws_key = (0, 0, 0)

    # (weights: ModelHandle - state_dict keys relative to ``eps_model``)
    def eval(self):
        return self

    # ---- forward --------------------------------------------------------------------------------
    @staticmethod
    def _groups(shared_x) -> int:
        """``shared_x`` as a group count: 0 for a plain forward, ``True`` = 2 (classifier-free guidance), 2 or 3 as given."""
        if not shared_x:                # False, None, or a group count of 0 as this method returns it
            return 0
        g = 2 if shared_x is True else int(shared_x)
        if g not in (2, 3):
            raise ValueError(f"shared_x={shared_x!r}: the shared-prefix plan runs 2 or 3 stacked evaluations (True means 2)")
        return g

    def workspace(self, batch: int, n_cond: int, shared_x=False) -> torch.Tensor:
        # tile choice (and buffer sizes) depend on the arithmetic mode and on the plan options; the shared-prefix guidance plan has a layout of
        # its own per group count
        g = self._groups(shared_x)
        key = (batch, n_cond, g, self._lib.pf_unet_get_precision(self._h)) + self.options_key()
        if self._ws is None or self._ws_key != key:
            nbytes = self._lib.pf_unet_workspace_bytes_cfgn(self._h, batch, g, n_cond) if g else self._lib.pf_unet_workspace_bytes(self._h, batch, n_cond)
            self.workspace_for(nbytes, self.device)
            self._ws_key = key
        return self._ws

    # ---- step-invariant prefix (hoisted out of a sampler's loop; include/pfhip.h pf_unet_prepared) ---------------
    def prepare_time(self, n_rows: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[n_rows, W] table: row r = the additive time biases of every ResBlock for time-step VALUE r - what ``forward`` derives
        from ``t == r`` through ``time_embed`` and the ``emb_layers`` (unet.py:181-182, 286-289).  Depends on the weights only."""
        if self._blob_dev is None:
            raise RuntimeError("UNetModel.prepare_time: weights not loaded")
        w = int(self._lib.pf_unet_time_bias_width(self._h))
        if out is None:
            out = torch.empty(n_rows, w, dtype=torch.float32, device=self.device)
        assert out.shape == (n_rows, w) and out.is_contiguous()
        scratch = torch.empty(n_rows * 4 * self.cfg.channels, dtype=torch.float32, device=self.device)
        self._check(self._lib.pf_unet_prepare_time(self._h, n_rows, out.data_ptr(), scratch.data_ptr(), scratch.numel() * 4,
                                                  _lib.current_stream()), "pf_unet_prepare_time")
        return out

    def prepare_cond(self, cond: torch.Tensor, out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """[B, W] collapsed cross-attention biases ``to_out(to_v(cond))`` of every transformer block for ONE context token
        (unet_attention.py:186-212 with softmax over a single key); ``None`` when ``cond`` has several tokens (general path)."""
        if self._blob_dev is None:
            raise RuntimeError("UNetModel.prepare_cond: weights not loaded")
        w = int(self._lib.pf_unet_cross_bias_width(self._h))
        if cond.dim() != 3 or cond.shape[1] != 1 or w == 0:
            return None
        if cond.shape[2] != self.cfg.d_cond:
            raise RuntimeError(f"UNetModel.prepare_cond: cond has shape {tuple(cond.shape)}, expected [B,1,{self.cfg.d_cond}]")
        cond = cond.contiguous().float()
        B = cond.shape[0]
        if out is None:
            out = torch.empty(B, w, dtype=torch.float32, device=cond.device)
        assert out.shape == (B, w) and out.is_contiguous()
        scratch = torch.empty(B * w, dtype=torch.float32, device=cond.device)
        self._check(self._lib.pf_unet_prepare_cond(self._h, cond.data_ptr(), B, out.data_ptr(), scratch.data_ptr(), scratch.numel() * 4,
                                                  _lib.current_stream()), "pf_unet_prepare_cond")
        return out

    def forward(self, x: torch.Tensor, time_steps: torch.Tensor, cond: torch.Tensor, out: Optional[torch.Tensor] = None, *,
                time_table: Optional[torch.Tensor] = None, cross_bias: Optional[torch.Tensor] = None, check_t: bool = False,
                shared_x=False):
        """``time_table`` / ``cross_bias``: results of ``prepare_time`` / ``prepare_cond(cond)`` - the caller vouches that they
        belong to these weights and this ``cond``; either may be ``None`` (computed here).  Bit-identical either way.
        ``shared_x=True`` - classifier-free guidance (``sampler/__init__.py:69-74``): ``x`` holds B samples while ``time_steps`` and
        ``cond`` hold the 2B rows of ``cat([t, t])`` / ``cat([uncond_cond, cond])``; the result equals ``forward(cat([x, x]), ...)`` up to
        tile-choice rounding, but everything in front of the first transformer block - where the two halves cannot differ - is computed
        once (``pf_unet_forward_cfg``).  PRECONDITION: ``time_steps[:B] == time_steps[B:]`` (the shared prefix uses the first half's rows;
        verified under ``check_t``).  ``shared_x=3``: the same over three groups - ``time_steps`` and ``cond`` hold the 3B rows of a dual-guidance
        evaluation, ``cat([uncond_cond, partial, cond])`` (``pf_unet_forward_cfgn``); every group carries the same ``t``.
        The prepared path is valid for ``0 <= t < time_table.shape[0]`` only; ``check_t=True`` verifies that (one device->host
        sync - the samplers, whose t values are rows of a host-built table, do not ask for it)."""
        if self._blob_dev is None:
            raise RuntimeError("UNetModel.forward: weights not loaded")
        G = self._groups(shared_x)
        B = x.shape[0] * (G or 1)
        if tuple(x.shape[1:]) != (self.cfg.in_channels, self.img_h, self.img_w):
            raise RuntimeError(f"UNetModel.forward: x has shape {tuple(x.shape)}, expected [B,{self.cfg.in_channels},{self.img_h},{self.img_w}]")
        if cond.dim() != 3 or cond.shape[0] != B or cond.shape[2] != self.cfg.d_cond:
            raise RuntimeError(f"UNetModel.forward: cond has shape {tuple(cond.shape)}, expected [{f'{G}B' if G else 'B'},n_cond,{self.cfg.d_cond}]")
        if time_steps.shape[0] != B:
            raise RuntimeError(f"UNetModel.forward: {time_steps.shape[0]} time steps for {B} condition rows")
        x = x.contiguous().float()
        cond = cond.contiguous().float()
        t = time_steps.to(torch.int64).contiguous()
        if G and check_t and not all(torch.equal(t[: B // G], t[g * (B // G): (g + 1) * (B // G)]) for g in range(1, G)):
            # the shared prefix is evaluated once, with the first group's time rows: all groups of a guidance evaluation carry the same t
            raise RuntimeError(f"UNetModel.forward(shared_x={shared_x!r}): the {G} groups of time_steps must be equal "
                               "(the evaluations of one guidance step share everything in front of the first transformer block)")
        n_cond = cond.shape[1]
        ws = self.workspace(B, n_cond, G)
        if out is None:
            out = torch.empty(B, self.cfg.out_channels, self.img_h, self.img_w, dtype=torch.float32, device=x.device)
        prep = None
        if time_table is not None or cross_bias is not None:
            prep = _lib.UNetPrepared()
            if time_table is not None:
                assert time_table.dtype == torch.float32 and time_table.is_contiguous() and time_table.device == x.device
                # the kernels clamp a row index into the table for memory safety only: a t outside it would silently read the
                # wrong row.  Callers that hold t on the host say so (check_t); the samplers' loops index a [n_steps+1]-row table
                # with values < n_steps + 1 by construction.
                if check_t:
                    lo, hi = int(t.min()), int(t.max())
                    if lo < 0 or hi >= time_table.shape[0]:
                        raise RuntimeError(f"UNetModel.forward: time step {lo if lo < 0 else hi} outside the prepared table "
                                           f"({time_table.shape[0]} rows)")
                prep.time_table, prep.n_time_rows = time_table.data_ptr(), time_table.shape[0]
            if cross_bias is not None:
                assert n_cond == 1 and cross_bias.shape[0] == B and cross_bias.is_contiguous() and cross_bias.device == x.device
                prep.cross_bias = cross_bias.data_ptr()
        args = (None if prep is None else C.byref(prep), out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream())
        if G:
            rc = self._lib.pf_unet_forward_cfgn(self._h, x.data_ptr(), t.data_ptr(), cond.data_ptr(), B, G, n_cond, *args)
        else:
            rc = self._lib.pf_unet_forward_prepared(self._h, x.data_ptr(), t.data_ptr(), cond.data_ptr(), B, n_cond, *args)
        self._check(rc, "pf_unet_forward")
        return out

    __call__ = forward

    # ---- arithmetic mode ------------------------------------------------------------------------
    def set_precision(self, mode: str):
        """"f32" (exact fp32 MFMA) or this model's split mode: "bf16x3" (error-compensated split on the bf16 matrix pipe), or "f16x3"
        (the same on the fp16 pipe) for a model constructed with x3="f16"."""
        if mode not in ("f32", self._split_name):
            raise ValueError(f"precision {mode!r}: this model supports 'f32' and {self._split_name!r} "
                             "(the split element type is chosen at construction: UNetModel(..., x3='f16') for f16x3)")
        code = 0 if mode == "f32" else 1
        self._check(self._lib.pf_unet_set_precision(self._h, code), "pf_unet_set_precision")
        return self

    @property
    def split_mode(self) -> str:
        """Name of this model's split-precision mode: "bf16x3", or "f16x3" for a model constructed with x3="f16"."""
        return self._split_name

    @property
    def precision(self) -> str:
        return ["f32", self._split_name][self._lib.pf_unet_get_precision(self._h)]

    # ---- plan options (which of two equivalent kernel forms the plan launches; include/pfhip.h PF_OPT_*) --------
    _OPTS = {"mlp_fused": _lib.OPT_MLP_FUSED, "attn_wide": _lib.OPT_ATTN_WIDE, "conv_t16": _lib.OPT_CONV_T16, "conv_pp": _lib.OPT_CONV_PP, "conv_wino": _lib.OPT_CONV_WINO}

    def set_option(self, name: str, value: Optional[bool]):
        """``None`` = automatic (the default), ``False`` / ``True`` = never / always (where the form exists)."""
        v = _lib.OPT_AUTO if value is None else int(bool(value))
        self._check(self._lib.pf_unet_set_option(self._h, self._OPTS[name], v), "pf_unet_set_option")
        return self

    def get_option(self, name: str) -> Optional[bool]:
        v = self._lib.pf_unet_get_option(self._h, self._OPTS[name])
        return None if v < 0 else bool(v)

    def options_key(self) -> tuple:
        """Every plan option's current setting: part of the key of anything that bakes the launch sequence in (workspace, graphs)."""
        return tuple(self._lib.pf_unet_get_option(self._h, o) for o in range(_lib.OPT_COUNT)) + (self._amax is not None,)

    # ---- range telemetry (include/pfhip.h pf_unet_track_absmax) -----------------------------------
    def track_absmax(self, on: bool = True):
        """While on, every forward max-combines the largest |value| its layers store into one device word (reset here)."""
        dev = self._blob_dev.device if self._blob_dev is not None else torch.device("cuda")
        self._amax = torch.zeros(1, dtype=torch.int32, device=dev) if on else None
        self._check(self._lib.pf_unet_track_absmax(self._h, None if self._amax is None else self._amax.data_ptr()), "pf_unet_track_absmax")
        self._ws = None          # the plan changes (fused launches run as their chains while tracking)
        return self

    def read_absmax(self) -> float:
        """Largest |stored value| since track_absmax(True) (nan / inf if one was stored); 65504 / it = the fp16 split's headroom."""
        if self._amax is None:
            raise RuntimeError("read_absmax: telemetry is off (track_absmax(True) first)")
        return float(self._amax.view(torch.float32).item())

    # ---- profiling ------------------------------------------------------------------------------
    def set_profiling(self, on: bool):
        self._check(self._lib.pf_unet_set_profiling(self._h, int(on)))

    def read_profile(self) -> List[Tuple[int, float, float]]:
        cap = 4096
        kind = (C.c_int * cap)()
        ms = (C.c_float * cap)()
        fl = (C.c_double * cap)()
        n = self._check(self._lib.pf_unet_profile_read(self._h, kind, ms, fl, cap))
        return [(kind[i], ms[i], fl[i]) for i in range(n)]

    def read_profile_direct(self) -> List[float]:
        """Per launch of the last profiled forward: the operation count of the layer's DIRECT form (= read_profile()'s count except for
        Winograd launches, which execute 16 / 36 of it)."""
        cap = 4096
        fl = (C.c_double * cap)()
        n = self._check(self._lib.pf_unet_profile_read_direct(self._h, fl, cap))
        return [fl[i] for i in range(n)]

    def n_launches(self, batch: int, n_cond: int = 1, prepared: bool = False, shared_x=False) -> int:
        g = self._groups(shared_x)
        if g:            # batch = the 2B (3B) rows of a guidance evaluation
            return int(self._lib.pf_unet_n_launches_cfgn(self._h, batch, g, n_cond, int(prepared), int(prepared)))
        if prepared:
            return int(self._lib.pf_unet_n_launches_prepared(self._h, batch, n_cond, 1, 1))
        return int(self._lib.pf_unet_n_launches(self._h, batch, n_cond))


class LatentDiffusion:
    """Mirror of ``stable_diffusion/latent_diffusion.py:LatentDiffusion``.  ``autoencoder``: None (``inference_sdf.py:537``, the
    Polyffusion path: latents are the images) or an ``autoencoder.Autoencoder``, which ``autoencoder_encode`` / ``autoencoder_decode``
    then call with ``latent_scaling_factor``."""

    def __init__(self, unet_model: UNetModel, autoencoder=None, latent_scaling_factor: float = 0.18215,
                 n_steps: int = 1000, linear_start: float = 0.00085, linear_end: float = 0.012):
        if autoencoder is not None and not (hasattr(autoencoder, "encode_sample") and hasattr(autoencoder, "decode")):
            raise TypeError("LatentDiffusion: autoencoder must be a polyffusion_amd.autoencoder.Autoencoder (or None)")
        self.eps_model = unet_model
        self.first_stage_model = autoencoder
        self.latent_scaling_factor = latent_scaling_factor
        self.n_steps = n_steps
        # sqrt-linear schedule computed in float64 then cast (latent_diffusion.py:90-103)
        beta = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, n_steps, dtype=torch.float64) ** 2
        alpha = 1.0 - beta
        alpha_bar = torch.cumprod(alpha, dim=0)
        self.alpha = alpha.to(torch.float32)
        self.beta = beta.to(torch.float32)
        self.alpha_bar = alpha_bar.to(torch.float32)
        self.sigma2 = self.beta

    @property
    def device(self):
        return self.eps_model.device

    def eval(self):
        return self

    def autoencoder_encode(self, image: torch.Tensor, noise: Optional[torch.Tensor] = None, seed: int = 0, stream_id: int = 0,
                           offset: int = 0) -> torch.Tensor:
        """``latent_scaling_factor * first_stage_model.encode(image).sample()`` (latent_diffusion.py:112-125); the image itself without
        an autoencoder.  The sample's noise: as ``GaussianDistribution.sample``."""
        if self.first_stage_model is None:
            return image
        return self.first_stage_model.encode_sample(image, self.latent_scaling_factor, noise, seed, stream_id, offset)[0]

    def autoencoder_decode(self, z: torch.Tensor) -> torch.Tensor:
        """``first_stage_model.decode(z / latent_scaling_factor)`` (latent_diffusion.py:127-136); ``z`` itself without an autoencoder."""
        if self.first_stage_model is None:
            return z
        return self.first_stage_model.decode(z, self.latent_scaling_factor)

    # ---- the training objective, forward only (latent_diffusion.py:149-177, 203-240) -----------------------------------------------
    def _tables(self, device):
        """``alpha_bar ** 0.5`` / ``(1 - alpha_bar) ** 0.5`` in float32 on ``device`` (built once per device)."""
        key = str(device)
        cache = self.__dict__.setdefault("_sqrt_tables", {})
        if key not in cache:
            cache[key] = _steps.sqrt_tables(self.alpha_bar, device)
        return cache[key]

    def x0_threshold_table(self, device) -> torch.Tensor:
        """The coefficient table of ``pf_x0_threshold`` (``_steps.x0_threshold_table``) on ``device`` (built once per device)."""
        key = str(device)
        cache = self.__dict__.setdefault("_x0t_tables", {})
        if key not in cache:
            cache[key] = _steps.x0_threshold_table(self.alpha_bar).to(device)
        return cache[key]

    def q_xt_x0(self, x0: torch.Tensor, t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(mean, var)`` of q(x_t | x_0) (latent_diffusion.py:149-161): ``alpha_bar[t] ** 0.5 * x0`` and ``1 - alpha_bar[t]``, the
        latter shaped ``[B, 1, 1, 1]``.  An accessor kept for parity (two torch operations); ``q_sample`` / ``loss`` run the kernel."""
        ab = self.alpha_bar.to(x0.device)[t.to(x0.device)].reshape(-1, *([1] * (x0.dim() - 1)))
        return ab ** 0.5 * x0, 1 - ab

    def q_sample(self, x0: torch.Tensor, t, eps: Optional[torch.Tensor] = None, *, seed: int = 0, draw: int = 0,
                 elem_offset: int = 0) -> torch.Tensor:
        """``alpha_bar[t] ** 0.5 * x0 + (1 - alpha_bar[t]) ** 0.5 * eps`` with one ``t`` per sample (latent_diffusion.py:163-177), as one
        ``pf_qsample_rows`` launch.  ``eps=None``: draw ``draw`` of the library's generator under ``seed``, made inside the kernel."""
        x0 = x0.contiguous().float()
        t = _steps.time_steps(t, x0.shape[0], self.n_steps, 0, x0.device)
        sa, sb = self._tables(x0.device)
        if eps is not None:
            return _steps.qsample_rows(self.eps_model._lib, x0, t, sa, sb, noise=eps.to(device=x0.device, dtype=torch.float32).contiguous())
        return _steps.qsample_rows(self.eps_model._lib, x0, t, sa, sb, rng=(seed, draw, elem_offset))

    def loss_rows(self, x0: torch.Tensor, cond: torch.Tensor, noise: Optional[torch.Tensor] = None,
                  cond_concat: Optional[torch.Tensor] = None, *, t=None, seed: int = 0, draw: int = 0, elem_offset: int = 0,
                  return_t: bool = False):
        """The per-sample mean of ``(noise - eps_theta) ** 2`` as float64 ``[B]``; ``loss`` is its mean.  See ``loss``."""
        B = x0.shape[0]
        dev = self.device
        t = _steps.time_steps(t, B, self.n_steps, seed, dev)
        x0 = x0.to(dev)
        if self.first_stage_model is not None:
            # the posterior sample's noise: a draw of its own under the same seed, keyed by the same global element index
            x0 = self.autoencoder_encode(x0, seed=seed, stream_id=(1 << 32) + int(draw), offset=elem_offset)
        cond = cond.to(dev)
        if cond_concat is not None:
            cc = cond_concat.to(device=dev, dtype=torch.float32)
            predict = lambda xt: self.eps_model(torch.cat([xt, cc], dim=1), t, cond)      # latent_diffusion.py:229-232
        else:
            predict = lambda xt: self.eps_model(xt, t, cond)
        rows = _steps.diffusion_loss_rows(self.eps_model._lib, x0, t, self._tables(dev), predict, noise=noise,
                                          rng=(seed, draw, elem_offset))[0]
        return (rows, t) if return_t else rows

    def loss(self, x0: torch.Tensor, cond: torch.Tensor, noise: Optional[torch.Tensor] = None,
             cond_concat: Optional[torch.Tensor] = None, *, t=None, seed: int = 0, draw: int = 0, elem_offset: int = 0) -> torch.Tensor:
        """``F.mse_loss(noise, eps_model(q_sample(x0, t, noise), t, cond))`` (latent_diffusion.py:203-240) as a 0-d float32 tensor.
        ``t=None``: ``randint(0, n_steps, (B,))`` from a CPU ``torch.Generator`` seeded with ``seed`` (the reference draws it on the
        device from the global generator, which nothing can pin).  ``noise=None``: draw ``draw`` of the library's counter-based
        generator under ``seed``; element ``i`` of ``x0`` uses global element ``elem_offset + i``, so a batch split into several calls
        sees the noise of the unsplit batch.  The noise is then made inside ``pf_qsample_rows`` and made again inside ``pf_mse_rows``:
        it never exists as a tensor.  ``cond_concat`` is concatenated to ``x_t`` on the channel axis in front of the UNet (:229-232).
        With a first-stage model ``x0`` first goes through ``autoencoder_encode``."""
        return self.loss_rows(x0, cond, noise, cond_concat, t=t, seed=seed, draw=draw, elem_offset=elem_offset).mean().float()

    supports_shared_x = True     # forward(..., shared_x=True): the guidance evaluation with its condition-independent prefix computed once

    def forward(self, x: torch.Tensor, t: torch.Tensor, context: torch.Tensor, **prepared):
        return self.eps_model(x, t, context, **prepared)

    __call__ = forward
