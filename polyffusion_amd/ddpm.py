"""The vanilla DDPM model of the reference (``main.py --model ddpm``) on the HIP path.

Mirrors ``ddpm/unet.py`` (``UNet``), ``ddpm/__init__.py`` (``DenoiseDiffusion``), ``models/model_ddpm.py`` (``load_trained``) and the
``Configs`` sampler of ``inference.py``.  The noise predictor is the ``pf_ddpm`` plan of ``libpfhip.so`` (``csrc/ddpm_unet.hip``);
the reverse step is the library's ``pf_ddpm_step`` kernel with ``c_x0 = 1, c_xt = 0, sigma = sqrt(beta)``, ``q_sample`` its ``pf_axpby``
(both launched through ``_steps``, which the SDF samplers share).  PyTorch holds the buffers and builds the schedule tables on the host,
in float32, as the reference does on the CPU.

The model's parameters (``params/ddpm.yaml``) live here as ``DDPM_PARAMS``, not in ``params.PRESETS``: that table feeds the SDF CLI.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict
from dataclasses import dataclass
from typing import Callable, Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib, _steps
from ._handle import ModelHandle

# params/ddpm.yaml of the reference (the keys the sampler reads)
DDPM_PARAMS = {
    "model_name": "ddpm", "batch_size": 16, "image_channels": 2, "image_size_h": 128, "image_size_w": 128, "n_channels": 64,
    "channel_multipliers": [1, 2, 2, 4], "is_attention": [False, False, False, True], "n_steps": 1000,
}
PREFIX = "ddpm.eps_model."


@dataclass(frozen=True)
class DDPMConfig:
    """Constructor arguments of the reference ``UNet`` (unet.py:296-303) plus the image size."""
    image_channels: int = 2
    n_channels: int = 64
    ch_mults: Tuple[int, ...] = (1, 2, 2, 4)
    is_attn: Tuple[bool, ...] = (False, False, False, True)
    n_blocks: int = 2
    img_h: int = 128
    img_w: int = 128

    @classmethod
    def from_params(cls, p: Mapping) -> "DDPMConfig":
        return cls(int(p["image_channels"]), int(p["n_channels"]), tuple(int(v) for v in p["channel_multipliers"]),
                   tuple(bool(v) for v in p["is_attention"]), 2, int(p["image_size_h"]), int(p["image_size_w"]))


def ddpm_param_shapes(cfg: DDPMConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """The reference UNet's state_dict keys and shapes (relative to ``eps_model.``), walked as ``UNet.__init__`` builds it
    (unet.py:352-392).  ``pf_ddpm_param_info`` lists the same table."""
    out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    n, d_t = cfg.n_channels, 4 * cfg.n_channels
    out["image_proj.weight"] = (n, cfg.image_channels, 3, 3)
    out["image_proj.bias"] = (n,)
    out["time_emb.lin1.weight"] = (d_t, d_t // 4)
    out["time_emb.lin1.bias"] = (d_t,)
    out["time_emb.lin2.weight"] = (d_t, d_t)
    out["time_emb.lin2.bias"] = (d_t,)

    def res(p, ci, co):
        out[p + ".norm1.weight"] = (ci,); out[p + ".norm1.bias"] = (ci,)
        out[p + ".conv1.weight"] = (co, ci, 3, 3); out[p + ".conv1.bias"] = (co,)
        out[p + ".norm2.weight"] = (co,); out[p + ".norm2.bias"] = (co,)
        out[p + ".conv2.weight"] = (co, co, 3, 3); out[p + ".conv2.bias"] = (co,)
        if ci != co:
            out[p + ".shortcut.weight"] = (co, ci, 1, 1); out[p + ".shortcut.bias"] = (co,)
        out[p + ".time_emb.weight"] = (co, d_t); out[p + ".time_emb.bias"] = (co,)

    def attn(p, c):
        out[p + ".norm.weight"] = (c,); out[p + ".norm.bias"] = (c,)
        out[p + ".projection.weight"] = (3 * c, c); out[p + ".projection.bias"] = (3 * c,)
        out[p + ".output.weight"] = (c, c); out[p + ".output.bias"] = (c,)

    L = len(cfg.ch_mults)
    i_ch = o_ch = n
    m = 0
    for i in range(L):
        o_ch = i_ch * cfg.ch_mults[i]
        for _ in range(cfg.n_blocks):
            res(f"down.{m}.res", i_ch, o_ch)
            if cfg.is_attn[i]:
                attn(f"down.{m}.attn", o_ch)
            i_ch = o_ch
            m += 1
        if i < L - 1:
            out[f"down.{m}.conv.weight"] = (i_ch, i_ch, 3, 3); out[f"down.{m}.conv.bias"] = (i_ch,)
            m += 1
    res("middle.res1", o_ch, o_ch)
    attn("middle.attn", o_ch)
    res("middle.res2", o_ch, o_ch)
    i_ch = o_ch
    m = 0
    for i in reversed(range(L)):
        o_ch = i_ch
        for j in range(cfg.n_blocks + 1):
            if j == cfg.n_blocks:
                o_ch = i_ch // cfg.ch_mults[i]
            res(f"up.{m}.res", i_ch + o_ch, o_ch)
            if cfg.is_attn[i]:
                attn(f"up.{m}.attn", o_ch)
            m += 1
        i_ch = o_ch
        if i > 0:
            out[f"up.{m}.conv.weight"] = (i_ch, i_ch, 4, 4); out[f"up.{m}.conv.bias"] = (i_ch,)
            m += 1
    out["norm.weight"] = (n,); out["norm.bias"] = (n,)
    out["final.weight"] = (cfg.image_channels, n, 3, 3); out["final.bias"] = (cfg.image_channels,)
    return out


class DDPMUNet(ModelHandle):
    """``eps = UNet(x, t)`` (unet.py:398-421) on the ``pf_ddpm`` plan.  ``x3="f16"``: the model lives in libpfhip_f16.so, whose split
    mode is "f16x3".  Weights (ModelHandle): state_dict keys relative to ``eps_model.``."""
    PREFIX = "pf_ddpm"

    def __init__(self, cfg: DDPMConfig = DDPMConfig(), device: Optional[torch.device] = None, x3: Optional[str] = None):
        self.cfg = cfg
        self._split_name = "f16x3" if x3 == "f16" else "bf16x3"
        c = _lib.DDPMCfg()
        c.image_channels, c.n_channels, c.n_levels = cfg.image_channels, cfg.n_channels, len(cfg.ch_mults)
        for i, (mu, at) in enumerate(zip(cfg.ch_mults, cfg.is_attn)):
            c.ch_mults[i], c.is_attn[i] = mu, int(bool(at))
        c.n_blocks, c.img_h, c.img_w = cfg.n_blocks, cfg.img_h, cfg.img_w
        super().__init__(_lib.load(x3), C.byref(c), device=device)

    def workspace(self, batch: int) -> torch.Tensor:
        return self.workspace_for(self._lib.pf_ddpm_workspace_bytes(self._h, batch), self.device)

    def forward(self, x: torch.Tensor, t: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self._blob_dev is None:
            raise RuntimeError("DDPMUNet.forward: weights not loaded")
        c = self.cfg
        if tuple(x.shape[1:]) != (c.image_channels, c.img_h, c.img_w) or t.shape[0] != x.shape[0]:
            raise RuntimeError(f"DDPMUNet.forward: x {tuple(x.shape)} / t {tuple(t.shape)}, expected [B,{c.image_channels},{c.img_h},{c.img_w}] / [B]")
        B = x.shape[0]
        x = x.contiguous().float()
        t = t.to(device=x.device, dtype=torch.int64).contiguous()
        ws = self.workspace(B)
        if out is None:
            out = torch.empty_like(x)
        self._check(self._lib.pf_ddpm_forward(self._h, x.data_ptr(), t.data_ptr(), B, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _lib.current_stream()), "pf_ddpm_forward")
        return out

    __call__ = forward

    def set_precision(self, mode: str):
        """"f32" (exact fp32) or this model's split mode ("bf16x3", or "f16x3" for a model constructed with x3="f16")."""
        if mode not in ("f32", self._split_name):
            raise ValueError(f"precision {mode!r}: this model supports 'f32' and {self._split_name!r}")
        self._check(self._lib.pf_ddpm_set_precision(self._h, 0 if mode == "f32" else 1), "pf_ddpm_set_precision")
        return self

    @property
    def precision(self) -> str:
        return ["f32", self._split_name][self._lib.pf_ddpm_get_precision(self._h)]

    def n_launches(self, batch: int) -> int:
        return int(self._lib.pf_ddpm_n_launches(self._h, batch))

    def flops(self, batch: int) -> float:
        return float(self._lib.pf_ddpm_flops(self._h, batch))


def ddpm_tables(n_steps: int = 1000):
    """beta / alpha / alpha_bar exactly as ``DenoiseDiffusion.__init__`` builds them on the CPU (float32)."""
    beta = torch.linspace(0.0001, 0.02, n_steps)
    alpha = 1.0 - beta
    alpha_bar = torch.cumprod(alpha, dim=0)
    return beta, alpha, alpha_bar


NoiseFn = Callable[[Tuple[int, ...]], torch.Tensor]


class DenoiseDiffusion:
    """``ddpm/__init__.py`` with ``inference.py``'s ``Configs.sample``.  Noise: ``noise_fn(shape)`` when given (an injected tape, in the
    reference's draw order: the start, then one per step), otherwise the library's counter-based Philox stream keyed by ``seed`` (drawn
    inside the step kernel)."""

    def __init__(self, eps_model: DDPMUNet, n_steps: int = 1000, seed: int = 0, noise_fn: Optional[NoiseFn] = None):
        self.eps_model = eps_model
        self.n_steps = n_steps
        self.beta, self.alpha, self.alpha_bar = ddpm_tables(n_steps)
        self.sigma2 = self.beta
        self.seed = int(seed)
        self.noise_fn = noise_fn
        self._draws = 0
        self._lib = eps_model._lib

    def _randn(self, shape, device) -> torch.Tensor:
        return _steps.draw(self, shape, device)

    def _tables(self, device):
        """``alpha_bar ** 0.5`` / ``(1 - alpha_bar) ** 0.5`` in float32 on ``device`` (built once per device)."""
        key = str(device)
        cache = self.__dict__.setdefault("_sqrt_tables", {})
        if key not in cache:
            cache[key] = _steps.sqrt_tables(self.alpha_bar, device)
        return cache[key]

    def q_xt_x0(self, x0: torch.Tensor, t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(mean, var)`` of q(x_t | x_0) (ddpm/__init__.py:36-48): ``alpha_bar[t] ** 0.5 * x0`` and ``1 - alpha_bar[t]`` shaped
        ``[B, 1, 1, 1]``.  An accessor kept for parity (two torch operations); ``q_sample`` / ``loss`` run the kernels."""
        ab = self.alpha_bar.to(x0.device)[t.to(x0.device)].reshape(-1, *([1] * (x0.dim() - 1)))
        return ab ** 0.5 * x0, 1 - ab

    def q_sample(self, x0: torch.Tensor, t, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x_t = sqrt(alpha_bar_t) x0 + sqrt(1 - alpha_bar_t) eps (``q_xt_x0`` + ``q_sample``, ddpm/__init__.py:36-64).  ``t``: an
        ``int`` - one time step for the whole batch, ``pf_axpby`` - or a tensor of one time step per sample (``pf_qsample_rows``).
        ``eps=None``: the owner's next draw (``noise_fn``, else the library's generator: made inside the kernel on the tensor route)."""
        if not isinstance(t, torch.Tensor):
            ab = self.alpha_bar[t]
            return _steps.q_sample(self, x0.contiguous().float(), eps, ab ** 0.5, (1 - ab) ** 0.5)
        x0 = x0.contiguous().float()
        tt = _steps.time_steps(t, x0.shape[0], self.n_steps, 0, x0.device)
        sa, sb = self._tables(x0.device)
        if eps is None and self.noise_fn is not None:
            eps = _steps.draw(self, x0.shape, x0.device)
        if eps is not None:
            return _steps.qsample_rows(self._lib, x0, tt, sa, sb, noise=eps.to(device=x0.device, dtype=torch.float32).contiguous())
        out = _steps.qsample_rows(self._lib, x0, tt, sa, sb, rng=(self.seed, self._draws, 0))
        self._draws += 1
        return out

    def loss_rows(self, x0: torch.Tensor, noise: Optional[torch.Tensor] = None, *, t=None, seed: Optional[int] = None, draw: int = 0,
                  elem_offset: int = 0, return_t: bool = False):
        """The per-sample mean of ``(noise - eps_theta) ** 2`` as float64 ``[B]``; ``loss`` is its mean.  See ``loss``."""
        dev = self.eps_model.device
        seed = self.seed if seed is None else int(seed)
        t = _steps.time_steps(t, x0.shape[0], self.n_steps, seed, dev)
        rows = _steps.diffusion_loss_rows(self._lib, x0.to(dev), t, self._tables(dev), lambda xt: self.eps_model(xt, t), noise=noise,
                                          rng=(seed, draw, elem_offset))[0]
        return (rows, t) if return_t else rows

    def loss(self, x0: torch.Tensor, noise: Optional[torch.Tensor] = None, *, t=None, seed: Optional[int] = None, draw: int = 0,
             elem_offset: int = 0) -> torch.Tensor:
        """``F.mse_loss(noise, eps_model(q_sample(x0, t, noise), t))`` (ddpm/__init__.py:90-111) as a 0-d float32 tensor.  ``t=None``:
        ``randint(0, n_steps, (B,))`` from a CPU ``torch.Generator`` seeded with ``seed`` (default: the object's seed; the reference
        draws on the device from the global generator).  ``noise=None``: draw ``draw`` of the library's generator under ``seed``, keyed
        by the global element index ``elem_offset + i`` and made inside the two kernels - it never exists as a tensor."""
        return self.loss_rows(x0, noise, t=t, seed=seed, draw=draw, elem_offset=elem_offset).mean().float()

    def coef(self, t: int) -> "_lib.DdpmCoef":
        """``p_sample``'s mean = 1/sqrt(a) (x - (1-a)/sqrt(1-ab) eps), sigma = sqrt(beta) as the library's step coefficients."""
        a, ab, b = self.alpha[t], self.alpha_bar[t], self.beta[t]
        c = _lib.DdpmCoef()
        c.c_recip = float(1 / a ** 0.5)
        c.c_recipm1 = float(1 / a ** 0.5) * float((1 - a) / (1 - ab) ** 0.5)
        c.c_x0, c.c_xt, c.sigma = 1.0, 0.0, float(b ** 0.5)
        return c

    def p_sample(self, xt: torch.Tensor, t: int) -> torch.Tensor:
        """One reverse step at time step ``t`` for the whole batch; noise is drawn at every step, t = 0 included (the reference's sigma2 =
        beta has no special case)."""
        xt = xt.contiguous().float()
        tt = torch.full((xt.shape[0],), int(t), dtype=torch.int64, device=xt.device)
        eps = self.eps_model(xt, tt)
        out = torch.empty_like(xt)
        if self.noise_fn is None:
            _steps.ddpm_step(self._lib, xt, eps, out, coef=self.coef(t), rng=(self.seed, 0, self._draws, 0))
            self._draws += 1
            return out
        return _steps.ddpm_step(self._lib, xt, eps, out, coef=self.coef(t), noise_p=self._randn(xt.shape, xt.device))

    def sample(self, n: int, init: Optional[torch.Tensor] = None, init_step: Optional[int] = None,
               callback: Optional[Callable[[int, int, torch.Tensor], None]] = None) -> torch.Tensor:
        """``Configs.sample`` (inference.py:104-128): from x_T ~ N(0, I), or - with ``init`` - from ``q_sample(init, init_step)``, then
        steps ``init_step - 1 ... 0``.  ``callback(t_, t, x)`` runs after every step (the CLI's progress files)."""
        c = self.eps_model.cfg
        dev = self.eps_model.device
        if init is not None:
            assert init_step is not None, "sample: init needs init_step"
            xt = self.q_sample(init.to(dev), init_step)
        else:
            xt = self._randn((n, c.image_channels, c.img_h, c.img_w), dev)
        steps = init_step or self.n_steps
        for t_ in range(steps):
            t = steps - t_ - 1
            xt = self.p_sample(xt, t)
            if callback is not None:
                callback(t_, t, xt)
        return xt


class Polyffusion_DDPM:
    """``models/model_ddpm.py``: the wrapper the reference's learner drives.  ``get_loss_dict`` (:32-37) is the whole of it here."""

    def __init__(self, ddpm: DenoiseDiffusion, params: Optional[Mapping] = None, max_simu_note: int = 20):
        self.ddpm, self.params = ddpm, params

    def p_sample(self, xt: torch.Tensor, t: int) -> torch.Tensor:
        return self.ddpm.p_sample(xt, t)

    def q_sample(self, x0: torch.Tensor, t) -> torch.Tensor:
        return self.ddpm.q_sample(x0, t)

    def get_loss_dict(self, batch, step, *, detail: bool = False, **loss_kw):
        """``{"loss": ddpm.loss(prmat2c)}`` for a reference-layout batch ``(prmat2c, pnotree, chord, prmat)``; ``loss_kw`` (``noise``,
        ``t``, ``seed``, ``draw``, ``elem_offset``) go to ``DenoiseDiffusion.loss``; ``detail=True`` adds the per-sample ``"loss_rows"``
        (float64 ``[B]``) and the ``"t"`` they were evaluated at."""
        prmat2c = batch[0]
        if not detail:
            return {"loss": self.ddpm.loss(prmat2c, **loss_kw)}
        rows, t = self.ddpm.loss_rows(prmat2c, return_t=True, **loss_kw)
        return {"loss": rows.mean().float(), "loss_rows": rows, "t": t}


def state_from_checkpoint(path: str) -> Tuple["OrderedDict[str, torch.Tensor]", Optional[torch.Tensor], Optional[dict]]:
    """A trained ``ddpm`` checkpoint -> (eps_model state relative to ``eps_model.``, the saved ``ddpm.beta`` buffer, saved params).
    ``.pt`` (learner.py: ``{"model": state_dict}``) and Lightning ``.ckpt`` (``state_dict`` under ``model.``) both hold ``ddpm.*`` keys."""
    from .checkpoint import load_checkpoint
    state, params = load_checkpoint(path)
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    beta = None
    for k, v in state.items():
        if k == "ddpm.beta":
            beta = v
        elif k.startswith(PREFIX):
            out[k[len(PREFIX):]] = v
        else:
            raise RuntimeError(f"{path}: unexpected key {k!r} in a ddpm checkpoint")
    return out, beta, params


def load_trained(path: str, cfg: Optional[DDPMConfig] = None, n_steps: Optional[int] = None, x3: Optional[str] = None,
                 **diffusion_kw) -> DenoiseDiffusion:
    """``Polyffusion_DDPM.load_trained`` (models/model_ddpm.py:17-22): build the UNet, load the checkpoint, check the saved beta buffer
    against the float32 linspace the tables are rebuilt from."""
    state, beta, params = state_from_checkpoint(path)
    p = dict(DDPM_PARAMS)
    if params:
        p.update({k: v for k, v in params.items() if k in DDPM_PARAMS})
    cfg = cfg or DDPMConfig.from_params(p)
    n_steps = n_steps or int(p["n_steps"])
    ref_beta = ddpm_tables(n_steps)[0]
    if beta is not None and not torch.equal(torch.as_tensor(beta).float().cpu(), ref_beta):
        raise RuntimeError(f"{path}: the saved ddpm.beta is not linspace(1e-4, 0.02, {n_steps}) in float32")
    unet = DDPMUNet(cfg, x3=x3)
    unet.load_state_dict(state)
    return DenoiseDiffusion(unet, n_steps, **diffusion_kw)


def ddpm_model_state(eps_state: Mapping[str, object], n_steps: int = 1000) -> "OrderedDict[str, torch.Tensor]":
    """The full ``Polyffusion_DDPM`` state_dict (``ddpm.eps_model.*`` + ``ddpm.beta``) of an eps_model state (checkpoint fixtures)."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    out["ddpm.beta"] = ddpm_tables(n_steps)[0]
    for k, v in eps_state.items():
        out[PREFIX + k] = torch.as_tensor(np.asarray(v))
    return out


def params_from_dir(model_dir: Optional[str]) -> dict:
    """``<model_dir>/params.yaml`` when it exists, else the built-in ``ddpm.yaml`` values."""
    p = dict(DDPM_PARAMS)
    path = os.path.join(model_dir, "params.yaml") if model_dir else None
    if not path or not os.path.exists(path):
        return p
    import yaml
    with open(path) as f:
        data = yaml.safe_load(f) or {}
    p.update({k: v for k, v in data.items() if k in DDPM_PARAMS})
    return p
