"""Reverse-diffusion loops on the GPU: mirrors of the reference sampler classes.

* ``DiffusionSampler``  - ``stable_diffusion/sampler/__init__.py:25-80`` (``get_eps`` with
  classifier-free guidance; exact-float branches on the scale are kept).
* ``SDFSampler``        - ``sampler_sdf.py`` (tables :52-78, ``p_sample`` :80-171, ``q_sample``
  :173-192, ``sample`` :194-255, ``paint`` :257-350 incl. the RePaint quirks of Appendix A).
* ``DDIMSampler``       - ``sampler_ddim.py`` (tables :40-102, step :168-272, ``paint`` :301-362).
* ``DualScale`` / ``guidance_plan`` - not in the reference: separate guidance scales for the chord and texture parts of a ``chord+txt``
  condition, passed as ``uncond_scale``; the one function that decides what a guided eps evaluates.
* ``DDIMSampler.invert`` - not in the reference: the eta = 0 loop walked upwards, each step solved implicitly by fixed-point iterates
  (``pf_invert_step``), so that ``paint`` under another condition edits a given song; ``invert_coef_rows``, ``InversionRecord``.
* ``DDIMSampler.morph`` / ``DiffusionSampler.morph_from_noise`` - not in the reference: a path between two songs - both inverted as one
  batch, their noises interpolated on the sphere (``pf_slerp_rows``) and their conditions linearly, every point painted back down;
  ``morph_fractions``, ``MorphRecord``.
* ``DPMSolverSampler``  - not in the reference: DPM-Solver++(2M), the second-order multistep solver, driven like ``DDIMSampler``.
* ``WindowPlan``        - not in the reference: a song as one canvas whose half-overlapping windows are denoised as ONE batch per step, their
  noise predictions blended where they overlap (``DiffusionSampler.windows``; ``pf_window_split`` / ``pf_window_merge``).
* ``guidance_rescale`` / ``guidance_interval`` - not in the reference: settings of every family (``DiffusionSampler``).  Rescale (Lin et al.
  2024, section 3.4): a guided eps scaled back towards the conditional prediction's per-sample standard deviation and mixed with the plain
  combine by phi (``pf_cfg_rescale``).  Interval (Kynkaanniemi et al. 2024): guidance only while the time-step value lies in
  ``[t_lo, t_hi]``, the conditional evaluation alone outside it; ``normalize_guidance_interval``, ``guidance_interval_from_fractions``.
* ``x0_threshold`` - not in the reference: a setting of every family (``X0Threshold``).  The predicted clean image is clipped to the data
  range (``mode="clip"``; Ho et al. 2020, ``clip_denoised``) or dynamically thresholded at a percentile of its own magnitudes
  (``mode="dynamic"``; Saharia et al. 2022, section 2.3) inside every step, as a rewrite of eps (``pf_x0_threshold``).
* ``steering`` - not in the reference: a setting of ``SDFSampler`` and of ``DDIMSampler`` with eta > 0 (``Steering``).  The rows of a ``paint``
  call are groups of candidates for one song; every few steps their predicted clean images are scored and each group is resampled in
  proportion to ``exp(lam * reward gain)`` (``pf_x0_predict``, ``pf_steer_resample``, ``pf_rows_gather``); ``SteeringRecord``.

Same method names and argument meaning as the reference, so ``Experiments.predict`` drives
them unchanged.  Differences, all host-side plumbing:
  - per-step scalars are read from host tables and passed by value into ONE fused HIP kernel
    per step (``pf_ddpm_step`` / ``pf_ddim_step`` / ``pf_dpm_step``, launched through ``_steps`` - this module decides the route, ``_steps`` fills
    the argument struct) instead of ~20 elementwise launches and five device->host syncs per step;
  - noise comes from ``noise_fn(shape)`` when given (parity tests inject the reference's noise
    tape) and otherwise from the counter-based on-device generator keyed by (seed, draw counter,
    global sample index), so a batch sharded over N GPUs draws the same noise per sample as the
    unsharded batch.  Inside the loops the draws happen IN the update kernel
    (the ``rng`` form of the step: bit-identical to ``pf_randn`` + step, two launches and the noise
    tensors' HBM round trips less per step);
  - what the eps model computes from ``t`` and ``cond`` alone - the time MLP with every
    ResBlock's ``emb_layers`` and, for one context token, the whole cross-attention - is hoisted
    out of the loops: ``prepare()`` builds it once per ``paint()`` / ``sample()`` call and every
    step's forward receives it (``UNetModel.forward(time_table=, cross_bias=)``).  ``p_sample`` /
    ``get_eps`` called on their own keep working unprepared.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib, _steps
from .unet import LatentDiffusion

NoiseFn = Callable[[tuple], torch.Tensor]

GUIDANCE_ORDERS = ("chd,txt", "txt,chd")


@dataclass(frozen=True)
class DualScale:
    """Two guidance scales for a condition token that concatenates a chord part (columns ``[:split]``) and a texture part (``[split:]``), as
    the ``chord+txt`` models build it (``Polyffusion_SDF.get_loss_dict``: ``cat([zchd, ztxt], -1)``) and ``cond_mode: mix2`` trains it (each
    part dropped on its own).  Not in the reference.  Passed wherever ``uncond_scale`` takes a float::

        eps = eps(-, -) + first * (eps(a, -) - eps(-, -)) + second * (eps(a, b) - eps(a, -))

    where ``a`` is the part ``order`` names first (``"chd,txt"``: the intermediate evaluation keeps the chord and drops the texture;
    ``"txt,chd"``: the other way round) and a dropped part takes ``uncond_cond``'s columns.  Frozen and hashable: it is part of the key of a
    captured step.  Exact-float reductions (``guidance_plan``): ``first == second`` is single-scale guidance with that scale, bit for bit;
    ``second == 0`` is single-scale guidance towards the partial condition."""
    first: float
    second: float
    split: int
    order: str = "chd,txt"

    def __post_init__(self):
        if self.order not in GUIDANCE_ORDERS:
            raise ValueError(f"DualScale: order {self.order!r}, expected one of {GUIDANCE_ORDERS}")
        object.__setattr__(self, "first", float(self.first))
        object.__setattr__(self, "second", float(self.second))
        object.__setattr__(self, "split", int(self.split))

    @property
    def chd(self) -> float:
        """The scale of the term that brings the chord in."""
        return self.first if self.order == "chd,txt" else self.second

    @property
    def txt(self) -> float:
        return self.second if self.order == "chd,txt" else self.first

    def __str__(self):          # what Experiments._stamp writes after "scale="
        return f"chd:{self.chd},txt:{self.txt}" + ("" if self.order == "chd,txt" else ",txt-first")

    def partial(self, cond: torch.Tensor, uncond_cond: torch.Tensor) -> torch.Tensor:
        """``cond`` with the columns of the part named second replaced by ``uncond_cond``'s."""
        if not 0 < self.split < cond.shape[-1]:
            raise ValueError(f"DualScale: split {self.split} is not inside (0, {cond.shape[-1]}), the condition's last dimension")
        k, uc = self.split, uncond_cond.expand_as(cond)
        if self.order == "chd,txt":
            return torch.cat([cond[..., :k], uc[..., k:]], dim=-1)
        return torch.cat([uc[..., :k], cond[..., k:]], dim=-1)


Scale = Union[float, DualScale]


def scale_key(uncond_scale: Scale):
    """The guidance scale as part of a hashable key: the ``DualScale`` itself, or the float."""
    return uncond_scale if isinstance(uncond_scale, DualScale) else float(uncond_scale)


def guidance_plan(cond: torch.Tensor, uncond_scale: Scale, uncond_cond: Optional[torch.Tensor]) -> Tuple[torch.Tensor, int, tuple]:
    """THE branch logic of guided eps, shared by ``prepare`` and ``get_eps``: ``(context batch, groups, combine arguments)``.
      groups 1: the model on ``context`` is the result                                        (arguments ``()``)
      groups 2: ``context = cat([uncond_cond, c])``, ``pf_cfg_combine`` with ``(scale,)``       (the reference's ``get_eps``)
      groups 3: ``context = cat([uncond_cond, partial, cond])``, ``pf_cfg_combine3`` with ``(first, second)``
    A float takes the reference's exact-float branches (``sampler/__init__.py:63-74``): no ``uncond_cond`` or scale 1 -> ``cond`` alone,
    scale 0 -> ``uncond_cond`` alone.  A ``DualScale`` reduces first - ``first == second``: the float ``first`` with ``cond``;
    ``second == 0``: the float ``first`` with the partial condition in place of ``cond`` - and takes the float's branches from there."""
    if isinstance(uncond_scale, DualScale):
        ds = uncond_scale
        if uncond_cond is None:
            raise ValueError("DualScale guidance needs uncond_cond (the columns a dropped part takes)")
        partial = ds.partial(cond, uncond_cond)        # (validates split also where a reduction does not use the result)
        if ds.first == ds.second:
            uncond_scale = ds.first
        elif ds.second == 0.0:
            cond, uncond_scale = partial, ds.first
        else:
            return torch.cat([uncond_cond, partial, cond]), 3, (ds.first, ds.second)
    if uncond_cond is None or uncond_scale == 1.0:
        return cond, 1, ()
    if uncond_scale == 0.0:
        return uncond_cond, 1, ()
    return torch.cat([uncond_cond, cond]), 2, (float(uncond_scale),)


def normalize_guidance_interval(interval, n_steps: int) -> Optional[Tuple[int, int]]:
    """``(t_lo, t_hi)`` as a pair of ints with ``0 <= t_lo <= t_hi <= n_steps - 1`` (a ``ValueError`` otherwise), time-step VALUES of a schedule
    of ``n_steps``; the whole schedule ``(0, n_steps - 1)`` and ``None`` are ``None``: no interval, every step guided."""
    if interval is None:
        return None
    try:
        lo, hi = interval
        lo_i, hi_i = int(lo), int(hi)
    except (TypeError, ValueError):
        raise ValueError(f"guidance_interval {interval!r}: expected (t_lo, t_hi) or None") from None
    if lo_i != lo or hi_i != hi:
        raise ValueError(f"guidance_interval {interval!r}: t_lo and t_hi are time-step values, whole numbers")
    if not 0 <= lo_i <= hi_i <= int(n_steps) - 1:
        raise ValueError(f"guidance_interval ({lo_i}, {hi_i}): expected 0 <= t_lo <= t_hi <= {int(n_steps) - 1}, the time-step values of the schedule")
    return None if (lo_i, hi_i) == (0, int(n_steps) - 1) else (lo_i, hi_i)


def guidance_interval_from_fractions(lo: float, hi: float, n_steps: int) -> Optional[Tuple[int, int]]:
    """The interval given as fractions of the schedule, ``0 <= lo <= hi <= 1``: ``t_lo = ceil(lo * (T - 1))``, ``t_hi = floor(hi * (T - 1))``
    (what ``--guidance_interval LO HI`` passes on), normalised as above.  Fractions so close that no time step lies between them are refused."""
    lo, hi, T = float(lo), float(hi), int(n_steps)
    if not 0.0 <= lo <= hi <= 1.0:       # (a NaN fails)
        raise ValueError(f"guidance interval fractions ({lo}, {hi}): expected 0 <= LO <= HI <= 1")
    t_lo, t_hi = math.ceil(lo * (T - 1)), math.floor(hi * (T - 1))
    if t_lo > t_hi:
        raise ValueError(f"guidance interval fractions ({lo}, {hi}) hold no time step of a schedule of {T}")
    return normalize_guidance_interval((t_lo, t_hi), T)


X0_MODES = ("clip", "dynamic")


@dataclass(frozen=True)
class X0Threshold:
    """How the predicted clean image is bounded inside every reverse step (not in the reference).  ``mode="clip"``: x0 is clipped to
    ``range`` (``clip_denoised`` of Ho et al. 2020).  ``mode="dynamic"`` (Saharia et al. 2022, section 2.3): with ``c`` / ``h`` the centre
    / half-width of ``range``, every sample's ``x0 - c`` is clipped at ``s = min(max(q, h), s_max * h)``, ``q`` the exact ``p``-quantile
    of its own ``|x0 - c|``, and scaled by ``h / s`` back into the range; a sample with ``q <= h`` is clipped statically.  Frozen and
    hashable: it is part of the key of a captured step."""
    mode: str = "dynamic"
    p: float = 0.995
    range: Tuple[float, float] = (0.0, 1.0)
    s_max: float = float("inf")

    def __post_init__(self):
        if self.mode not in X0_MODES:
            raise ValueError(f"x0_threshold mode {self.mode!r}: expected one of {X0_MODES}")
        try:
            lo, hi = (float(v) for v in self.range)
        except (TypeError, ValueError):
            raise ValueError(f"x0_threshold range {self.range!r}: expected (lo, hi)") from None
        if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
            raise ValueError(f"x0_threshold range ({lo}, {hi}): expected lo < hi, both finite")
        p, s_max = float(self.p), float(self.s_max)
        if not 0.0 < p <= 1.0:           # (a NaN fails both)
            raise ValueError(f"x0_threshold p {p} outside (0, 1]")
        if not s_max >= 1.0:
            raise ValueError(f"x0_threshold s_max {s_max} below 1")
        object.__setattr__(self, "range", (lo, hi))
        object.__setattr__(self, "p", p)
        object.__setattr__(self, "s_max", s_max)

    @property
    def label(self) -> str:
        """The setting as file names and reports spell it: ``x0clip`` / ``x0thr=P``, with the range and the cap only when not the defaults."""
        how = "x0clip" if self.mode == "clip" else f"x0thr={self.p}"
        how += "" if self.range == (0.0, 1.0) else f",x0range={self.range[0]}-{self.range[1]}"
        return how + ("" if self.mode == "clip" or math.isinf(self.s_max) else f",x0max={self.s_max}")


def normalize_x0_threshold(setting) -> Optional[X0Threshold]:
    """``None`` or an ``X0Threshold`` (a ``ValueError`` for anything else; the dataclass validates its own fields)."""
    if setting is None or isinstance(setting, X0Threshold):
        return setting
    raise ValueError(f"x0_threshold {setting!r}: expected None or an X0Threshold")


# named steering rewards: the score of score.scores_of / score.texture_fit on the song-summed counters, and its sign (higher is better)
STEER_REWARDS = {"chord": ("chord_f1", 1.0), "bass": ("bass_fit", 1.0), "integrity": ("integrity", -1.0), "texture": ("texture_fit", 1.0)}


@dataclass
class Steering:
    """Steer the candidates of a song while they are sampled (Feynman-Kac / SMC steering, Singhal et al. 2025; the twisted diffusion
    sampler of Wu et al. 2023; not in the reference).  The rows of a ``paint`` call are groups of ``n`` consecutive particles of ``per``
    consecutive images each (a song of ``per`` segments; under a ``WindowPlan`` a particle is one canvas).  At a steered step the predicted
    clean image of every particle is scored, each group is resampled in proportion to ``exp(lam * (reward - reward at its last
    resampling))`` when its effective sample size is at most ``ess * n`` (``pf_steer_resample``), and ``x`` and eps move to their survivors
    (``pf_rows_gather``); copies diverge again because every row draws its own noise.  A step is steered when it is the ``every``-th of the
    loop, its time-step value lies in ``window`` (fractions of the schedule, as ``guidance_interval_from_fractions`` reads them) and it is
    not the last.  The particles of a group are candidates for the SAME song: only ``x`` and eps (and a multistep solver's history) are moved, so ``cond``, ``orig``, ``mask``
    and ``cond_concat`` are expected equal within a group.

    ``reward``: ``"chord"`` (chord_f1), ``"bass"`` (bass_fit), ``"integrity"`` (the orphan fraction, negated) or ``"texture"`` (texture_fit
    against ``onsets``) of ``score.roll_stats`` on the predicted image - with ``chord`` (rows of 36, one per beat, in the images' order),
    ``mask`` (shaped like the images: only cells whose mask is 0 count) and ``bass_relative`` as there, ``onsets`` int ``[particles or 1,
    steps of a particle]`` the reference onset counts per step; or a callable ``(x0 [rows, C, H, W]) -> float64 [rows / per]`` on the device.
    ``lam = 0`` or ``steering=None`` give today's bits."""
    n: int
    reward: Union[str, Callable] = "chord"
    per: int = 1
    lam: float = 10.0
    every: int = 5
    window: Tuple[float, float] = (0.0, 1.0)
    ess: float = 0.5
    chord: Optional[torch.Tensor] = None
    mask: Optional[torch.Tensor] = None
    bass_relative: bool = False
    onsets: Optional[torch.Tensor] = None

    def __post_init__(self):
        for f in ("n", "per", "every"):
            v = getattr(self, f)
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"steering {f} {v!r}: a whole number")
            setattr(self, f, int(v))
        if not 1 <= self.n <= _lib.STEER_MAX_N:
            raise ValueError(f"steering n {self.n} outside [1, {_lib.STEER_MAX_N}] particles per group")
        if self.per < 1 or self.every < 1:
            raise ValueError(f"steering per {self.per} and every {self.every}: both at least 1")
        self.lam, self.ess = float(self.lam), float(self.ess)
        if not (math.isfinite(self.lam) and self.lam >= 0.0):
            raise ValueError(f"steering lam {self.lam}: finite and >= 0")
        if not 0.0 < self.ess <= 1.0:        # (a NaN fails both)
            raise ValueError(f"steering ess {self.ess} outside (0, 1]")
        try:
            lo, hi = (float(v) for v in self.window)
        except (TypeError, ValueError):
            raise ValueError(f"steering window {self.window!r}: expected (lo, hi)") from None
        if not 0.0 <= lo <= hi <= 1.0:
            raise ValueError(f"steering window ({lo}, {hi}): expected 0 <= lo <= hi <= 1, fractions of the schedule")
        self.window = (lo, hi)
        if not callable(self.reward):
            if self.reward not in STEER_REWARDS:
                raise ValueError(f"steering reward {self.reward!r}: expected one of {sorted(STEER_REWARDS)} or a callable")
            if self.reward in ("chord", "bass") and self.chord is None:
                raise ValueError(f"steering reward {self.reward!r} needs chord, the chord rows of the images")
            if self.reward == "texture" and self.onsets is None:
                raise ValueError("steering reward 'texture' needs onsets, the reference onset counts per step")

    def window_values(self, n_steps: int) -> Tuple[int, int]:
        """The window as time-step values of a schedule of ``n_steps``: ``(ceil(lo * (T - 1)), floor(hi * (T - 1)))`` - possibly empty."""
        T = int(n_steps)
        return math.ceil(self.window[0] * (T - 1)), math.floor(self.window[1] * (T - 1))

    @property
    def label(self) -> str:
        """The setting as file names spell it: ``steer=REWARD,lam=L`` and whatever else is not the default."""
        how = f"steer={self.reward if isinstance(self.reward, str) else 'fn'},lam={self.lam}"
        how += "" if self.every == 5 else f",every={self.every}"
        how += "" if self.window == (0.0, 1.0) else f",win={self.window[0]}-{self.window[1]}"
        return how + ("" if self.ess == 0.5 else f",ess={self.ess}")


def normalize_steering(setting) -> Optional[Steering]:
    if setting is None or isinstance(setting, Steering):
        return setting
    raise ValueError(f"steering {setting!r}: expected None or a Steering")


@dataclass
class SteeringRecord:
    """What the steering events of one ``paint`` call leave behind, as device tensors that nothing reads until asked: per event the loop's
    step number and time-step value (host ints), ``rewards`` / ``weights`` float64 ``[groups * n]``, ``stats`` float64 ``[groups, 4]``
    (ESS, sum of weights, flag - 0 kept, 1 resampled, 2 no finite weight -, u) and ``ancestors`` int32 ``[groups * n]``, group-local."""
    n: int
    particles: int
    steps: list
    t_values: list
    rewards: list
    weights: list
    stats: list
    ancestors: list

    @classmethod
    def merged(cls, records) -> "SteeringRecord":
        """The records of several ``paint`` calls over the same steps (consecutive groups of one run) as one, their groups in the calls' order."""
        a = records[0]
        if any((r.n, r.steps, r.t_values) != (a.n, a.steps, a.t_values) for r in records):
            raise ValueError("SteeringRecord.merged: the records do not describe the same events")
        cat = lambda name: [torch.cat([getattr(r, name)[k] for r in records]) for k in range(len(a.steps))]
        return cls(a.n, sum(r.particles for r in records), list(a.steps), list(a.t_values), cat("rewards"), cat("weights"), cat("stats"), cat("ancestors"))

    def lineage(self) -> np.ndarray:
        """int64 ``[groups, n]``: the particle of the start population every final particle descends from, group-local - the events'
        ancestors composed (copies the tables: the one host sync).  Without an event: the identity."""
        out = None
        for a in self.ancestors:
            a = a.detach().cpu().numpy().astype(np.int64).reshape(-1, self.n)
            out = a if out is None else np.take_along_axis(out, a, axis=1)
        return np.tile(np.arange(self.n, dtype=np.int64), (self.particles // self.n, 1)) if out is None else out

    def report(self) -> dict:
        """The events as plain Python (one host copy): step numbers, time-step values, per-group ESS and flags."""
        st = [s.detach().cpu().numpy() for s in self.stats]
        return {"steps": list(self.steps), "t": list(self.t_values), "ess": [s[:, 0].tolist() for s in st],
                "resampled": [[int(f) for f in s[:, 2]] for s in st], "u": [s[:, 3].tolist() for s in st]}


BLENDS = ("mean", "ramp")
MAX_COVER = 8          # windows over one canvas row that pf_window_merge accepts: ceil(win_h / stride)


@dataclass(frozen=True)
class WindowPlan:
    """A song as ONE canvas of ``canvas_h = stride * (n_windows - 1) + win_h`` rows that the denoiser sees as the batch of its ``n_windows``
    windows of ``win_h`` rows, ``stride`` rows apart (MultiDiffusion, Bar-Tal et al. 2023, along the time axis; not in the reference).  Window
    ``j`` of song ``s`` is batch row ``s * n_windows + j`` and canvas rows ``[j * stride, j * stride + win_h)``.  Where windows overlap their
    noise predictions are blended per row with ``weights()``: ``mean`` - ones; ``ramp`` - with ``ov = win_h - stride`` and
    ``r = row + 0.5``, ``min(1, r / ov, (win_h - r) / ov)``: a window fades in over the rows it shares with its left neighbour and out over
    those it shares with its right one (at ``stride == win_h / 2`` the weights of the two windows over a row sum to exactly 1).  Set as
    ``DiffusionSampler.windows``.  Frozen and hashable: ``key`` is part of the key of a captured step."""
    n_windows: int
    stride: int
    win_h: int
    blend: str = "mean"

    def __post_init__(self):
        for f in ("n_windows", "stride", "win_h"):
            object.__setattr__(self, f, int(getattr(self, f)))
        if self.blend not in BLENDS:
            raise ValueError(f"WindowPlan: blend {self.blend!r}, expected one of {BLENDS}")
        if self.n_windows < 1 or self.win_h < 1:
            raise ValueError(f"WindowPlan: {self.n_windows} windows of {self.win_h} rows")
        if not 1 <= self.stride <= self.win_h:
            raise ValueError(f"WindowPlan: stride {self.stride} outside [1, win_h = {self.win_h}] (beyond it rows would belong to no window)")
        if -(-self.win_h // self.stride) > MAX_COVER:
            raise ValueError(f"WindowPlan: stride {self.stride} puts {-(-self.win_h // self.stride)} windows of {self.win_h} rows over one row, "
                             f"at most {MAX_COVER}")

    @property
    def canvas_h(self) -> int:
        return self.stride * (self.n_windows - 1) + self.win_h

    @property
    def key(self) -> tuple:
        return (self.n_windows, self.stride, self.win_h, self.blend)

    def cover(self, y: int) -> List[int]:
        """The windows over canvas row ``y``, ascending: every ``j`` with ``0 <= y - j * stride < win_h``."""
        if not 0 <= y < self.canvas_h:
            raise IndexError(f"WindowPlan: row {y} outside a canvas of {self.canvas_h} rows")
        lo = 0 if y < self.win_h else (y - self.win_h) // self.stride + 1
        return list(range(lo, min(self.n_windows - 1, y // self.stride) + 1))

    def weights(self) -> np.ndarray:
        """float32 ``[win_h]``, every weight > 0: what ``pf_window_merge`` receives as ``row_weight``."""
        ov = self.win_h - self.stride
        if self.blend == "mean" or ov == 0:
            return np.ones(self.win_h, dtype=np.float32)
        r = np.arange(self.win_h, dtype=np.float64) + 0.5
        return np.minimum(1.0, np.minimum(r / ov, (self.win_h - r) / ov)).astype(np.float32)


class DiffusionSampler:
    model: LatentDiffusion

    def __init__(self, model: LatentDiffusion, noise_fn: Optional[NoiseFn] = None, seed: int = 0, sample_offset: int = 0,
                 graph: bool = False, windows: Optional[WindowPlan] = None, guidance_rescale: float = 0.0,
                 guidance_interval: Optional[Tuple[int, int]] = None, x0_threshold: Optional[X0Threshold] = None,
                 steering: Optional[Steering] = None):
        self.model = model
        # windows: x, orig, mask, orig_noise and cond_concat are song canvases [S, ., canvas_h, W], cond / uncond_cond have S * n_windows rows
        # in the plan's window order, and get_eps evaluates the denoiser on the batch of windows (pf_window_split), blending its predictions
        # back onto the canvas (pf_window_merge).  Everything behind get_eps is elementwise on the canvas.  None: no windows, today's launches.
        self.windows = windows
        self.n_steps = model.n_steps
        self.noise_fn = noise_fn
        self.seed = int(seed)
        self.sample_offset = int(sample_offset)  # global index of this rank's first sample (multi-GPU sharding)
        self._draws = 0
        # classifier-free guidance evaluates the denoiser on cat([x, x]); the part of it that cannot depend on the condition is shared
        # between the halves unless this is switched off (results equal up to tile-choice rounding; tests compare both)
        self.share_cfg_prefix = True
        self._lib = _lib.load()
        self._trows = None
        # graph=True: paint() captures ONE reverse step as a hipGraph and replays it.  What varies per step
        # (table row, time-step value, noise draw counter) lives in a device-resident pf_step_state, the coefficient table is on
        # the device, x is updated in place: a replay issues no host-side launches (about 220 per step in eager mode), which is
        # what bounds small batches (batch 1 of the --autoreg CLI, batch 8 per GPU of BASELINE config 5).  Results are bit-identical
        # to the eager loop.  Used only with the on-device noise generator (an injected noise_fn is host code).
        self.graph = bool(graph)
        self._dev_cache = {}
        # captured steps, kept across paint() calls (the autoregressive schedule calls paint() 2B-1 times with the same shapes):
        # key = everything that shapes the captured launch sequence, value = the graph + the static buffers its nodes point at
        self._graphs = {}
        self.graph_captures = 0
        # on_step(step, x): called by the eager loops of paint() after every reverse step with the step's number and its result
        # (the reference's `is_show_image` hook, sampler_sdf.py:338-345, as a callback).  None = no call, no cost.  Used by the
        # full-length parity runs (tools/long_parity.py) to record how two arithmetic modes drift apart along one noise tape.
        self.on_step: Optional[Callable[[int, torch.Tensor], None]] = None
        # guidance_rescale (phi): a guided eps is scaled back towards the conditional prediction's per-sample standard deviation and mixed
        # with the plain combine by phi (pf_cfg_rescale in place of pf_cfg_combine / pf_cfg_combine3); 0.0: today's combine, exactly.
        # guidance_interval (t_lo, t_hi): guidance only while the time-step VALUE the denoiser is fed lies in [t_lo, t_hi]; outside it a
        # call is get_eps(..., uncond_scale=1.0): cond alone, one evaluation at the plain batch.  None: every step is guided.
        self.guidance_rescale = guidance_rescale
        self.guidance_interval = guidance_interval
        self.last_rescale = None      # (stats float64 [rows, 3] = var_pos, var_cfg, f; weights float32 [rows]) of the last rescaled call, on the device
        # x0_threshold: None, or how the predicted clean image is bounded at EVERY step (independent of the interval): get_eps ends with
        # pf_x0_threshold on its result - after the combine, the rescale or the merge; under a window plan on the canvas.  None: today's launches.
        self.x0_threshold = x0_threshold
        self.last_threshold = None    # stats float64 [rows, 4] = q, s, w, changed elements of the last thresholded call, on the device
        # steering: None, or how the candidates of a song are resampled while the eager loops of paint() run (Steering).  None: today's launches.
        self._steer_events = 0        # steering events so far: the counter word of the resampling draw, as _draws is of the noise draws
        self.last_steering = None     # SteeringRecord of the last steered paint()
        self.steering = steering
        self._check_guidance()

    # ---- steering by resampling (not in the reference) ---------------------------------------------------------------------------------
    @property
    def steering(self) -> Optional[Steering]:
        return getattr(self, "_steering", None)

    @steering.setter
    def steering(self, setting):
        setting = normalize_steering(setting)
        if setting is not None:
            why = self._steer_refusal()
            if why is not None:
                raise ValueError(f"steering: {why}")
        self._steering = setting

    def _steer_refusal(self) -> Optional[str]:
        """Why this sampler cannot be steered, or ``None``."""
        if self.graph:
            return ("graph=True: a captured step is ONE launch sequence, and the steered and the unsteered step are two (the cause that "
                    "refuses guidance_interval; out of scope)")
        if self.noise_fn is not None:
            return "an injected noise_fn: copies of a survivor diverge through the per-row draws of the on-device generator"
        return None

    def _steer_begin(self, x, repaint_n: int = 1):
        """The state of a steered ``paint`` loop, or ``None`` without steering: validates the rows, resets ``last_steering``."""
        st = self.steering
        if st is None:
            return None
        why = self._steer_refusal()
        if why is not None:
            raise ValueError(f"steering: {why}")
        if int(repaint_n) > 1:
            raise ValueError(f"steering: repaint_n {repaint_n} > 1 (a resampled state cannot be re-noised back to the step it came from)")
        rows, block = x.shape[0], st.n * st.per
        if rows % block != 0 or self.sample_offset % block != 0:
            raise ValueError(f"steering: {rows} rows at sample_offset {self.sample_offset} are not whole groups of {st.n} particles of {st.per} image(s)")
        self.last_steering = SteeringRecord(st.n, rows // st.per, [], [], [], [], [], [])
        return {"st": st, "base": torch.zeros(rows // st.per, dtype=torch.float64, device=x.device), "window": st.window_values(self.model.n_steps),
                "group_offset": self.sample_offset // block}

    @staticmethod
    def _steered_at(ctx, i: int, t_value: int, last: bool) -> bool:
        """The host's decision: step ``i`` (0-based) of the loop is the ``every``-th, its time-step value lies in the window, it is not the last."""
        lo, hi = ctx["window"]
        return (i + 1) % ctx["st"].every == 0 and lo <= int(t_value) <= hi and not last

    def _steer_reward(self, st: Steering, x0: torch.Tensor) -> torch.Tensor:
        particles = x0.shape[0] // st.per
        if callable(st.reward):
            r = st.reward(x0)
        else:
            from . import score
            rs = score.roll_stats(x0, st.chord, st.mask, bass_relative=st.bass_relative).songs(st.per)
            key, sign = STEER_REWARDS[st.reward]
            if st.reward == "texture":
                ref = st.onsets.to(device=x0.device).reshape(-1, rs.onsets.shape[1]).expand(particles, -1)
                r = score.texture_fit(rs, score.RollStats(rs.counters, rs.chroma, ref))
            else:
                r = rs.scores()[key]
            r = r if sign > 0 else -r
        if not isinstance(r, torch.Tensor) or r.device != x0.device or r.numel() != particles:
            raise ValueError(f"steering: the reward must be a tensor of {particles} values (one per particle) where x0 lives")
        return r.to(torch.float64).reshape(particles).contiguous()

    def _steer_event(self, ctx, x, e_t, t, i: int, t_value: int, extra=()):
        """One steering event between ``get_eps`` and the update: ``(x, e_t)`` moved to their survivors.  ``t``: the int64 vector the
        denoiser was fed.  ``extra``: further row tensors shaped like ``x`` that belong to a particle (a multistep solver's history) - they
        move in the same ``pf_rows_gather`` launch and follow in the result, ``(x, e_t, *extra)``.  Five launches beside the reward's own;
        no host sync."""
        st, wp = ctx["st"], getattr(self, "windows", None)
        x, e_t = x.contiguous(), e_t.contiguous()
        x0 = _steps.x0_predict(self._lib, x, e_t, t.contiguous(), self.model.x0_threshold_table(x.device), t_stride=1 if wp is None else wp.n_windows)
        reward = self._steer_reward(st, x0)
        anc, weights, stats = _steps.steer_resample(self._lib, reward, ctx["base"], st.n, lam=st.lam, ess=st.ess, seed=self.seed,
                                                    group_offset=ctx["group_offset"], event=self._steer_events)
        self._steer_events += 1
        moved = _steps.rows_gather(self._lib, [x, e_t] + [v.contiguous() for v in extra], anc, st.n, st.per)
        rec = self.last_steering
        for lst, v in ((rec.steps, int(i)), (rec.t_values, int(t_value)), (rec.rewards, reward), (rec.weights, weights), (rec.stats, stats), (rec.ancestors, anc)):
            lst.append(v)
        return tuple(moved)

    # ---- clipping / dynamic thresholding of the predicted x0 (not in the reference) -------------------------------------------------------
    @property
    def x0_threshold(self) -> Optional[X0Threshold]:
        return getattr(self, "_x0_threshold", None)

    @x0_threshold.setter
    def x0_threshold(self, setting):
        self._x0_threshold = normalize_x0_threshold(setting)

    def _threshold(self, x, t, e_t):
        """``e_t`` with its predicted x0 bounded as ``self.x0_threshold`` says (in place: ``e_t`` is this call's own tensor).  ``x``: what
        eps was predicted from, ``cond_concat`` channels included (they lie behind the row's first elements); ``t``: the int64 vector the
        denoiser was fed - under a window plan one entry per window, and a canvas reads its first window's."""
        th = self.x0_threshold
        if th is None:
            return e_t
        wp = getattr(self, "windows", None)
        e_t = e_t.contiguous()
        _, stats = _steps.x0_threshold(self._lib, x.contiguous(), e_t, t.contiguous(), self.model.x0_threshold_table(x.device), mode=th.mode, p=th.p,
                                       range=th.range, s_max=th.s_max, t_stride=1 if wp is None else wp.n_windows, out=e_t, want_stats=True)
        self.last_threshold = stats
        return e_t

    # ---- guidance rescale and guidance interval (not in the reference) ------------------------------------------------------------------
    @property
    def guidance_rescale(self) -> float:
        return getattr(self, "_guidance_rescale", 0.0)

    @guidance_rescale.setter
    def guidance_rescale(self, phi):
        phi = float(phi)
        if not 0.0 <= phi <= 1.0:        # (a NaN fails both)
            raise ValueError(f"guidance_rescale {phi} outside [0, 1]")
        self._guidance_rescale = phi

    @property
    def guidance_interval(self) -> Optional[Tuple[int, int]]:
        return getattr(self, "_guidance_interval", None)

    @guidance_interval.setter
    def guidance_interval(self, interval):
        self._guidance_interval = normalize_guidance_interval(interval, self.model.n_steps)

    def _check_guidance(self):
        if self.graph and self.guidance_interval is not None:
            raise ValueError(f"guidance_interval {self.guidance_interval} with graph=True: a captured step is ONE launch sequence, and the guided "
                             "and the unguided step are two (out of scope: two captures with a hand-over between their static buffers)")

    def guided_at(self, t_value) -> bool:
        """Whether a call that feeds the denoiser time-step value ``t_value`` (for DDIM / DPM the tau entry, not the grid index) is guided."""
        iv = self.guidance_interval
        return iv is None or iv[0] <= int(t_value) <= iv[1]

    def _guidance_at(self, t_value, uncond_scale, prep):
        """THE place the interval is resolved, for every loop, ``p_sample``, ``invert`` and ``morph`` (all of them reach ``get_eps`` through
        ``_eps``, which knows the time-step value on the host): ``(uncond_scale, prep)`` of this call - as given inside the interval, ``1.0``
        and the prefix hoisted for ``cond`` alone (``prepare()``'s ``"unguided"`` entry) outside it."""
        if self.guidance_interval is None:
            return uncond_scale, prep
        if t_value is None:
            raise ValueError(f"get_eps: guidance_interval {self.guidance_interval} is set and the call does not say which time step it is "
                             "(t_value=): it cannot tell whether it is guided")
        if self.guided_at(t_value):
            return uncond_scale, prep
        return 1.0, None if prep is None else prep.get("unguided")

    def _step_state(self, device) -> torch.Tensor:
        key = ("state", str(device))
        if key not in self._dev_cache:
            self._dev_cache[key] = torch.zeros(2, dtype=torch.int64, device=device)   # pf_step_state {int64 index; uint64 draws}
        return self._dev_cache[key]

    def _set_state(self, st: torch.Tensor, index: int):
        _lib.check(self._lib.pf_step_state_set(st.data_ptr(), int(index), int(self._draws), _lib.current_stream()), "pf_step_state_set")

    _MAX_GRAPHS = 4

    def _graph_token(self):
        """What a captured step depends on besides its own buffers: the UNet's workspace and weight blob (addresses are baked
        into the graph nodes; the workspace is re-allocated when a larger batch comes along) and the arithmetic mode."""
        m = self.model.eps_model
        ws = getattr(m, "_ws", None)
        blob = getattr(m, "_blob_dev", None)
        return (0 if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), 0 if blob is None else blob.data_ptr(),
                getattr(m, "precision", None)) + (m.options_key() if hasattr(m, "options_key") else ())

    def _graph_for(self, key, inputs, make_body, reset, uncond_scale=1.0):
        """The captured step for `key`, with `inputs` (name -> tensor or None) copied into its static buffers.  A cached entry is
        dropped when the UNet's workspace / weights / mode changed since its capture.  `make_body(bufs)` returns the step closure
        over the static buffers, `reset()` re-arms the device step state (called after every buffer refresh).  Returns the entry
        {"g": graph, "bufs": {...}}.  bufs["_prep"] holds the hoisted prefix (prepare()) in static buffers of its own: it is
        recomputed IN PLACE from the refreshed cond buffers on every call, so the captured forward always reads current values."""
        ent = self._graphs.get(key)
        if ent is not None and ent["token"] != self._graph_token():
            del self._graphs[key]
            ent = None
        if ent is None:
            bufs = {k: (None if v is None else v.clone()) for k, v in inputs.items()}
            bufs["_prep"] = self.prepare(bufs["cond"], uncond_scale=uncond_scale, uncond_cond=bufs.get("uncond_cond"))

            def restore():
                bufs["x"].copy_(inputs["x"])
                reset()

            reset()
            g = self._capture(make_body(bufs), restore)
            self.graph_captures += 1
            while len(self._graphs) >= self._MAX_GRAPHS:
                self._graphs.pop(next(iter(self._graphs)))
            ent = self._graphs[key] = {"g": g, "bufs": bufs, "token": self._graph_token()}   # token AFTER the warm-up sized the workspace
        else:
            for k, v in inputs.items():
                if v is not None:
                    ent["bufs"][k].copy_(v)
            self.prepare(ent["bufs"]["cond"], uncond_scale=uncond_scale, uncond_cond=ent["bufs"].get("uncond_cond"), out=ent["bufs"]["_prep"])
            reset()
        return ent

    @staticmethod
    def _shape_key(**tensors):
        return tuple((k, None if v is None else (tuple(v.shape), str(v.dtype))) for k, v in sorted(tensors.items()))

    def _capture(self, body, restore):
        """Warm `body` up once on a side stream (sizes the workspace, primes the allocator), undo its effect with `restore`,
        then capture it.  Returns the instantiated graph."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            body()
            restore()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            body()
        restore()
        return g

    def _replay_loop(self, family, inputs, table, taus, ndraw, n_noise, replays, t_start, uncond_scale, update, body_of=None):
        """`replays` reverse steps from table row `t_start` down as replays of ONE captured step; returns the resulting x.  `inputs`: name ->
        tensor or None (x, cond, uncond_cond, cond_concat and what `update` reads), `taus`: the device tau table (None: the row index is
        the time step), `ndraw`: noise draws per step, `n_noise`: how many of them need a tensor (bufs["_noise"]; none when they are made in
        the update kernel), `update(bufs, e_t, table, state)`: the family's in-place update of bufs["x"].  `body_of(bufs, t_buf, state)`: a
        step of another shape than {begin, eps, update, end} (the upward step of `DDIMSampler.invert`) - it returns the closure to capture and
        `update` is not used; the static buffers of the call stay reachable as `self._last_bufs`."""
        self._check_guidance()
        x = inputs["x"]
        dev, B, st = x.device, self._eps_rows(x), self._step_state(x.device)      # B: rows the denoiser sees (one per window under a plan)

        def make_body(bf):
            tb = bf["_t"] = torch.empty(B, dtype=torch.long, device=dev)
            bf["_noise"] = [torch.empty_like(bf["x"]) for _ in range(n_noise)]
            if body_of is not None:
                return body_of(bf, tb, st)

            def body():
                _lib.check(self._lib.pf_step_begin(st.data_ptr(), _lib.ptr(taus), tb.data_ptr(), B, _lib.current_stream()), "pf_step_begin")
                xin = bf["x"] if bf["cond_concat"] is None else torch.cat([bf["x"], bf["cond_concat"]], dim=1)
                e_t = self.get_eps(xin, tb, bf["cond"], uncond_scale=uncond_scale, uncond_cond=bf["uncond_cond"], prep=bf["_prep"])
                update(bf, e_t, table, st)
                _lib.check(self._lib.pf_step_end(st.data_ptr(), ndraw, _lib.current_stream()), "pf_step_end")
            return body

        wkey = None if self.windows is None else self.windows.key
        key = (family, str(dev), scale_key(uncond_scale), self.guidance_rescale, self.x0_threshold, self.seed, self._elem_offset(x.shape), ndraw, wkey) + self._shape_key(**inputs)
        ent = self._graph_for(key, inputs, make_body, lambda: self._set_state(st, t_start), uncond_scale)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            ent["g"].replay()
        e1.record()
        self.last_replay = (e0, e1, replays)     # bench.py reads the per-step replay time from these events
        self._last_bufs = ent["bufs"]
        self._draws += ndraw * replays
        return ent["bufs"]["x"].clone()   # the static buffer is overwritten by the next paint() with these shapes

    # ---- noise ------------------------------------------------------------------------------------
    def _elem_offset(self, shape) -> int:
        """Index of this rank's first element of a [B, ...] tensor in the unsharded one."""
        return self.sample_offset * int(np.prod(shape[1:]))

    def randn(self, shape, device) -> torch.Tensor:
        return _steps.draw(self, shape, device, self._elem_offset(shape))

    # ---- the step-invariant prefix of the eps model, hoisted out of the loops ------------------------------
    def prepare(self, cond: torch.Tensor, *, uncond_scale: float = 1.0, uncond_cond: Optional[torch.Tensor] = None,
                out: Optional[dict] = None) -> dict:
        """What ``get_eps(x, t, cond, uncond_scale=, uncond_cond=)`` computes WITHOUT looking at x, for every t of the schedule:
        ``time_table`` [n_steps, W] (time MLP + all ``emb_layers`` per time-step value, ``unet.py:181-182, 286-289``) and ``cross`` -
        the collapsed one-token cross-attention biases (``unet_attention.py:186-212``) of exactly the context batch ``get_eps`` feeds
        the model: ``cond``, ``uncond_cond`` or ``cat([uncond_cond, cond])`` by the reference's exact-float branches
        (``sampler/__init__.py:63-74``; ``guidance_plan`` decides, for ``get_eps`` too).  ``None`` entries (several context tokens) are computed inside every forward as before.
        Called explicitly by the loops of this class; pass the result as ``prep=`` with the SAME cond / guidance arguments.
        ``out``: a previous result whose buffers are overwritten in place (captured-graph replay).
        With a ``guidance_interval`` the steps outside it evaluate ``cond`` alone: the result then carries a second prefix for that context
        under ``"unguided"`` (the time table is shared), which ``get_eps`` picks for such a step."""
        m = self.model.eps_model
        ctx, groups, _ = guidance_plan(cond, uncond_scale, uncond_cond)     # (a DualScale: possibly the three groups of dual guidance)
        o = out or {}
        # one row more than the schedule has steps: the DDIM tau table is shifted by +1 (sampler_ddim.py:63-73)
        prep = {"time_table": m.prepare_time(self.model.n_steps + 1, out=o.get("time_table")),
                "cross": m.prepare_cond(ctx, out=o.get("cross"))}
        if self.guidance_interval is not None:
            un = o.get("unguided") or {}
            prep["unguided"] = prep if groups == 1 and ctx is cond else {"time_table": prep["time_table"], "cross": m.prepare_cond(cond, out=un.get("cross"))}
        return prep

    @staticmethod
    def _prep_kw(prep):
        return {} if prep is None else {"time_table": prep["time_table"], "cross_bias": prep["cross"]}

    # ---- eps with classifier-free guidance ----------------------------------------------------------
    def get_eps(self, x: torch.Tensor, t: torch.Tensor, c: torch.Tensor, *, uncond_scale: Scale,
                uncond_cond: Optional[torch.Tensor], prep: Optional[dict] = None, t_value: Optional[int] = None):
        """``uncond_scale``: the reference's float, or a ``DualScale`` (separate scales for the chord and texture parts of ``c``).
        With a window plan (``self.windows``): ``x`` is the canvas ``[S, C, canvas_h, W]``, ``t`` / ``c`` / ``uncond_cond`` have one row per
        window, and the result is the canvas eps - split, the same evaluation on the windows, and ONE merge launch that also combines the groups.
        ``t_value``: the time-step value of ``t`` on the host; needed (a ``ValueError`` without it) only under a ``guidance_interval``,
        outside which the call is ``uncond_scale=1.0``.  ``guidance_rescale != 0``: a guided call combines its groups with ``pf_cfg_rescale``
        (per batch entry; under a window plan per WINDOW, on the window batch, followed by a plain merge) and leaves the device tables
        in ``self.last_rescale``; one group (scale 1, scale 0, no ``uncond_cond``) has nothing to rescale.
        ``x0_threshold``: the result - whatever produced it - then has its predicted x0 clipped or thresholded (``pf_x0_threshold``, per
        batch entry, under a window plan per canvas), at every step, and the device ``stats`` stay in ``self.last_threshold``."""
        e_t = self._get_eps(x, t, c, uncond_scale, uncond_cond, prep, t_value)
        return e_t if self.x0_threshold is None else self._threshold(x, t, e_t)

    def _get_eps(self, x, t, c, uncond_scale, uncond_cond, prep, t_value):
        uncond_scale, prep = self._guidance_at(t_value, uncond_scale, prep)
        wp = getattr(self, "windows", None)
        if wp is not None:
            return self._get_eps_windows(wp, x, t, c, uncond_scale, uncond_cond, prep)
        epsg, groups, scales = self._eps_groups(x, t, c, uncond_scale, uncond_cond, prep)
        if groups == 1:
            return epsg
        if self.guidance_rescale != 0.0:
            return self._rescale(epsg.contiguous(), groups, scales)
        e_t = torch.empty_like(epsg[: x.shape[0]])   # eps has out_channels; x may carry extra cond_concat channels
        if groups == 2:
            _lib.check(self._lib.pf_cfg_combine(epsg.data_ptr(), scales[0], e_t.data_ptr(), e_t.numel(), _lib.current_stream()), "pf_cfg_combine")
        else:
            _lib.check(self._lib.pf_cfg_combine3(epsg.data_ptr(), scales[0], scales[1], e_t.data_ptr(), e_t.numel(), _lib.current_stream()),
                       "pf_cfg_combine3")
        return e_t

    def _rescale(self, epsg, groups, scales):
        e_t, stats, weights = _steps.cfg_rescale(self._lib, epsg, groups, scales, self.guidance_rescale, want_stats=True)
        self.last_rescale = (stats, weights)
        return e_t

    def _eps_groups(self, x, t, c, uncond_scale, uncond_cond, prep):
        """The denoiser on what ``guidance_plan`` decides: ``(eps of every group stacked group-major, groups, combine arguments)``."""
        kw = self._prep_kw(prep)
        # the context is re-concatenated on every call like the reference (sampler/__init__.py:69-74): [2B,n_cond,d_cond] is a few KB, and a
        # cache keyed on addresses could serve a stale tensor after an in-place update or an allocator address reuse
        ctx, groups, scales = guidance_plan(c, uncond_scale, uncond_cond)
        if groups == 1:
            return self.model(x, t, ctx, **kw), 1, scales
        tg = torch.cat([t] * groups)
        if self.share_cfg_prefix and getattr(self.model, "supports_shared_x", False):
            # the groups see the same x and t and differ only in the condition, which enters the UNet at its first transformer
            # block: everything in front of it is evaluated once for all (UNetModel.forward(shared_x=), pf_unet_forward_cfg / _cfgn)
            epsg = self.model(x, tg, ctx, shared_x=True if groups == 2 else groups, **kw)
        else:
            epsg = self.model(torch.cat([x] * groups), tg, ctx, **kw)
        return epsg, groups, scales

    def _eps_rows(self, x) -> int:
        """Rows of the batch the denoiser sees for ``x``: its own, or one per window of every song under a window plan."""
        wp = getattr(self, "windows", None)
        return x.shape[0] * (1 if wp is None else wp.n_windows)

    def _window_weights(self, wp: WindowPlan, device) -> torch.Tensor:
        key = ("window_weights", wp.key, str(device))
        if key not in self._dev_cache:
            self._dev_cache[key] = torch.from_numpy(wp.weights()).to(device)
        return self._dev_cache[key]

    def _get_eps_windows(self, wp: WindowPlan, x, t, c, uncond_scale, uncond_cond, prep):
        x = x.contiguous()
        S, rows = x.shape[0], x.shape[0] * wp.n_windows
        if x.dim() != 4 or x.shape[2] != wp.canvas_h:
            raise ValueError(f"get_eps: x of shape {tuple(x.shape)} is not a canvas of {wp.canvas_h} rows ({wp.n_windows} windows of "
                             f"{wp.win_h}, stride {wp.stride})")
        if c.shape[0] != rows or t.shape[0] != rows or (uncond_cond is not None and uncond_cond.shape[0] != rows):
            raise ValueError(f"get_eps: {S} songs of {wp.n_windows} windows need {rows} rows of t, cond and uncond_cond, got {t.shape[0]}, "
                             f"{c.shape[0]}" + ("" if uncond_cond is None else f", {uncond_cond.shape[0]}"))
        xw = _steps.window_split(self._lib, x, wp.n_windows, wp.stride, wp.win_h)
        epsg, groups, scales = self._eps_groups(xw, t, c, uncond_scale, uncond_cond, prep)
        if groups > 1 and self.guidance_rescale != 0.0:
            # the statistics are those of one WINDOW's eps, not of the canvas: the combine runs on the window batch, the merge is then plain
            epsg, groups, scales = self._rescale(epsg.contiguous(), groups, scales), 1, ()
        return _steps.window_merge(self._lib, epsg.contiguous(), self._window_weights(wp, x.device), S, wp.n_windows, wp.stride, groups, scales)

    def _t_of(self, step: int, batch: int, device) -> torch.Tensor:
        """[batch] int64 on the device, all == step: a row of a constant [n_steps, batch] table (no fill launch per step)."""
        tr = self._trows
        if tr is None or tr.shape[1] != batch or tr.device != device:
            tr = self._trows = torch.arange(self.model.n_steps + 1, dtype=torch.long, device=device).unsqueeze(1).repeat(1, batch).contiguous()
        return tr[int(step)]

    def _eps(self, x, c, step, uncond_scale, uncond_cond, cond_concat, prep=None):
        t = self._t_of(step, self._eps_rows(x), x.device)
        xin = x if cond_concat is None else torch.cat([x, cond_concat], dim=1)
        return self.get_eps(xin, t, c, uncond_scale=uncond_scale, uncond_cond=uncond_cond, prep=prep, t_value=int(step))

    def _rng_ok(self, x, *others) -> bool:
        """The in-kernel noise path: on-device generator, whole Philox groups per tensor and per shard, and every tensor the
        update kernel reads as 16-byte vectors (x and, when present, orig / orig_noise / mask) 16-byte aligned - anything else takes
        the randn() + step path, which reads 4-byte elements.  BOTH paths read their tensors as dense buffers through raw pointers: the
        callers (``_step``, ``repaint_step``, ``p_sample``) make every tensor contiguous before they get here."""
        if self.noise_fn is not None or x.numel() % 4 != 0 or self._elem_offset(x.shape) % 4 != 0:
            return False
        return all(v is None or (v.is_contiguous() and v.data_ptr() % 16 == 0) for v in (x,) + others)


    # ---- a path between two songs (not in the reference) -------------------------------------------------------------------------------
    def morph_noise(self, xa: torch.Tensor, xb: torch.Tensor, fracs):
        """``len(fracs)`` noises on the great circle from ``xa`` to ``xb``, one circle per batch entry (a ``WindowPlan`` canvas is one row):
        ``(x [K, rows, ...], stats [rows, 3] float64, weights [K, rows, 2] float32)``, all on the device (``pf_slerp_rows``, mode slerp).
        A linear mix of two Gaussian noises has the wrong norm (``sqrt((1 - t)^2 + t^2)`` of it at an angle of pi / 2); this one keeps it."""
        return _steps.slerp_rows(self._lib, xa, xb, fracs, mode="slerp")

    def morph_cond(self, ca: torch.Tensor, cb: torch.Tensor, fracs, how: str = "lerp") -> torch.Tensor:
        """The conditions of the frames, ``[K, rows, n_cond, d_cond]``: ``lerp`` - ``(1 - t)*ca + t*cb`` on the encoded conditions (mode lerp
        of the same kernel; ``t = 0`` and ``t = 1`` are copies); ``switch`` - ``ca`` where ``t < 0.5``, else ``cb``."""
        if how not in MORPH_CONDS:
            raise ValueError(f"morph_cond: how {how!r}, expected one of {MORPH_CONDS}")
        if ca.shape != cb.shape:
            raise ValueError(f"morph_cond: conditions of shapes {tuple(ca.shape)} and {tuple(cb.shape)}")
        if how == "lerp":
            return _steps.slerp_rows(self._lib, ca, cb, fracs, mode="lerp", want_stats=False)[0]
        ca, cb = ca.contiguous().float(), cb.contiguous().float()
        return torch.stack([ca if float(t) < 0.5 else cb for t in fracs])

    def _morph_refusal(self) -> Optional[str]:
        """Why this sampler has no morph, or ``None``.  A loop that draws noise maps neighbouring starts to unrelated images."""
        return f"{type(self).__name__} draws noise in every step: the frames of such a loop are not a path (use DDIMSampler with eta 0 or DPMSolverSampler)"

    def _morph_paint(self, xs, cs, t_start: int, batch: int, uncond_scale, uncond_cond, cond_concat) -> torch.Tensor:
        """``paint`` of the ``K * R`` starts ``xs [K, R, ...]`` under the conditions ``cs [K, Rc, ...]`` (``Rc = R``, or ``R`` times the windows
        of the plan), frame-major, at most ``batch`` rows of ``xs`` per call; ``uncond_cond`` ``[Rc, ...]`` and ``cond_concat`` ``[R, ...]`` are
        those of one frame.  Returns ``[K, R, C, H, W]``."""
        K, R = xs.shape[0], xs.shape[1]
        per = cs.shape[1] // R                                  # condition rows per row of x
        tile = lambda v: None if v is None else v.repeat(K, *([1] * (v.dim() - 1))).contiguous()
        x, c, uc, cc = xs.reshape(K * R, *xs.shape[2:]), cs.reshape(K * cs.shape[1], *cs.shape[2:]), tile(uncond_cond), tile(cond_concat)
        cut = lambda v, i0, i1, m=1: None if v is None else v[i0 * m: i1 * m].contiguous()
        outs = [self.paint(cut(x, i, min(i + batch, K * R)), cut(c, i, min(i + batch, K * R), per), t_start, uncond_scale=uncond_scale,
                           uncond_cond=cut(uc, i, min(i + batch, K * R), per), cond_concat=cut(cc, i, min(i + batch, K * R)))
                for i in range(0, K * R, batch)]
        out = outs[0] if len(outs) == 1 else torch.cat(outs)
        return out.reshape(K, R, *out.shape[1:])

    def _morph_conds(self, cond_a, cond_b, fracs, cond_how, conds, rows: int) -> torch.Tensor:
        K = len(fracs)
        if conds is None:
            conds = self.morph_cond(cond_a, cond_b, fracs, cond_how)
        else:
            conds = conds.contiguous().float()
            if conds.numel() != K * cond_a.numel():
                raise ValueError(f"morph: conds of shape {tuple(conds.shape)} for {K} frames of conditions of shape {tuple(cond_a.shape)}")
            conds = conds.reshape(K, *cond_a.shape)
        if conds.shape[1] % rows != 0:
            raise ValueError(f"morph: {conds.shape[1]} condition rows for {rows} rows of x")
        return conds

    @torch.no_grad()
    def morph_from_noise(self, shape, cond_a, cond_b, frames: int = 5, *, t_start: Optional[int] = None, ease: str = "linear",
                         cond_how: str = "lerp", conds=None, uncond_scale: Scale = 1.0, uncond_cond=None, cond_concat=None, batch: int = 16):
        """A path between two GENERATED songs: the end noises are two fresh draws of this sampler's own generator (``shape`` each), the
        frames between them ``morph_noise`` / ``morph_cond`` at ``morph_fractions(frames, ease)``, every frame painted from ``t_start``
        (default: the whole grid) - the rest as ``DDIMSampler.morph``.  For deterministic loops only: ``DDIMSampler`` with eta 0 and
        ``DPMSolverSampler``; anything else is a ``ValueError``.  Returns ``[K, R, C, H, W]`` and leaves ``self.last_morph``."""
        why = self._morph_refusal()
        if why is not None:
            raise ValueError(f"morph_from_noise: {why}")
        fracs = morph_fractions(frames, ease)
        t_start = len(self.time_steps) - 1 if t_start is None else int(t_start)
        if int(batch) < 1:
            raise ValueError(f"morph: batch {batch} < 1")
        xa, xb = self.randn(shape, cond_a.device), self.randn(shape, cond_a.device)
        xs, stats, weights = self.morph_noise(xa, xb, fracs)
        cs = self._morph_conds(cond_a, cond_b, fracs, cond_how, conds, xa.shape[0])
        self.last_morph = MorphRecord(fracs, stats, weights, None, (xa, xb))
        return self._morph_paint(xs, cs, t_start, int(batch), uncond_scale, uncond_cond, cond_concat)


MORPH_EASES = ("linear", "cosine")
MORPH_CONDS = ("lerp", "switch")


def morph_fractions(frames: int, ease: str = "linear") -> np.ndarray:
    """float64 ``[frames]``: where the frames of a morph sit between song A (0) and song B (1), the endpoints included.  ``linear``:
    ``k / (frames - 1)``; ``cosine``: ``(1 - cos(pi * k / (frames - 1))) / 2`` - slow at both ends.  One frame sits in the middle."""
    frames = int(frames)
    if ease not in MORPH_EASES:
        raise ValueError(f"morph_fractions: ease {ease!r}, expected one of {MORPH_EASES}")
    if not 1 <= frames <= _lib.SLERP_MAX_FRAMES:
        raise ValueError(f"morph_fractions: {frames} frames outside [1, {_lib.SLERP_MAX_FRAMES}]")
    if frames == 1:
        return np.asarray([0.5], dtype=np.float64)
    lin = np.arange(frames, dtype=np.float64) / (frames - 1)
    if ease == "cosine":
        # libm's cos, one value at a time: numpy's vectorised cos may differ in the last bit from host to host.  cos(0) and cos(pi) are
        # exact, so the end points are 0 and 1
        lin = np.asarray([(1.0 - math.cos(math.pi * float(v))) / 2.0 for v in lin], dtype=np.float64)
    return lin


@dataclass
class MorphRecord:
    """What a morph leaves behind without a host sync: ``fractions`` (host float64 ``[K]``), the device tables of ``pf_slerp_rows`` -
    ``stats`` float64 ``[rows, 3]`` (sum a*a, a*b, b*b of the two end noises per row) and ``weights`` float32 ``[K, rows, 2]`` -, the
    ``InversionRecord`` of the upward walk (rows: A's, then B's; ``None`` for ``morph_from_noise``) and the two end noises."""
    fractions: np.ndarray
    stats: torch.Tensor
    weights: torch.Tensor
    inversion: Optional["InversionRecord"] = None
    end_noises: Optional[tuple] = None

    def angles(self) -> np.ndarray:
        """The angle between the two end noises of every row, radians, as numpy ``[rows]`` (copies the table: the one host sync)."""
        s = self.stats.detach().cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.arccos(np.clip(s[:, 1] / np.sqrt(s[:, 0] * s[:, 2]), -1.0, 1.0))


class SDFSampler(DiffusionSampler):
    def __init__(self, model: LatentDiffusion, is_show_image: bool = False, **kw):
        super().__init__(model, **kw)
        self.time_steps = np.asarray(list(range(self.n_steps)), dtype=np.int32)
        self.is_show_image = is_show_image
        ab, beta = model.alpha_bar, model.beta  # fp32 host tensors
        ab_prev = torch.cat([ab.new_tensor([1.0]), ab[:-1]])
        self.sqrt_alpha_bar = ab ** 0.5
        self.sqrt_1m_alpha_bar = (1.0 - ab) ** 0.5
        self.sqrt_recip_alpha_bar = ab ** -0.5
        self.sqrt_recip_m1_alpha_bar = (1 / ab - 1) ** 0.5
        variance = beta * (1.0 - ab_prev) / (1.0 - ab)
        self.log_var = torch.log(torch.clamp(variance, min=1e-20))
        self.mean_x0_coef = beta * (ab_prev ** 0.5) / (1.0 - ab)
        self.mean_xt_coef = (1.0 - ab_prev) * ((1 - beta) ** 0.5) / (1.0 - ab)
        self._sigma = (0.5 * self.log_var).exp()

    def _coef_table(self, device) -> torch.Tensor:
        """[n_steps, 7] fp32 on the device: row t = the pf_ddpm_coef of step t (same floats `_coef` passes by value)."""
        key = ("ddpm_table", str(device))
        if key not in self._dev_cache:
            rows = torch.stack([self.sqrt_recip_alpha_bar, self.sqrt_recip_m1_alpha_bar, self.mean_x0_coef, self.mean_xt_coef,
                                self._sigma, self.sqrt_alpha_bar, self.sqrt_1m_alpha_bar], dim=1).to(torch.float32).contiguous()
            self._dev_cache[key] = rows.to(device)
        return self._dev_cache[key]

    def _paint_graph(self, x, cond, t_start, orig, mask, uncond_scale, uncond_cond, cond_concat):
        """Steps t_start .. 1 as replays of one captured step; returns x_1 (the caller runs step 0, which draws no noise)."""
        lib, off, rng = self._lib, self._elem_offset(x.shape), self._rng_ok(x)
        ndraw = 2 if orig is not None else 1

        def update(bf, e_t, table, st):
            xb, known = bf["x"], dict(orig=bf["orig"], mask=bf["mask"])
            if rng:   # both draws inside the update kernel (draw order of the reference: known-region noise, then the p_sample noise)
                _steps.ddpm_step(lib, xb, e_t, xb, table=table, state=st, rng=(self.seed, 0, 0, off), **known)
                return
            nq = None if orig is None else _steps.randn_dev(lib, bf["_noise"][0], self.seed, st, 0, off)
            npz = _steps.randn_dev(lib, bf["_noise"][-1], self.seed, st, ndraw - 1, off)
            _steps.ddpm_step(lib, xb, e_t, xb, table=table, state=st, noise_p=npz, noise_q=nq, **known)

        inputs = dict(x=x, cond=cond, orig=orig, mask=mask, uncond_cond=uncond_cond, cond_concat=cond_concat)
        return self._replay_loop("ddpm", inputs, self._coef_table(x.device), None, ndraw, 0 if rng else ndraw, t_start, t_start, uncond_scale, update)

    def _coef(self, step: int) -> _lib.DdpmCoef:
        return _lib.DdpmCoef(float(self.sqrt_recip_alpha_bar[step]), float(self.sqrt_recip_m1_alpha_bar[step]),
                             float(self.mean_x0_coef[step]), float(self.mean_xt_coef[step]), float(self._sigma[step]),
                             float(self.sqrt_alpha_bar[step]), float(self.sqrt_1m_alpha_bar[step]))

    @torch.no_grad()
    def p_sample(self, x, c, t, step: int, repeat_noise: bool = False, temperature: float = 1.0,
                 uncond_scale: float = 1.0, uncond_cond=None, cond_concat=None, return_x0: bool = True, prep: Optional[dict] = None):
        """Returns (x_prev, x0, e_t) like the reference (sampler_sdf.py:80-171).  ``x0`` costs two extra elementwise
        launches; the loops of this class (``sample`` / ``paint``) pass ``return_x0=False`` and get ``None`` for it.
        ``prep``: the result of ``prepare(c, uncond_scale=, uncond_cond=)`` when the caller hoisted it."""
        step = int(step)
        x = x.contiguous()
        e_t = self._eps(x, c, step, uncond_scale, uncond_cond, cond_concat, prep)
        return self._update(x, e_t, step, repeat_noise, temperature, return_x0)

    def _update(self, x, e_t, step: int, repeat_noise: bool = False, temperature: float = 1.0, return_x0: bool = False):
        """What ``p_sample`` does with its eps: ``(x_prev, x0, e_t)``.  A steered loop calls it on the resampled ``x`` and eps."""
        coef = self._coef(step)
        x_prev = torch.empty_like(x)
        if step != 0 and not repeat_noise and temperature == 1.0 and self._rng_ok(x):
            # the draw happens inside the update kernel: same values as randn() + the tensor form, one launch
            _steps.ddpm_step(self._lib, x, e_t, x_prev, coef=coef, rng=(self.seed, 0, self._draws, self._elem_offset(x.shape)))
            self._draws += 1
            x0 = (coef.c_recip * x - coef.c_recipm1 * e_t) if return_x0 else None
            return x_prev, x0, e_t
        noise = None
        if step != 0:
            noise = self.randn((1, *x.shape[1:]) if repeat_noise else x.shape, x.device)
            if repeat_noise:
                noise = noise.expand_as(x).contiguous()
            if temperature != 1.0:
                noise = noise * temperature
        _steps.ddpm_step(self._lib, x, e_t, x_prev, coef=coef, noise_p=noise)
        x0 = (coef.c_recip * x - coef.c_recipm1 * e_t) if return_x0 else None
        return x_prev, x0, e_t

    @torch.no_grad()
    def q_sample(self, x0: torch.Tensor, index: int, noise: Optional[torch.Tensor] = None):
        return _steps.q_sample(self, x0, noise, self.sqrt_alpha_bar[index], self.sqrt_1m_alpha_bar[index], self._elem_offset(x0.shape))

    @torch.no_grad()
    def sample(self, shape: List[int], cond, repeat_noise=False, temperature=1.0, x_last=None, uncond_scale=1.0,
               uncond_cond=None, t_start: int = 0):
        x = x_last if x_last is not None else self.randn(shape, cond.device)
        prep = self.prepare(cond, uncond_scale=uncond_scale, uncond_cond=uncond_cond)
        for step in np.flip(self.time_steps)[t_start:]:
            x, _, _ = self.p_sample(x, cond, None, int(step), repeat_noise=repeat_noise, temperature=temperature,
                                    uncond_scale=uncond_scale, uncond_cond=uncond_cond, return_x0=False, prep=prep)
        return x

    def repaint_step(self, x_t, cond, step: int, orig, mask, *, uncond_scale: float = 1.0, uncond_cond=None, cond_concat=None,
                     prep: Optional[dict] = None):
        """ONE iteration of ``paint``'s loop body with a known region (sampler_sdf.py:307-336): eps, the reverse step on the unknown
        region, the forward-noised known region, the blend.  Two noise draws for step > 0 - known-region noise first, then the
        ``p_sample`` noise, the reference's order - made inside the update kernel when the on-device generator is in use.
        ``bench.py`` times exactly this method."""
        step = int(step)
        x_t, orig, mask = x_t.contiguous(), orig.contiguous(), mask.contiguous()     # the update kernels read dense buffers
        e_t = self._eps(x_t, cond, step, uncond_scale, uncond_cond, cond_concat, prep)
        return self._repaint_update(x_t, e_t, step, orig, mask)

    def _repaint_update(self, x_t, e_t, step: int, orig, mask):
        """What ``repaint_step`` does with its eps.  A steered loop calls it on the resampled ``x_t`` and eps."""
        lib, coef = self._lib, self._coef(step)
        x = torch.empty_like(x_t)
        if step > 0 and self._rng_ok(x_t, orig, mask):
            _steps.ddpm_step(lib, x_t, e_t, x, coef=coef, orig=orig, mask=mask,
                             rng=(self.seed, self._draws, self._draws + 1, self._elem_offset(x_t.shape)))
            self._draws += 2
            return x
        # injected noise tape (parity tests) / step 0: the draws are tensors.  The tape's order is the reference's: q before the eps
        # evaluation, p after it - randn() only counts draws, so drawing both here keeps the tape aligned
        noise_q = self.randn(orig.shape, x_t.device) if step > 0 else None
        noise_p = self.randn(x_t.shape, x_t.device) if step > 0 else None
        return _steps.ddpm_step(lib, x_t, e_t, x, coef=coef, noise_p=noise_p, noise_q=noise_q, orig=orig, mask=mask)

    @torch.no_grad()
    def paint(self, x, cond, t_start: int, orig=None, mask=None, orig_noise=None, uncond_scale: float = 1.0,
              uncond_cond=None, cond_concat=None, repaint_n: int = 1):
        """RePaint-style loop.  ``orig_noise`` is ignored exactly like the reference (fresh noise per step)."""
        x = x.contiguous()
        if orig is not None:
            assert mask is not None
            orig, mask = orig.contiguous().float(), mask.contiguous().float()
        steps = np.flip(self.time_steps[: t_start + 1])
        if self.graph and self.noise_fn is None and repaint_n == 1 and t_start >= 1 and self.on_step is None:
            x = self._paint_graph(x, cond, int(t_start), orig, mask, uncond_scale, uncond_cond, cond_concat)
            steps = steps[-1:]          # step 0 (no noise) runs eagerly below
        # everything the denoiser derives from (t, cond) alone, once for the whole loop
        prep = self.prepare(cond, uncond_scale=uncond_scale, uncond_cond=uncond_cond)
        steer = self._steer_begin(x, repaint_n)
        for i, step in enumerate(steps):
            step = int(step)
            if steer is not None:
                # eps with everything get_eps applies, then - at a steered step - the population resampled, then the unchanged update
                e_t = self._eps(x, cond, step, uncond_scale, uncond_cond, cond_concat, prep)
                if self._steered_at(steer, i, step, i == len(steps) - 1):
                    x, e_t = self._steer_event(steer, x, e_t, self._t_of(step, self._eps_rows(x), x.device), i, step)
                x = self._update(x, e_t, step)[0] if orig is None else self._repaint_update(x, e_t, step, orig, mask)
                if self.on_step is not None:
                    self.on_step(step, x)
                continue
            if orig is None:
                x, _, _ = self.p_sample(x, cond, None, step, uncond_scale=uncond_scale, uncond_cond=uncond_cond,
                                        cond_concat=cond_concat, return_x0=False, prep=prep)
                if self.on_step is not None:
                    self.on_step(step, x)
                continue
            x_t = x
            for u in range(repaint_n):
                x = self.repaint_step(x_t, cond, step, orig, mask, uncond_scale=uncond_scale, uncond_cond=uncond_cond,
                                      cond_concat=cond_concat, prep=prep)
                if u < repaint_n - 1 and step > 0:
                    noise = self.randn(orig.shape, x.device)
                    b = self.model.beta[step - 1]
                    x_t = _steps.axpby(self._lib, x, noise, (1 - b) ** 0.5, b)
            if self.on_step is not None:
                self.on_step(step, x)
        return x


class DDIMSampler(DiffusionSampler):
    def __init__(self, model: LatentDiffusion, n_steps: int, ddim_discretize: str = "uniform", ddim_eta: float = 0.0,
                 is_show_image: bool = False, **kw):
        super().__init__(model, **kw)
        self.is_show_image = is_show_image
        self.n_steps = model.n_steps
        if ddim_discretize == "uniform":
            c = self.n_steps // n_steps
            self.time_steps = np.asarray(list(range(0, self.n_steps, c))) + 1
        elif ddim_discretize == "quad":
            self.time_steps = ((np.linspace(0, np.sqrt(self.n_steps * 0.8), n_steps)) ** 2).astype(int) + 1
        else:
            raise NotImplementedError(ddim_discretize)
        ab = model.alpha_bar
        self.ddim_alpha = ab[self.time_steps].clone().to(torch.float32)
        self.ddim_alpha_sqrt = torch.sqrt(self.ddim_alpha)
        self.ddim_alpha_prev = torch.cat([ab[0:1], ab[self.time_steps[:-1]]])
        self.ddim_sigma = (ddim_eta * ((1 - self.ddim_alpha_prev) / (1 - self.ddim_alpha)
                                       * (1 - self.ddim_alpha / self.ddim_alpha_prev)) ** 0.5)
        self.ddim_sqrt_one_minus_alpha = (1.0 - self.ddim_alpha) ** 0.5
        self.steering = self.steering         # (checked again now that the sampler knows its eta)

    def _steer_refusal(self) -> Optional[str]:
        if getattr(self, "ddim_sigma", None) is not None and not bool((self.ddim_sigma != 0).any()):
            return "DDIMSampler with ddim_eta == 0 draws no noise: copies of a survivor would never diverge (use eta > 0 or SDFSampler)"
        return super()._steer_refusal()

    def _coef_table(self, device):
        """([S, 7] fp32 coefficient rows, [S] int32 tau table) on the device - the floats `_coef` passes by value."""
        key = ("ddim_table", str(device))
        if key not in self._dev_cache:
            rows = torch.tensor([[getattr(c, f) for f, _ in _lib.DdimCoef._fields_] for c in map(self._coef, range(len(self.time_steps)))],
                                dtype=torch.float32)
            self._dev_cache[key] = (rows.to(device), torch.from_numpy(np.asarray(self.time_steps, dtype=np.int32)).to(device))
        return self._dev_cache[key]

    def _paint_graph(self, x, cond, t_start, orig, mask, orig_noise, uncond_scale, uncond_cond, cond_concat, noisy: bool):
        """All t_start+1 steps of a DDIM loop as replays of one captured step.  ``noisy``: every step of the range has sigma != 0
        (eta > 0) and draws one noise tensor, in the eager loop's draw order; otherwise (eta = 0) no step draws."""
        lib, off = self._lib, self._elem_offset(x.shape)
        rng = noisy and self._rng_ok(x)

        def update(bf, e_t, table, st):
            xb, known = bf["x"], dict(orig=bf["orig"], orig_noise=bf["orig_noise"], mask=bf["mask"])
            if rng:
                _steps.ddim_step(lib, xb, e_t, xb, table=table, state=st, rng=(self.seed, 0, off), **known)
                return
            nz = _steps.randn_dev(lib, bf["_noise"][0], self.seed, st, 0, off) if noisy else None
            _steps.ddim_step(lib, xb, e_t, xb, table=table, state=st, noise=nz, **known)

        inputs = dict(x=x, cond=cond, orig=orig, mask=mask, orig_noise=orig_noise, uncond_cond=uncond_cond, cond_concat=cond_concat)
        table, taus = self._coef_table(x.device)
        return self._replay_loop("ddim", inputs, table, taus, int(noisy), int(noisy and not rng), t_start + 1, t_start, uncond_scale, update)

    def _coef(self, index: int) -> _lib.DdimCoef:
        a, ap, sg = self.ddim_alpha[index], self.ddim_alpha_prev[index], self.ddim_sigma[index]
        return _lib.DdimCoef(float(self.ddim_sqrt_one_minus_alpha[index]), float(a ** 0.5), float(ap ** 0.5),
                             float((1.0 - ap - sg ** 2).sqrt()), float(sg), float(self.ddim_alpha_sqrt[index]),
                             float(self.ddim_sqrt_one_minus_alpha[index]))

    def _step(self, x, e_t, index, orig=None, orig_noise=None, mask=None, temperature=1.0, repeat_noise=False):
        coef = self._coef(index)
        noise = None
        # both kernel paths below read x / e_t / orig / orig_noise / mask as dense buffers
        x, e_t = x.contiguous(), e_t.contiguous()
        orig, orig_noise, mask = (None if v is None else v.contiguous() for v in (orig, orig_noise, mask))
        noisy = float(self.ddim_sigma[index]) != 0.0
        if noisy and not repeat_noise and temperature == 1.0 and self._rng_ok(x, e_t, orig, orig_noise, mask):
            # the step's draw happens inside the update kernel (same values as randn() + the tensor form)
            draw = self._draws
            self._draws += 1
            if orig is not None and orig_noise is None:   # reference: a fresh q_sample noise per step, drawn after p_sample's
                orig_noise = self.randn(orig.shape, x.device)
            out = torch.empty_like(x)
            _steps.ddim_step(self._lib, x, e_t, out, coef=coef, rng=(self.seed, draw, self._elem_offset(x.shape)),
                             orig=orig, orig_noise=orig_noise, mask=mask)
            return out, coef
        if noisy:
            noise = self.randn((1, *x.shape[1:]) if repeat_noise else x.shape, x.device)
            if repeat_noise:
                noise = noise.expand_as(x).contiguous()
            if temperature != 1.0:
                noise = noise * temperature
        if orig is not None and orig_noise is None:
            # reference: q_sample(orig, index, noise=None) draws randn_like per step, after p_sample's draw (sampler_ddim.py:355-359)
            orig_noise = self.randn(orig.shape, x.device)
        out = torch.empty_like(x)
        return _steps.ddim_step(self._lib, x, e_t, out, coef=coef, noise=noise, orig=orig, orig_noise=orig_noise, mask=mask), coef

    @torch.no_grad()
    def get_x_prev_and_pred_x0(self, e_t, index: int, x, *, temperature: float = 1.0, repeat_noise: bool = False):
        x_prev, coef = self._step(x.contiguous(), e_t.contiguous(), index, temperature=temperature, repeat_noise=repeat_noise)
        pred_x0 = (x - coef.s1m * e_t) / coef.sqrt_a
        return x_prev, pred_x0

    @torch.no_grad()
    def p_sample(self, x, c, t, step: int, index: int, *, repeat_noise=False, temperature=1.0, uncond_scale=1.0,
                 uncond_cond=None, cond_concat=None, prep: Optional[dict] = None):
        e_t = self._eps(x, c, int(step), uncond_scale, uncond_cond, cond_concat, prep)
        x_prev, pred_x0 = self.get_x_prev_and_pred_x0(e_t, index, x, temperature=temperature, repeat_noise=repeat_noise)
        return x_prev, pred_x0, e_t

    @torch.no_grad()
    def q_sample(self, x0, index: int, noise=None):
        return _steps.q_sample(self, x0, noise, self.ddim_alpha_sqrt[index], self.ddim_sqrt_one_minus_alpha[index], self._elem_offset(x0.shape))

    @torch.no_grad()
    def sample(self, shape, cond, repeat_noise=False, temperature=1.0, x_last=None, uncond_scale=1.0, uncond_cond=None,
               t_start: int = 0):
        x = x_last if x_last is not None else self.randn(shape, cond.device)
        time_steps = np.flip(self.time_steps)[t_start:]
        prep = self.prepare(cond, uncond_scale=uncond_scale, uncond_cond=uncond_cond)
        for i, step in enumerate(time_steps):
            index = len(time_steps) - i - 1
            e_t = self._eps(x, cond, int(step), uncond_scale, uncond_cond, None, prep)
            x, _ = self._step(x, e_t, index, temperature=temperature, repeat_noise=repeat_noise)
        return x

    @torch.no_grad()
    def paint(self, x, cond, t_start: int, *, orig=None, mask=None, orig_noise=None, uncond_scale: float = 1.0,
              uncond_cond=None, cond_concat=None, repaint_n: int = 1):
        x = x.contiguous()
        if orig is not None:
            assert mask is not None
            orig, mask = orig.contiguous().float(), mask.contiguous().float()
            orig_noise = None if orig_noise is None else orig_noise.contiguous().float()
        time_steps = np.flip(self.time_steps[: t_start + 1])
        if self.graph and self.noise_fn is None and (orig is None or orig_noise is not None) and self.on_step is None:
            nonzero = self.ddim_sigma[: t_start + 1] != 0
            if not bool(nonzero.any()) or bool(nonzero.all()):    # a mixed range would need a per-step decision on the host
                return self._paint_graph(x, cond, int(t_start), orig, mask, orig_noise, uncond_scale, uncond_cond, cond_concat,
                                         noisy=bool(nonzero.all()))
        prep = self.prepare(cond, uncond_scale=uncond_scale, uncond_cond=uncond_cond)
        steer = self._steer_begin(x, repaint_n)
        for i, step in enumerate(time_steps):
            index = len(time_steps) - i - 1
            e_t = self._eps(x, cond, int(step), uncond_scale, uncond_cond, cond_concat, prep)
            if steer is not None and self._steered_at(steer, i, int(step), index == 0):
                x, e_t = self._steer_event(steer, x, e_t, self._t_of(int(step), self._eps_rows(x), x.device), i, int(step))
            # x_prev and the known-region blend (fixed orig_noise, sampler_ddim.py:355-359) in one kernel
            x, _ = self._step(x, e_t, index, orig=orig, orig_noise=orig_noise, mask=mask)
            if self.on_step is not None:
                self.on_step(int(step), x)
        return x


    # ---- exact inversion of the eta = 0 loop (not in the reference) -------------------------------------------------------------
    def invert_rows(self) -> np.ndarray:
        """float32 ``[len(time_steps), 2]``: ``invert_coef_rows`` of this sampler's own float32 tables, rounded once."""
        if getattr(self, "_inv_rows", None) is None:
            self._inv_rows = invert_coef_rows(self.ddim_alpha.numpy(), self.ddim_alpha_prev.numpy()).astype(np.float32)
        return self._inv_rows

    def _invert_table(self, device):
        """([S, 2] fp32 rows, [S] int32 tau table) on the device: row i = the pf_invert_coef of upward step i."""
        key = ("invert_table", str(device))
        if key not in self._dev_cache:
            self._dev_cache[key] = (torch.from_numpy(self.invert_rows()).to(device), self._coef_table(device)[1])
        return self._dev_cache[key]

    def _invert_graph(self, x, cond, t_end, iters, resid, uncond_scale, uncond_cond, cond_concat):
        """Steps 0 .. t_end as replays of ONE captured upward step {begin, iters x (eps, iterate), advance}.  The iterate lives in the
        static x buffer (x_iter = x_out), the step's lower state y in a second one that every replay first refills from x."""
        lib = self._lib
        table, taus = self._invert_table(x.device)

        def body_of(bf, tb, st):
            yb = bf["_y"] = torch.empty_like(bf["x"])
            ws = bf["_ws"] = _steps.invert_workspace(lib, yb.shape[0], yb.numel() // yb.shape[0], yb.device)

            def body():
                _lib.check(lib.pf_step_begin(st.data_ptr(), taus.data_ptr(), tb.data_ptr(), tb.numel(), _lib.current_stream()), "pf_step_begin")
                yb.copy_(bf["x"])
                for k in range(iters):
                    cur = yb if k == 0 else bf["x"]
                    xin = cur if bf["cond_concat"] is None else torch.cat([cur, bf["cond_concat"]], dim=1)
                    e_t = self.get_eps(xin, tb, bf["cond"], uncond_scale=uncond_scale, uncond_cond=bf["uncond_cond"], prep=bf["_prep"])
                    _steps.invert_step(lib, yb, e_t.contiguous(), bf["x"], table=table, state=st, x_iter=None if k == 0 else bf["x"],
                                       resid=bf["resid"], workspace=ws, iters=iters, k=k)
                _lib.check(lib.pf_step_advance(st.data_ptr(), 1, 0, _lib.current_stream()), "pf_step_advance")
            return body

        inputs = dict(x=x, cond=cond, uncond_cond=uncond_cond, cond_concat=cond_concat, resid=resid)
        out = self._replay_loop(("ddim_invert", int(iters)), inputs, table, taus, 0, 0, t_end + 1, 0, uncond_scale, None, body_of=body_of)
        return out, self._last_bufs["resid"].clone()      # the static table is overwritten by the next call with these shapes

    @torch.no_grad()
    def invert(self, x0, cond, t_end: Optional[int] = None, *, iters: int = 3, uncond_scale: Scale = 1.0, uncond_cond=None, cond_concat=None,
               keep_iterates: bool = False):
        """Walk the eta = 0 DDIM ODE UPWARDS from ``x0`` - taken at the level ``paint`` ends at, ``ddim_alpha_prev[0]`` - through indices
        0 .. ``t_end`` (default: the last) to the noise ``x`` that ``paint(x, cond, t_end)`` brings back to ``x0``; a different ``cond`` in
        that ``paint`` edits the image.  Step i goes from ``ddim_alpha_prev[i]`` to ``ddim_alpha[i]`` and is IMPLICIT: it looks for the x
        whose DDIM step lands exactly on the state below, y, by ``iters`` fixed-point iterates ``x <- c_y*y + c_e*eps(x, time_steps[i])``
        from ``x = y``, one denoiser evaluation each (``pf_invert_step``).  ``iters = 1`` is the naive explicit inversion, which falls apart
        under guidance above 1.  Everything goes through ``get_eps``: float or ``DualScale`` guidance, ``cond_concat`` and a window plan
        (``x0`` a canvas) work as in ``paint``.  ``graph=True``: one captured step replayed ``t_end + 1`` times, bit-identical to this loop.

        No host sync: the per-row sums (x_K+1 - x_K)^2 and x_K+1^2 of every iterate are left in a device table, ``self.last_inversion``
        (``.table`` float64 ``[t_end + 1, iters, rows, 2]``, ``.shape``, ``.residuals()`` -> sqrt of their ratio as numpy); the round-trip defect
        of step i after k iterates is residual k+1 over c_y.  ``keep_iterates`` (eager, for tests): every iterate in ``last_inversion.iterates[i][k]``."""
        n = len(self.time_steps)
        t_end = n - 1 if t_end is None else int(t_end)
        iters = int(iters)
        if not 0 <= t_end < n:
            raise ValueError(f"invert: t_end {t_end} outside [0, {n - 1}], the indices of this sampler's grid")
        if iters < 1:
            raise ValueError(f"invert: iters {iters} < 1 (one iterate is the explicit inversion)")
        if bool((self.ddim_sigma[: t_end + 1] != 0).any()):
            raise ValueError("invert: the loop is stochastic over this range (ddim_sigma != 0, eta > 0): only the eta = 0 ODE has an inverse")
        y = x0.contiguous().float()
        rows, dev = y.shape[0], y.device
        use_graph = self.graph and self.noise_fn is None and self.on_step is None and not keep_iterates
        # graph mode keeps one table of the whole grid's size in the captured step, so that one capture serves every t_end
        resid = torch.zeros((n if use_graph else t_end + 1), iters, rows, 2, dtype=torch.float64, device=dev)
        its = [] if keep_iterates else None
        if use_graph:
            y, full = self._invert_graph(y, cond, t_end, iters, resid, uncond_scale, uncond_cond, cond_concat)
            resid = full[: t_end + 1]
        else:
            ws = _steps.invert_workspace(self._lib, rows, y.numel() // rows, dev)
            prep = self.prepare(cond, uncond_scale=uncond_scale, uncond_cond=uncond_cond)
            rws = self.invert_rows()
            for i in range(t_end + 1):
                step, coef = int(self.time_steps[i]), _lib.InvertCoef(float(rws[i, 0]), float(rws[i, 1]))
                cur = y
                if its is not None:
                    its.append([])
                for k in range(iters):
                    e_t = self._eps(cur, cond, step, uncond_scale, uncond_cond, cond_concat, prep).contiguous()
                    out = torch.empty_like(y)
                    _steps.invert_step(self._lib, y, e_t, out, coef=coef, x_iter=None if k == 0 else cur, resid=resid, workspace=ws,
                                       slot=i * iters + k)
                    cur = out
                    if its is not None:
                        its[-1].append(out)
                y = cur
        self.last_inversion = InversionRecord(resid, (t_end + 1, iters, rows, 2), its)
        return y

    # ---- a path between two given songs (not in the reference) ------------------------------------------------------------------------------
    def _morph_refusal(self) -> Optional[str]:
        if bool((self.ddim_sigma != 0).any()):
            return "this DDIM loop is stochastic (ddim_sigma != 0, eta > 0): the frames of a loop that draws noise are not a path"
        return None

    @torch.no_grad()
    def morph(self, x0_a, cond_a, x0_b, cond_b, frames: int = 5, *, t_end: Optional[int] = None, iters: int = 3, ease: str = "linear",
              cond_how: str = "lerp", conds=None, uncond_scale: Scale = 1.0, invert_scale: Optional[Scale] = None, uncond_cond=None,
              cond_concat=None, batch: int = 16):
        """``frames`` songs on a path from ``x0_a`` to ``x0_b`` (``[R, C, H, W]`` each; canvases under a window plan): both are taken to their
        noises by ONE ``invert`` of the ``2R`` stacked rows under their own conditions (``invert_scale``: its guidance, default
        ``uncond_scale``), the noises are interpolated on the sphere (``morph_noise``) and the conditions as ``cond_how`` says (``morph_cond``;
        ``conds`` ``[K, rows of cond_a, ...]`` overrides them) at ``morph_fractions(frames, ease)``, and the ``K * R`` points are painted back
        down from ``t_end`` in batches of at most ``batch`` rows, frame-major.  ``uncond_cond`` / ``cond_concat``: those of ONE song, shaped
        like ``cond_a`` / ``x0_a``'s rows.  Everything ``invert`` and ``paint`` support carries over (float / ``DualScale`` guidance, a window
        plan, ``graph=True``), and eta != 0 is refused by ``invert``.  With a converged inversion the first and last frame are the two
        songs.  Returns ``[K, R, C, H, W]``.  No host sync: the fractions, the slerp tables and the inversion's residuals stay in
        ``self.last_morph`` (``MorphRecord``)."""
        fracs = morph_fractions(frames, ease)
        if x0_a.shape != x0_b.shape or cond_a.shape != cond_b.shape:
            raise ValueError(f"morph: songs of shapes {tuple(x0_a.shape)} / {tuple(x0_b.shape)} under conditions of shapes "
                             f"{tuple(cond_a.shape)} / {tuple(cond_b.shape)}")
        if int(batch) < 1:
            raise ValueError(f"morph: batch {batch} < 1")
        R = x0_a.shape[0]
        t_end = len(self.time_steps) - 1 if t_end is None else int(t_end)
        two = lambda v: None if v is None else torch.cat([v, v])
        x = self.invert(torch.cat([x0_a.float(), x0_b.float()]), torch.cat([cond_a, cond_b]), t_end, iters=iters,
                        uncond_scale=uncond_scale if invert_scale is None else invert_scale, uncond_cond=two(uncond_cond),
                        cond_concat=two(cond_concat))
        xs, stats, weights = self.morph_noise(x[:R], x[R:], fracs)
        cs = self._morph_conds(cond_a, cond_b, fracs, cond_how, conds, R)
        self.last_morph = MorphRecord(fracs, stats, weights, self.last_inversion, (x[:R], x[R:]))
        return self._morph_paint(xs, cs, t_end, int(batch), uncond_scale, uncond_cond, cond_concat)


@dataclass
class InversionRecord:
    """What ``DDIMSampler.invert`` leaves behind without a host sync: ``table`` - device float64 of ``shape`` ``[steps, iters, rows, 2]``, the
    row sums (x_k+1 - x_k)^2 and x_k+1^2 of every iterate; ``iterates`` - ``[step][k]`` tensors under ``keep_iterates``, else ``None``."""
    table: torch.Tensor
    shape: tuple
    iterates: Optional[list] = None

    def residuals(self) -> np.ndarray:
        """``sqrt(sum diff^2 / sum x^2)`` as numpy ``[steps, iters, rows]`` (copies the table: the one host sync)."""
        t = self.table.detach().cpu().numpy().reshape(self.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.sqrt(t[..., 0] / t[..., 1])


def invert_coef_rows(alpha, alpha_prev) -> np.ndarray:
    """float64 ``[n, 2]``: row i = ``(c_y, c_e)`` of the upward step from level ``alpha_prev[i]`` to ``alpha[i]`` (``pf_invert_coef``):
    ``c_y = sqrt(a / ap)``, ``c_e = sqrt(1 - a) - sqrt(a * (1 - ap) / ap)`` - the DDIM step with eta = 0, ``x_prev = sqrt(ap) * (x -
    sqrt(1 - a) * eps) / sqrt(a) + sqrt(1 - ap) * eps``, solved for x.  A repeated time step (``a == ap``, as on the ``quad`` grid) is the
    identity: ``(1, 0)`` exactly."""
    a, ap = np.asarray(alpha, dtype=np.float64), np.asarray(alpha_prev, dtype=np.float64)
    rows = np.stack([np.sqrt(a / ap), np.sqrt(1.0 - a) - np.sqrt(a * (1.0 - ap) / ap)], axis=1)
    rows[a == ap] = (1.0, 0.0)
    return rows


def dpm_time_steps(alpha_bar, n_steps: int, discretize: str = "logsnr") -> np.ndarray:
    """The ascending time-step grid of ``DPMSolverSampler``.  ``uniform`` / ``quad``: DDIM's arrays (sampler_ddim.py:40-55).  ``logsnr``:
    ``n_steps`` targets uniform in lambda = log(alpha / sigma) between the schedule's last and second time step, each mapped to the nearest
    time step; duplicates and time step 0 (the end point of the last step) are dropped, so the grid can be shorter than asked for."""
    ab = np.asarray(alpha_bar, dtype=np.float64)
    n = len(ab)
    if discretize == "uniform":
        return np.asarray(list(range(0, n, n // n_steps))) + 1
    if discretize == "quad":
        return ((np.linspace(0, np.sqrt(n * 0.8), n_steps)) ** 2).astype(int) + 1
    if discretize == "logsnr":
        lam = 0.5 * np.log(ab / (1.0 - ab))
        ts = {int(np.argmin(np.abs(lam - target))) for target in np.linspace(lam[n - 1], lam[1], n_steps)}
        return np.asarray(sorted(ts - {0}), dtype=np.int64)
    raise NotImplementedError(discretize)


def dpm_coef_rows(alpha_bar, time_steps, t_start: int, order: int = 2, lower_order_final: bool = True) -> np.ndarray:
    """float64 ``[t_start + 1, 7]``: row i = the ``pf_dpm_coef`` fields (s1m, sqrt_a, c_x, c_0, c_1, q_sqrt_a, q_s1m) of grid index i in a
    loop that runs i = t_start .. 0.  Step i goes from ``time_steps[i]`` to ``time_steps[i - 1]`` (to time step 0 at i = 0, as DDIM ends).
    First order (c_1 = 0): the loop's first step, ``order == 1``, a step of zero length or after one (a grid that repeats a time step), and
    the last step of a loop of fewer than 15 steps when ``lower_order_final``."""
    ab = np.asarray(alpha_bar, dtype=np.float64)
    ts = np.asarray(time_steps)[: t_start + 1]
    cur = ab[ts]
    tgt = np.concatenate([ab[0:1], ab[ts[:-1]]])
    lam = lambda a: 0.5 * np.log(a / (1.0 - a))
    h = lam(tgt) - lam(cur)
    rows = np.zeros((len(ts), 7), dtype=np.float64)
    for i in range(len(ts)):
        e = -np.sqrt(tgt[i]) * np.expm1(-h[i])                 # alpha_tgt * (1 - exp(-h))
        second = (order == 2 and i < t_start and h[i] != 0.0 and h[i + 1] != 0.0
                  and not (i == 0 and lower_order_final and len(ts) < 15))
        k = 0.5 * h[i] / h[i + 1] if second else 0.0           # 1 / (2r), r = h_{i+1} / h_i
        s1m, sqrt_a = np.sqrt(1.0 - cur[i]), np.sqrt(cur[i])
        rows[i] = (s1m, sqrt_a, np.sqrt(1.0 - tgt[i]) / s1m, e * (1.0 + k), -e * k, sqrt_a, s1m)
    return rows


def dpm_sde_coef_rows(alpha_bar, time_steps, t_start: int, order: int = 2, lower_order_final: bool = True, eta: float = 1.0) -> np.ndarray:
    """float64 ``[t_start + 1, 8]``: row i = the ``pf_dpm_sde_coef`` fields (s1m, sqrt_a, c_x, c_0, c_1, q_sqrt_a, q_s1m, sigma_n) of grid
    index i of the stochastic loop, ``dpm_coef_rows`` with
    ``c_x = (sigma_tgt / sigma_cur) * exp(-eta*h)``, ``E = -alpha_tgt * expm1(-(1 + eta)*h)`` in place of ``-alpha_tgt * expm1(-h)``, and
    ``sigma_n = sigma_tgt * sqrt(-expm1(-2*eta*h))``.  The rows that are first order are the same ones.  ``eta = 0``: the first seven
    columns are ``dpm_coef_rows`` bit for bit and ``sigma_n = 0``; ``eta = 1``: SDE-DPM-Solver++(2M).  On every row
    ``c_x*alpha_cur + c_0 + c_1 = alpha_tgt`` and ``c_x**2 * sigma_cur**2 + sigma_n**2 = sigma_tgt**2``."""
    eta = float(eta)
    if not (np.isfinite(eta) and eta >= 0.0):
        raise ValueError(f"dpm_sde_coef_rows: eta {eta}, expected a finite value >= 0")
    ab = np.asarray(alpha_bar, dtype=np.float64)
    ts = np.asarray(time_steps)[: t_start + 1]
    cur = ab[ts]
    tgt = np.concatenate([ab[0:1], ab[ts[:-1]]])
    lam = lambda a: 0.5 * np.log(a / (1.0 - a))
    h = lam(tgt) - lam(cur)
    rows = np.zeros((len(ts), 8), dtype=np.float64)
    for i in range(len(ts)):
        e = -np.sqrt(tgt[i]) * np.expm1(-((1.0 + eta) * h[i]))
        second = (order == 2 and i < t_start and h[i] != 0.0 and h[i + 1] != 0.0
                  and not (i == 0 and lower_order_final and len(ts) < 15))
        k = 0.5 * h[i] / h[i + 1] if second else 0.0           # 1 / (2r), r = h_{i+1} / h_i
        s1m, sqrt_a, s_tgt = np.sqrt(1.0 - cur[i]), np.sqrt(cur[i]), np.sqrt(1.0 - tgt[i])
        sigma_n = s_tgt * np.sqrt(max(0.0, -np.expm1(-2.0 * eta * h[i])))
        rows[i] = (s1m, sqrt_a, s_tgt / s1m * np.exp(-eta * h[i]), e * (1.0 + k), -e * k, sqrt_a, s1m, sigma_n)
    return rows


# why DPMSolverSampler at eta == 0 is not steered (the CLI says the same before it loads anything)
DPM_STEER_REFUSAL = "DPMSolverSampler is deterministic: copies of a survivor would never diverge (use SDFSampler, or DDIMSampler with eta > 0) or eta > 0"


class DPMSolverSampler(DiffusionSampler):
    """DPM-Solver++(2M) (Lu et al. 2022, algorithm 2; multistep, data prediction): a second-order solver of the probability-flow ODE that
    DDIM with eta = 0 solves to first order, at the same cost per step - one denoiser evaluation and ONE update kernel (``pf_dpm_step``).
    Not in the reference; it is driven like ``DDIMSampler`` (same ``paint`` / ``sample`` / ``q_sample`` / ``p_sample`` arguments, grid index
    i counts up with the time step).  The update's coefficients are computed here in float64 and rounded once (``dpm_coef_rows``); the
    previous step's data prediction lives in one buffer the kernel reads and overwrites.  Every ``paint()`` / ``sample()`` call starts a
    fresh history: its first step is first order and never reads the buffer.  With ``eta == 0`` (the default) it is deterministic: no
    step draws noise (a known region without a fixed ``orig_noise`` draws a fresh one per step, as DDIM's paint does).

    ``eta > 0``: the stochastic form (``dpm_sde_coef_rows``; ``eta = 1`` is SDE-DPM-Solver++(2M)) - every step of ``paint`` / ``sample``
    is ONE ``pf_dpm_sde_step`` launch and consumes one draw index, on a row whose ``sigma_n`` is 0 too, so that eager and captured loops
    count alike.  The draw is made in the kernel when ``_rng_ok`` holds, else it comes from ``randn`` as a tensor; a known region without
    ``orig_noise`` draws its fresh noise after the step's draw, as ``DDIMSampler._step`` does.  Such a loop can be steered (copies of a
    survivor diverge through their draws) and has no morph."""

    def __init__(self, model: LatentDiffusion, n_steps: int, discretize: str = "logsnr", order: int = 2, lower_order_final: bool = True,
                 is_show_image: bool = False, eta: float = 0.0, **kw):
        eta = float(eta)
        if not (np.isfinite(eta) and eta >= 0.0):
            raise ValueError(f"DPM-Solver++(2M): eta {eta}, expected a finite value >= 0")
        self.eta = eta                        # (before the base class looks at the steering setting)
        super().__init__(model, **kw)
        if int(order) not in (1, 2):
            raise ValueError(f"DPM-Solver++(2M): order {order!r}, expected 1 or 2")
        self.is_show_image = is_show_image
        self.n_steps = model.n_steps
        self.order, self.lower_order_final, self.discretize = int(order), bool(lower_order_final), discretize
        self._ab = model.alpha_bar.detach().cpu().double().numpy()
        self.time_steps = dpm_time_steps(self._ab, n_steps, discretize)
        self._rows = {}

    def _morph_refusal(self) -> Optional[str]:
        if self.eta > 0:
            return "DPMSolverSampler with eta > 0 draws noise in every step: the frames of such a loop are not a path (use eta 0, or DDIMSampler with eta 0)"
        return None             # no step draws noise: morph_from_noise is a path

    def _steer_refusal(self) -> Optional[str]:
        return DPM_STEER_REFUSAL if self.eta == 0 else super()._steer_refusal()

    def coef_rows(self, t_start: Optional[int] = None) -> np.ndarray:
        """float32 ``[t_start + 1, 7]``: the coefficient rows of a loop that starts at grid index ``t_start`` (default: the whole grid)."""
        t_start = len(self.time_steps) - 1 if t_start is None else int(t_start)
        if t_start not in self._rows:
            self._rows[t_start] = dpm_coef_rows(self._ab, self.time_steps, t_start, self.order, self.lower_order_final).astype(np.float32)
        return self._rows[t_start]

    def _coef(self, index: int, t_start: int) -> _lib.DpmCoef:
        return _lib.DpmCoef(*(float(v) for v in self.coef_rows(t_start)[index]))

    def sde_coef_rows(self, t_start: Optional[int] = None) -> np.ndarray:
        """float32 ``[t_start + 1, 8]``: ``coef_rows`` for this sampler's ``eta`` (``dpm_sde_coef_rows`` rounded once)."""
        t_start = len(self.time_steps) - 1 if t_start is None else int(t_start)
        if ("sde", t_start) not in self._rows:
            self._rows[("sde", t_start)] = dpm_sde_coef_rows(self._ab, self.time_steps, t_start, self.order, self.lower_order_final,
                                                             self.eta).astype(np.float32)
        return self._rows[("sde", t_start)]

    def _sde_coef(self, index: int, t_start: int) -> _lib.DpmSdeCoef:
        return _lib.DpmSdeCoef(*(float(v) for v in self.sde_coef_rows(t_start)[index]))

    def _coef_table(self, device, t_start: int):
        """([S, 7] fp32 rows of a loop starting at ``t_start`` - rows above it are zero and never read -, [S] int32 tau table) on the device;
        with ``eta > 0`` the rows are the 8 floats of ``sde_coef_rows``."""
        key = ("dpm_table", str(device), int(t_start))
        if key not in self._dev_cache:
            src = self.sde_coef_rows(t_start) if self.eta > 0 else self.coef_rows(t_start)
            rows = np.zeros((len(self.time_steps), src.shape[1]), dtype=np.float32)
            rows[: t_start + 1] = src
            self._dev_cache[key] = torch.from_numpy(rows).to(device)
        tk = ("dpm_taus", str(device))
        if tk not in self._dev_cache:
            self._dev_cache[tk] = torch.from_numpy(np.asarray(self.time_steps, dtype=np.int32)).to(device)
        return self._dev_cache[key], self._dev_cache[tk]

    def _paint_graph(self, x, cond, t_start, orig, mask, orig_noise, uncond_scale, uncond_cond, cond_concat):
        """All t_start+1 steps as replays of one captured step.  The captured update reads its coefficient row from a STATIC table buffer
        (its address is part of the graph): the rows of this call's ``t_start`` are copied into it with the other inputs, so one captured
        step serves loops of every length.  The history buffer is static too; row ``t_start`` is first order and does not read it."""
        lib, sde, off = self._lib, self.eta > 0, self._elem_offset(x.shape)
        rng = sde and self._rng_ok(x)              # eta > 0: one draw per step, in the update kernel or - bufs["_noise"] - by pf_randn_dev before it

        def update(bf, e_t, _table, st):
            hist = bf.get("_hist")
            if hist is None:                       # first (warm-up) run of the body, before the capture
                hist = bf["_hist"] = torch.empty_like(bf["x"])
            xb, known = bf["x"], dict(orig=bf["orig"], orig_noise=bf["orig_noise"], mask=bf["mask"])
            if not sde:
                _steps.dpm_step(lib, xb, e_t.contiguous(), xb, table=bf["dpm_table"], state=st, x0_prev=hist, x0_out=hist, **known)
            elif rng:
                _steps.dpm_sde_step(lib, xb, e_t.contiguous(), xb, table=bf["dpm_table"], state=st, x0_prev=hist, x0_out=hist,
                                    rng=(self.seed, 0, off), **known)
            else:
                nz = _steps.randn_dev(lib, bf["_noise"][0], self.seed, st, 0, off)
                _steps.dpm_sde_step(lib, xb, e_t.contiguous(), xb, table=bf["dpm_table"], state=st, x0_prev=hist, x0_out=hist, noise=nz, **known)

        table, taus = self._coef_table(x.device, t_start)
        inputs = dict(x=x, cond=cond, orig=orig, mask=mask, orig_noise=orig_noise, uncond_cond=uncond_cond, cond_concat=cond_concat,
                      dpm_table=table)
        if not sde:
            return self._replay_loop("dpm", inputs, table, taus, 0, 0, t_start + 1, t_start, uncond_scale, update)
        return self._replay_loop("dpm_sde", inputs, table, taus, 1, int(not rng), t_start + 1, t_start, uncond_scale, update)

    def _step(self, x, e_t, index, t_start, hist, orig=None, orig_noise=None, mask=None, temperature=1.0, repeat_noise=False):
        """Grid index ``index`` of a loop that started at ``t_start``; ``hist``: the history buffer (read unless the row is first order,
        then overwritten with this step's x0).  ``temperature`` / ``repeat_noise`` shape the noise of an ``eta > 0`` step, as in
        ``DDIMSampler._step``; at ``eta == 0`` there is none."""
        x, e_t = x.contiguous(), e_t.contiguous()
        out = torch.empty_like(x)
        if self.eta == 0:
            coef = self._coef(index, t_start)
            if orig is not None and orig_noise is None:      # DDIM's paint: a fresh q_sample noise per step (sampler_ddim.py:355-359)
                orig_noise = self.randn(orig.shape, x.device)
            return _steps.dpm_step(self._lib, x, e_t, out, coef=coef, x0_prev=hist, x0_out=hist, orig=orig, orig_noise=orig_noise, mask=mask), coef
        coef = self._sde_coef(index, t_start)
        orig, orig_noise, mask = (None if v is None else v.contiguous() for v in (orig, orig_noise, mask))
        if not repeat_noise and temperature == 1.0 and self._rng_ok(x, e_t, hist, orig, orig_noise, mask):
            draw = self._draws                               # the step's draw happens inside the update kernel, also when sigma_n == 0
            self._draws += 1
            if orig is not None and orig_noise is None:      # the fresh q_sample noise comes after the step's draw
                orig_noise = self.randn(orig.shape, x.device)
            _steps.dpm_sde_step(self._lib, x, e_t, out, coef=coef, x0_prev=hist, x0_out=hist, rng=(self.seed, draw, self._elem_offset(x.shape)),
                                orig=orig, orig_noise=orig_noise, mask=mask)
            return out, coef
        noise = self.randn((1, *x.shape[1:]) if repeat_noise else x.shape, x.device)      # one draw index per step, whatever sigma_n is
        if repeat_noise:
            noise = noise.expand_as(x).contiguous()
        if temperature != 1.0:
            noise = noise * temperature
        if orig is not None and orig_noise is None:
            orig_noise = self.randn(orig.shape, x.device)
        return _steps.dpm_sde_step(self._lib, x, e_t, out, coef=coef, x0_prev=hist, x0_out=hist, noise=noise, orig=orig, orig_noise=orig_noise,
                                   mask=mask), coef

    @torch.no_grad()
    def p_sample(self, x, c, t, step: int, index: int, *, repeat_noise=False, temperature=1.0, uncond_scale=1.0,
                 uncond_cond=None, cond_concat=None, prep: Optional[dict] = None, x0_prev: Optional[torch.Tensor] = None):
        """One step on its own; returns (x_prev, pred_x0, e_t) like ``DDIMSampler.p_sample``.  Without ``x0_prev`` the step is first order;
        with the ``pred_x0`` of the step at ``index + 1`` it is the second-order step of the full grid.  ``repeat_noise`` / ``temperature``
        shape the noise of an ``eta > 0`` step (through the tensor form, as ``DDIMSampler._step`` does); at ``eta == 0`` there is none."""
        e_t = self._eps(x, c, int(step), uncond_scale, uncond_cond, cond_concat, prep)
        full = len(self.time_steps) - 1
        second = x0_prev is not None and index < full
        hist = x0_prev.contiguous().clone() if second else torch.empty_like(e_t)     # read by a second-order row only; receives this step's x0
        x_prev, _ = self._step(x, e_t, index, full if second else index, hist, temperature=temperature, repeat_noise=repeat_noise)
        return x_prev, hist, e_t

    @torch.no_grad()
    def q_sample(self, x0, index: int, noise=None):
        row = self.coef_rows()[index]
        return _steps.q_sample(self, x0, noise, float(row[5]), float(row[6]), self._elem_offset(x0.shape))

    @torch.no_grad()
    def sample(self, shape, cond, repeat_noise=False, temperature=1.0, x_last=None, uncond_scale=1.0, uncond_cond=None,
               t_start: int = 0):
        """From noise (or ``x_last``) down the grid, skipping its ``t_start`` highest entries like ``DDIMSampler.sample``."""
        x = x_last if x_last is not None else self.randn(shape, cond.device)
        return self.paint(x, cond, len(self.time_steps) - 1 - int(t_start), uncond_scale=uncond_scale, uncond_cond=uncond_cond)

    @torch.no_grad()
    def paint(self, x, cond, t_start: int, *, orig=None, mask=None, orig_noise=None, uncond_scale: float = 1.0,
              uncond_cond=None, cond_concat=None, repaint_n: int = 1):
        x, t_start = x.contiguous(), int(t_start)
        if orig is not None:
            assert mask is not None
            orig, mask = orig.contiguous().float(), mask.contiguous().float()
            orig_noise = None if orig_noise is None else orig_noise.contiguous().float()
        if self.graph and self.noise_fn is None and (orig is None or orig_noise is not None) and self.on_step is None:
            return self._paint_graph(x, cond, t_start, orig, mask, orig_noise, uncond_scale, uncond_cond, cond_concat)
        prep = self.prepare(cond, uncond_scale=uncond_scale, uncond_cond=uncond_cond)
        hist = torch.empty_like(x)          # the previous step's x0; uninitialised: the first step does not read it
        steer = self._steer_begin(x, repaint_n)
        for i, index in enumerate(range(t_start, -1, -1)):
            step = int(self.time_steps[index])
            e_t = self._eps(x, cond, step, uncond_scale, uncond_cond, cond_concat, prep)
            if steer is not None and self._steered_at(steer, i, step, index == 0):
                # the history is a particle's own: it moves with x and e_t (not on the first step, where it is still uninitialised)
                x, e_t, *moved = self._steer_event(steer, x, e_t, self._t_of(step, self._eps_rows(x), x.device), i, step, [] if i == 0 else [hist])
                hist = moved[0] if moved else hist
            x, _ = self._step(x, e_t, index, t_start, hist, orig=orig, orig_noise=orig_noise, mask=mask)
            if self.on_step is not None:
                self.on_step(step, x)
        return x
